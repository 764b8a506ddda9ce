#!/usr/bin/env python3
"""Times the directory cache's maintainer on one GPU: 1,000,000 cached entries over 8 silos, the
default TTLs.  Event-timed medians of the scan at 0 %, 10 % and 100 % expired, gd_dir_lookup_many at 100K and 1M
items (beside gd_dir_lookup_tagged), and the apply of an all-SAME response and of one with 10 % UPDATED; the
classify pass beside k_cache_adjust over the same table (gd_dir_remove_silos of no silo).  The CPU baseline is
tests/_maintain_ref.py's array model on a 100K-entry slice (stated in the output).  Prints one JSON line per figure."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import oracle as o  # noqa: E402

S = 10_000_000


def stage_ms(e, name):
    t = e.kernel_times()
    return t[name][1] / max(1, t[name][0]) if name in t else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from orleans_amd import graindispatch as g
    N = a.entries
    tc = o.grain_type_code(o.PING_GRAIN_CLASS)
    keys = o.grain_keys(tc, np.arange(N, dtype=np.int64))
    silos = [(s.ip, s.port, s.gen) for s in o.bench_silos(8)]

    def fresh(touch_frac):
        e = g.GrainDispatch(device=0, table_capacity=1024)
        e.ring_set_silos("D", silos)
        e.cache_configure(N, [], 8)
        e.cache_clock_set(0)
        e.cache_add(keys, np.arange(N) % (1 << 20), np.arange(N) % 8, np.arange(N) % 1000)
        if touch_frac:
            e.cache_lookup(keys[: int(N * touch_frac)])
        return e

    def report(name, ms, **kw):
        print(json.dumps({"bench": "cache_maintain", "what": name, "entries": N, "median_ms": statistics.median(ms),
                          "runs_ms": [round(x, 4) for x in ms], **kw}), flush=True)

    for frac, label in ((0.0, "scan_0pct"), (0.1, "scan_10pct"), (1.0, "scan_100pct")):
        cls, lists = [], []
        for _ in range(a.reps):
            e = fresh(frac)
            e.set_kernel_timing(2)
            e.kernel_times_reset()
            # 0 %: nothing expired; else everything is, and the touched fraction is refreshed
            e.cache_scan(1 * S if frac == 0.0 else 31 * S)
            cls.append(stage_ms(e, "stage:cache_scan_classify"))
            lists.append(stage_ms(e, "stage:cache_scan_lists") or 0.0)
            if _ == 0:
                slots = e.cache_stats()["capacity"]
            e.close()
        report(label + ":classify", cls, slots=slots, bytes_read_a_slot=80, bytes_written_a_slot=4)
        report(label + ":lists", lists)

    adj = []
    for _ in range(a.reps):
        e = fresh(0.0)
        e.set_kernel_timing(1)
        e.kernel_times_reset()
        e.remove_silos([])
        adj.append(stage_ms(e, "k_cache_adjust"))
        e.close()
    report("k_cache_adjust(same table)", adj, bytes_read_a_slot=64)

    owner = g.GrainDispatch(device=0, table_capacity=1 << 21)
    owner.ring_set_silos("D", silos)
    owner.register(keys, np.arange(N) % (1 << 20), np.arange(N) % 8)
    for n in (100_000, N):
        _, _, tags, _ = owner.lookup_tagged(keys[:n])
        et = tags.copy()
        et[::3] += 1
        for timing, name, call in ((2, "stage:dir_lookup_many", lambda: owner.dir_lookup_many(keys[:n], et)),
                                   (1, "k_dir_lookup_tagged", lambda: owner.lookup_tagged(keys[:n]))):
            ms = []
            for _ in range(a.reps):
                owner.set_kernel_timing(timing)
                owner.kernel_times_reset()
                call()
                ms.append(stage_ms(owner, name))
            report(f"{name}:{n}", ms)
    owner.close()

    for upd, label in ((0.0, "apply_all_same"), (0.1, "apply_10pct_updated")):
        ms = []
        for _ in range(a.reps):
            e = fresh(1.0)
            _, lists = e.cache_scan(31 * S)
            k = np.concatenate([v[0] for v in lists.values()])
            kinds = np.full(len(k), g.GD_LM_SAME, dtype=np.uint8)
            kinds[: int(len(k) * upd)] = g.GD_LM_UPDATED
            t0 = time.perf_counter()
            e.cache_refresh_apply(32 * S, k, kinds, np.zeros(len(k)), np.ones(len(k)), np.zeros(len(k)))
            ms.append((time.perf_counter() - t0) * 1e3)
            e.close()
        report(label + " (host wall time, copies included)", ms)

    import _maintain_ref as M
    n = 100_000
    m = M.Arrays(n)
    kk = [tuple(int(x) for x in r) for r in keys[:n]]
    m.add(kk, [0] * n, [1] * n, [0] * n)
    m.lookup(kk)
    t0 = time.perf_counter()
    m.scan(kk, 31 * S, lambda k: 1, set())
    report("cpu_baseline: _maintain_ref.Arrays.scan, 100K entries, 100 % expired", [(time.perf_counter() - t0) * 1e3])


if __name__ == "__main__":
    main()
