#!/usr/bin/env python3
"""Sniff-stage bench: gd_sniff_frames_device and gd_cache_invalidate_device on a device receive buffer.

Workload: --frames request frames of the encoder's bench shape (tools/bench_forward.py's build); a fraction of them
carry one CacheInvalidationHeader entry: 1 % in the first run, 100 % in the second.  The entries name --grains
distinct long-keyed grains, all cached, with an ActivationId that is not the cached one (every entry a hit that
stays: the cache is the same at every step).

Timed in the same run, --reps times over --steps steps, per kernel (gd_set_kernel_timing):
  (a) k_decode_frames on the buffer (gd_decode_frames_device: the parent's kernel over the same windows);
  (b) gd_sniff_frames_device: k_sniff_count, the scan, k_sniff_extract;
  (c) gd_cache_lookup's device kernels (k_cache_lookup, the scan, k_cache_touch, k_cache_advance,
      k_cache_count_access) on the batch's m entry keys;
  (d) gd_cache_invalidate_device on the same m keys: k_inv_find, k_inv_resolve, the scan, k_cache_touch,
      k_cache_advance, k_inv_apply.
Reported: medians over the repetitions, the spread ((max - min) / median), and the two ratios.

usage: python tools/bench_sniff.py [--frames 4194304] [--grains 65536] [--steps 10] [--warmup 3] [--reps 5]
                                   [--out profiles/sniff.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from orleans_amd import graindispatch as g  # noqa: E402
import bench_forward as BF  # noqa: E402

TCD = (3 << 56) + 77
SCAN = ("k_scan_reduce", "k_scan_down", "k_scan_single", "k_scan_partials")


def run_case(args, p_old, rng):
    n, dev = args.frames, torch.device("cuda:0")
    buf, off, bytes_in, m = BF.build(n, rng, p_old)
    # the entries' grains: N1 = entry index mod --grains (the GrainId's N1 lies 16 + 24 + 8 bytes into the frame)
    hdr = np.flatnonzero(buf[off.astype(np.int64) + 8] & 2)
    assert len(hdr) == m
    n1 = (np.arange(m, dtype=np.uint64) % np.uint64(args.grains))
    at = off[hdr].astype(np.int64) + 16 + 24 + 8
    buf[(at[:, None] + np.arange(8)).reshape(-1)] = n1.astype("<u8").view(np.uint8)
    keys = np.zeros((args.grains, 3), np.uint64)
    keys[:, 0], keys[:, 1], keys[:, 2] = 5, np.arange(args.grains), TCD
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    ids = rng.integers(1, 1 << 62, size=(1024, 3)).astype(np.uint64)
    e.activation_ids_set(np.arange(1024, dtype=np.uint32), ids)
    e.cache_configure(2 * args.grains, [], 8)
    e.cache_add(keys, rng.integers(0, 1024, size=args.grains), rng.integers(0, 8, size=args.grains),
                np.zeros(args.grains, np.int32))
    t = lambda a: torch.from_numpy(a).to(dev)
    d_buf, d_off = t(buf), t(off.view(np.int64))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    d = {"count": z(n, torch.int32), "ent_off": z(n + 1, torch.int32), "status": z(n, torch.uint8),
         "flags": z(n, torch.uint8), "ent_frame": z(m, torch.int32), "ent_silo": z((m, 6), torch.int32),
         "ent_grain": z((m, 3), torch.int64), "ent_ext_off": z(m, torch.int64), "ent_ext_len": z(m, torch.int32),
         "ent_act_id": z((m, 3), torch.int64)}
    d_out = {k: v.data_ptr() for k, v in d.items()}
    d_inv = z(m, torch.uint8)
    d_flags, d_tg = z(n, torch.int32), z((n, 3), torch.int64)
    ent_keys = np.zeros((m, 3), np.uint64)
    ent_keys[:, 0], ent_keys[:, 1], ent_keys[:, 2] = 5, n1, TCD
    s = torch.cuda.Stream(device=dev)
    e.set_stream(s.cuda_stream)

    decode = lambda: e.decode_frames_device(d_buf.data_ptr(), bytes_in, d_off.data_ptr(), n,
                                            {"flags": d_flags.data_ptr(), "target_grain": d_tg.data_ptr()})
    sniff = lambda: e.sniff_frames_device(d_buf.data_ptr(), bytes_in, d_off.data_ptr(), n, d_out, m)
    lookup = lambda: e.cache_lookup(ent_keys)
    inval = lambda: e.cache_invalidate_device(d["ent_grain"].data_ptr(), None, d["ent_act_id"].data_ptr(), m, None,
                                              d_inv.data_ptr())

    def kernels(run):
        e.set_kernel_timing(True)
        e.kernel_times_reset()
        for _ in range(args.steps):
            run()
        e.synchronize()
        kt = e.kernel_times()
        e.set_kernel_timing(False)
        us = {k: ms / args.steps * 1e3 for k, (cnt, ms) in kt.items()}
        out = {k: v for k, v in us.items() if v > 0 and not k.startswith("k_scan")}   # the names of earlier runs stay listed
        out["scan"] = sum(v for k, v in us.items() if k.startswith("k_scan"))
        out["total"] = sum(us.values())
        return out

    with torch.cuda.stream(s):
        sniff()
        e.synchronize()
        assert int(d["ent_off"][n].item()) == m and int((d["status"] == 2).sum().item()) == 0
        assert np.array_equal(d["ent_grain"].cpu().numpy().view(np.uint64), ent_keys)
        inval()
        e.synchronize()
        assert int((d_inv != g.GD_INV_KEPT).sum().item()) == 0
        for _ in range(args.warmup):
            decode(), sniff(), lookup(), inval()
        torch.cuda.synchronize()
        reps = [{"decode_us": kernels(decode), "sniff_us": kernels(sniff), "lookup_us": kernels(lookup),
                 "invalidate_us": kernels(inval)} for _ in range(args.reps)]
    e.close()
    med = lambda f: float(np.median([f(r) for r in reps]))
    spread = lambda f: (max(f(r) for r in reps) - min(f(r) for r in reps)) / med(f)
    stage = {k: {p: round(med(lambda r: r[k][p]), 1) for p in reps[0][k]} for k in reps[0]}
    count, dec = (lambda r: r["sniff_us"]["k_sniff_count"]), (lambda r: r["decode_us"]["k_decode_frames"])
    inv_t, look_t = (lambda r: r["invalidate_us"]["total"]), (lambda r: r["lookup_us"]["total"])
    return {"frames": n, "frames_with_one_entry": m, "bytes_in": bytes_in, "cached_grains": args.grains, **stage,
            "k_sniff_count_over_k_decode_frames": round(med(count) / med(dec), 3),
            "invalidate_over_lookup": round(med(inv_t) / med(look_t), 3),
            "spread": {"k_sniff_count": round(spread(count), 4), "k_decode_frames": round(spread(dec), 4),
                       "invalidate": round(spread(inv_t), 4), "lookup": round(spread(look_t), 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--grains", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sniff.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0025)
    rec = {"metric": "sniff stage: k_sniff_count against k_decode_frames on the same buffer, and InvalidateCacheEntry "
                     "against gd_cache_lookup's device kernels on the same keys; us a step, medians",
           "steps": args.steps, "reps": args.reps,
           "one_percent": run_case(args, 0.01, rng), "every_frame": run_case(args, 1.0, rng)}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
