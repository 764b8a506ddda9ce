#!/usr/bin/env python3
"""A/B for the batched placement on the cfg 2 shape: 16M messages over 2^20 grains, device-resident
keys and outputs, with 0 %, 0.1 % and 1 % of the grains unregistered when the batch arrives.  Per case, one step of

  place     gd_route_place_bucket_device (GD_PLACE_HASH): one call, the batch addressed and bucketed
  baseline  (a) gd_route_bucket_device on the same handle with every grain registered: what a batch costs when
            nothing is cold
  today     (b) the host's way without the call: gd_route_device, the 16-MB status read-back, the misses' keys
            read back, deduplicated with numpy (first message of a grain wins), gd_dir_register,
            gd_route_bucket_device

Wall time around each step including its last synchronisation; the steps of a round are interleaved, and between
steps (outside the timed region) the cold grains are unregistered again / registered for the baseline, so every
step sees the same misses.  Medians, minima and maxima over the rounds go to profiles/place_ab.json.

usage: python tools/place_ab.py [--rounds 9] [--log2-n 24] [--out profiles/place_ab.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orleans_amd import graindispatch as g  # noqa: E402

SILOS = [(f"10.0.0.{i + 1}", 11111, 1) for i in range(8)]
MISS = g.ROUTE_MISS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--log2-n", type=int, default=24)
    ap.add_argument("--log2-grains", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_ab.json"))
    args = ap.parse_args()
    N, G = 1 << args.log2_n, 1 << args.log2_grains
    n_act = G + (1 << 18)                      # room for the sparse numbers of a 1 % batch
    dev = torch.device("cuda:0")
    tc = g.calculate_id_hash("BenchmarkGrains.Ping.PingGrain")
    tcd = (3 << 56) + (tc & 0x00FFFFFFFFFFFFFF)
    allk = np.zeros((G, 3), dtype=np.uint64)
    allk[:, 1] = np.arange(G, dtype=np.uint64)
    allk[:, 2] = np.uint64(tcd)
    all_acts = np.arange(G, dtype=np.uint32)
    e = g.GrainDispatch(device=0, table_capacity=2 * G)
    e.ring_set_silos("D", SILOS)
    e.place_configure(SILOS)
    owner = e.ring_owner(allk)
    e.register(allk, all_acts, owner)
    rng = np.random.default_rng(0x5EED0002)
    ids = rng.integers(0, G, size=N)
    d_keys = torch.from_numpy(allk[ids].view(np.int64)).to(dev)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    d_silo, d_act, d_perm, d_new, d_off = i32(N), i32(N), i32(N), i32(N), i32(n_act + 2)
    d_st = torch.empty(N, dtype=torch.uint8, device=dev)
    d_pl = torch.empty(N, dtype=torch.uint8, device=dev)
    cold = {s: np.sort(rng.choice(G, size=int(round(G * s)), replace=False)) for s in (0.0, 0.001, 0.01)}

    def now_acts(c):
        return e.lookup(allk[c])[0]

    def make_cold(c):                          # the grains of c unregistered, whatever holds them now
        if len(c):
            e.unregister(allk[c], now_acts(c))
        e.synchronize()
        torch.cuda.synchronize()

    def make_warm(c):                          # ... registered under their first numbers again
        if len(c):
            e.unregister(allk[c], now_acts(c))
            e.register(allk[c], all_acts[c], owner[c])
        e.synchronize()
        torch.cuda.synchronize()

    def step_place():
        return e.route_place_device(d_keys.data_ptr(), N, None, g.PLACE_HASH, None, G, d_silo.data_ptr(),
                                    d_act.data_ptr(), d_st.data_ptr(), d_pl.data_ptr(), d_new.data_ptr(), n_act,
                                    d_perm.data_ptr(), d_off.data_ptr())

    def step_baseline():
        e.route_bucket_device(d_keys.data_ptr(), N, n_act, d_silo.data_ptr(), d_act.data_ptr(), d_st.data_ptr(),
                              d_perm.data_ptr(), d_off.data_ptr())

    def step_today():
        e.route_device(d_keys.data_ptr(), N, d_silo.data_ptr(), d_act.data_ptr(), d_st.data_ptr())
        e.synchronize()
        idx = np.flatnonzero(d_st.cpu().numpy() == MISS)
        if len(idx):
            mk = d_keys.view(N, 3)[torch.from_numpy(idx).to(dev)].cpu().numpy().view(np.uint64)
            _, first = np.unique(np.ascontiguousarray(mk).view("V24").ravel(), return_index=True)
            first.sort()                       # batch order: the first message of a grain places it
            uk = mk[first]
            e.register(uk, G + np.arange(len(uk), dtype=np.uint32), (uk[:, 1] % 8).astype(np.uint32))
        step_baseline()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        e.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    res = {}
    counts = {}
    for rnd in range(args.rounds + 1):         # round 0 warms every path (allocations, measured choices)
        for share, c in cold.items():
            for name, prep, fn in (("baseline", make_warm, step_baseline), ("place", make_cold, step_place),
                                   ("today", make_cold, step_today)):
                prep(c)
                ms, r = timed(fn)
                if rnd:
                    res.setdefault(f"{share:g}", {}).setdefault(name, []).append(ms)
                if name == "place":
                    counts[f"{share:g}"] = {"n_new": r[0], "n_proposed": r[1], "cold_grains": int(len(c))}
    out = {"shape": {"messages": N, "grains": G, "n_act": n_act, "rounds": args.rounds}, "cases": {}}
    for share, by in res.items():
        out["cases"][share] = dict(counts[share])
        for name, v in by.items():
            out["cases"][share][name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4),
                                         "max_ms": round(max(v), 4), "samples_ms": [round(x, 4) for x in v]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for share, cse in out["cases"].items():
        print(share, {k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in cse.items()})
    e.close()


if __name__ == "__main__":
    main()
