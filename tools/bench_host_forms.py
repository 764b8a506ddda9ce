#!/usr/bin/env python3
"""Host-pointer forms of the batched stages on one MI355X: wall time per call, PCIe copies and the
closing synchronisation included.

After one warm-up call, --calls calls each of turns, turns_complete, wait_list_merge, callbacks_respond,
send_queues and encode_frames at --n messages from pageable numpy arrays; the median per call in ms.  Only the
public Python binding is used, so the same file measures another build of the library (GRAINDISPATCH_LIB).
callbacks_respond fires every id of its batch, so the ids are added again (untimed) before each timed call.
Prints one JSON line; --out also appends it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from orleans_amd import graindispatch as g  # noqa: E402
import bench_encode as BE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--acts", type=int, default=1 << 16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, A = args.n, args.acts
    rng = np.random.default_rng(0x405F)
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    e.send_configure([g.silo_consistent_hash(*s) for s in BE.SILOS], 16)
    e.callbacks_configure(2 * n)
    e.encode_configure(BE.SILOS, ["BenchmarkGrains.Ping.PingGrain"])
    e.activation_ids_set(np.arange(BE.N_ACT, dtype=np.uint32), rng.integers(1, 1 << 62, size=(BE.N_ACT, 3)).astype(np.uint64))

    ctx = rng.integers(0, A, n).astype(np.uint32)
    has = rng.random(A) < 0.6
    fl = np.where(has, g.CTX_HAS_RUNNING, 0).astype(np.uint8)
    nr = has.astype(np.uint32)
    rc = rng.integers(0, 8, A).astype(np.uint32)
    mf = np.where(rng.random(n) < 0.3, g.MSG_READ_ONLY, 0).astype(np.uint8)
    woff = np.zeros(A + 1, np.uint32)
    woff[1:] = np.cumsum(rng.poisson(1.0, A))
    W = int(woff[-1])
    wfl = np.where(rng.random(W) < 0.3, g.MSG_READ_ONLY, 0).astype(np.uint8)
    wmsg = np.arange(W, dtype=np.uint32)
    turn, _, _, _, wperm, wpoff = e.turns(ctx, A, fl, nr, rc, msg_flags=mf)
    nr_done = nr + np.bincount(ctx, minlength=A).astype(np.uint32)     # every completion has its running request
    ndq = e.turns_complete(ctx, A, fl, nr_done, woff, wfl)[2]
    ids = np.arange(1, n + 1, dtype=np.int64)
    handles, deadlines = np.arange(n, dtype=np.uint32), np.full(n, 1 << 40, np.int64)
    silo = rng.integers(0, len(BE.SILOS), n).astype(np.uint32)
    rstat = np.zeros(n, np.uint8)
    buf, off, _ = BE.build(n, rng)
    act = rng.integers(0, BE.N_ACT, n).astype(np.uint32)
    out = np.empty(len(buf) + 64 * n, np.uint8)

    forms = {
        "turns": lambda: e.turns(ctx, A, fl, nr, rc, msg_flags=mf),
        "turns_complete": lambda: e.turns_complete(ctx, A, fl, nr_done, woff, wfl),
        "wait_list_merge": lambda: e.wait_list_merge(A, woff, wmsg, wfl, ndq, wperm, wpoff, msg_flags=mf),
        "callbacks_respond": lambda: e.callbacks_respond(ids),
        "send_queues": lambda: e.send_queues(silo, rstat),
        "encode_frames": lambda: e.encode_frames(buf, off, silo, act, rstat, out=out),
    }
    before = {"callbacks_respond": lambda: e.callbacks_add(ids, handles, deadlines)}
    ms = {}
    for name, f in forms.items():
        times = []
        for i in range(args.calls + 1):                 # call 0 warms the pool and the measured choices
            before.get(name, lambda: None)()
            t0 = time.perf_counter()
            f()
            times.append((time.perf_counter() - t0) * 1e3)
        ms[name] = round(float(np.median(times[1:])), 4)
    e.close()
    line = json.dumps({"metric": "host-pointer forms, wall ms per call (median)", "label": args.label, "n": n,
                       "acts": A, "calls": args.calls, "wait_entries": W, "frame_bytes": len(buf), "ms_median": ms})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
