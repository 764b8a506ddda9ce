#!/usr/bin/env python3
"""Turn completion and message pump on one MI355X.

--done completions over --acts contexts, the contexts uniform or Zipf(1.1).  Context state: every activation
Valid, 60% with a Running request (half of them read-only), num_running = the context's completions + 0 / 1,
1/16 of the completions flagged IS_RUNNING, 1% PUMP_ONLY.  Waiting lists: Poisson(1) entries a context (30%
read-only, 2% always-interleave) and one reentrant hot list of --hot entries on context 0, the Zipf head.
Timed, alternating within each round, inputs resident in HBM, device events on the handle's stream:
  complete         gd_turns_complete_device, context outputs only
  complete_starts  the same with n_started_by and start_pos
  merge            gd_wait_list_merge_device of the lists (less what the pump dequeued) with a gd_turns-shaped
                   batch of --done / 16 waiting messages
  copy             a device-to-device copy moving the bytes `complete` reads and writes (5 B a completion, 27 B a
                   context, 1 B a list entry): the stage's byte count, measured live -- not a bound on the
                   bucketing it reuses
Prints one JSON line; --out also writes it to a file.  No hardware-counter run is made here.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orleans_amd import graindispatch as g    # noqa: E402

BYTES_DONE, BYTES_CTX, BYTES_ENTRY = 4 + 1, (1 + 4 + 4 + 4) + (1 + 4 + 4 + 4 + 1), 1


def targets(kind, n, acts, dev, gen):
    if kind == "uniform":
        return torch.randint(0, acts, (n,), device=dev, generator=gen)
    w = 1.0 / torch.arange(1, acts + 1, device=dev, dtype=torch.float64) ** 1.1
    cdf = torch.cumsum(w / w.sum(), 0)
    return torch.searchsorted(cdf, torch.rand(n, device=dev, generator=gen, dtype=torch.float64)).clamp_(max=acts - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--done", type=int, default=1 << 24)
    ap.add_argument("--acts", type=int, default=1 << 20)
    ap.add_argument("--hot", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    A, N = args.acts, args.done
    rng = np.random.default_rng(0x9A11)
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    has = rng.random(A) < 0.6
    fl = (np.where(has, g.CTX_HAS_RUNNING, 0) | np.where(has & (rng.random(A) < 0.5), g.CTX_RUNNING_READ_ONLY, 0)).astype(np.uint8)
    fl[0] |= g.CTX_REENTRANT
    lens = rng.poisson(1.0, A)
    lens[0] = args.hot
    off = np.zeros(A + 1, np.int64)
    off[1:] = np.cumsum(lens)
    W = int(off[-1])
    u = rng.random(W)
    wf = (np.where(u < 0.3, g.MSG_READ_ONLY, 0) | np.where(u > 0.98, g.MSG_ALWAYS_INTERLEAVE, 0)).astype(np.uint8)
    d_fl = torch.from_numpy(fl).to(dev)
    d_off = torch.from_numpy(off.astype(np.int32)).to(dev)
    d_wf = torch.from_numpy(wf).to(dev)
    d_wm = torch.arange(W, dtype=torch.int32, device=dev)
    wait = e.wait_list_device(d_off.data_ptr(), d_wm.data_ptr(), d_wf.data_ptr())
    gen = torch.Generator(device=dev).manual_seed(0x9A12)
    u = torch.rand(N, device=dev, generator=gen)
    df = (torch.where(u < 1 / 16, g.DONE_IS_RUNNING, 0) | torch.where(u > 0.99, g.DONE_PUMP_ONLY, 0)).to(torch.uint8)

    i32 = lambda k: torch.empty(max(k, 1), dtype=torch.int32, device=dev)
    u8 = lambda k: torch.empty(max(k, 1), dtype=torch.uint8, device=dev)
    flo, nro, ndq, rpos, ev, nsb, sp, nsp = u8(A), i32(A), i32(A), i32(A), u8(A), i32(N), i32(W), i32(1)
    M = N // 16
    wperm, woff, mfl = i32(M), i32(A + 2), u8(M).zero_()
    cap = W + M
    n_off, n_msg, n_fl, n_tot = i32(A + 1), i32(cap), u8(cap), i32(1)
    stage_bytes = N * BYTES_DONE + A * BYTES_CTX + W * BYTES_ENTRY
    src, dst = u8(stage_bytes // 2), u8(stage_bytes // 2)
    stream = torch.cuda.Stream(dev)
    e.set_stream(stream.cuda_stream)
    P = lambda t: t.data_ptr()

    result = {"metric": "turn completion and message pump", "n_gpus": 1, "data": "synthetic",
              "config": {"done": N, "acts": A, "hot_list": args.hot, "list_entries": W, "merge_batch": M,
                         "rounds": args.rounds, "reps": args.reps, "stage_bytes": stage_bytes,
                         "pump_thin": 32, "counter_run": False}, "dist": {}}
    for kind in ("uniform", "zipf"):
        which = targets(kind, N, A, dev, gen)
        ctx = which.to(torch.int32)
        count = torch.bincount(which, minlength=A)
        d_nr = (count + torch.randint(0, 2, (A,), device=dev, generator=gen)).to(torch.int32)
        mkey = torch.where(torch.rand(M, device=dev, generator=gen) < 0.5, which[:M], A).to(torch.int32)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            e.bucket_device(P(mkey), M, A, P(wperm), P(woff))
        variants = {
            "complete": lambda: e.turns_complete_device(P(ctx), P(df), N, A, P(d_fl), P(d_nr), wait, W, P(flo), P(nro),
                                                        P(ndq), P(rpos), P(ev)),
            "complete_starts": lambda: e.turns_complete_device(P(ctx), P(df), N, A, P(d_fl), P(d_nr), wait, W, P(flo),
                                                               P(nro), P(ndq), P(rpos), P(ev), P(nsb), P(sp), P(nsp)),
            "merge": lambda: e.wait_list_merge_device(wait, P(ndq), A, P(wperm), P(woff), M, None, 0, P(mfl), None, None,
                                                      False, cap, P(n_off), P(n_msg), P(n_fl), P(n_tot)),
            "copy": lambda: dst.copy_(src),
        }
        times = {k: [] for k in variants}
        with torch.cuda.stream(stream):
            for f in variants.values():                # warm every shape (and the bucketing's variant choice)
                for _ in range(4):
                    f()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, f in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    for _ in range(args.reps):
                        f()
                    b.record(stream)
                    b.synchronize()
                    times[name].append(a.elapsed_time(b) / args.reps)
        # per-kernel times of the stage with starts, in a pass of its own (events around every launch)
        e.set_kernel_timing(True)
        e.kernel_times_reset()
        for _ in range(3):
            variants["complete_starts"]()
        torch.cuda.synchronize()
        kernels = {name: round(ms / 3, 4) for name, (launches, ms) in e.kernel_times().items()}
        e.set_kernel_timing(False)
        med = {k: float(np.median(v)) for k, v in times.items()}
        result["dist"][kind] = {
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
            "copy_over_complete": round(med["copy"] / med["complete"], 4),
            "hottest_context_share": round(float(count.max()) / N, 4),
            "n_start": int(nsp.item()), "dequeued": int(ndq.to(torch.int64).sum().item()),
            "events": torch.bincount(ev.to(torch.int64), minlength=8).tolist(),
            "merged_total": int(n_tot.item()),
            "complete_starts_kernel_ms": kernels,
        }
    d = result["dist"]
    result["zipf_over_uniform"] = {k: round(d["zipf"]["ms_median"][k] / d["uniform"]["ms_median"][k], 4)
                                   for k in ("complete", "complete_starts", "merge")}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    e.close()


if __name__ == "__main__":
    main()
