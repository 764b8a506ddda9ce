#!/usr/bin/env python3
"""Turn admission of a received batch on one MI355X.

A silo hosting --acts activations receives --msgs messages, TargetActivation uniform over the activations or
Zipf(1.1).  Context state: every activation Valid, 30% with a Running request (half of them read-only,
num_running 1), 5% reentrant; messages 30% read-only, 2% always-interleave, 1% expired, 20% responses.
Timed, alternating within each round, inputs resident in HBM, device events on the handle's stream:
  receive        gd_receive_device (per-context bucketing, no limits)
  receive_turns  gd_receive_turns_device: the same, then the turn stage with its lists
  turns          gd_turns_device without lists (k_turn_init, k_turn_classify, k_turn_decide, k_turn_finish)
  turns_lists    gd_turns_device with start_idx and the wait lists (one bucketing more)
  copy           a device-to-device copy moving the bytes the `turns` kernels stream per message: the stage's
                 byte bound, measured live
Prints one JSON line; --out also writes it to a file.
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

CAT_GRAIN = 3
# k_turn_classify streams ctx 4 + status 1 + direction 1 + ttl 8 + forward count 1 + flags 1 and writes 1;
# k_turn_decide streams ctx 4 + turn 1 and rewrites at most 1 (context gathers not counted)
STAGE_BYTES = 16 + 1 + 5 + 1


def targets(kind, n, acts, dev, gen):
    if kind == "uniform":
        return torch.randint(0, acts, (n,), device=dev, generator=gen)
    w = 1.0 / torch.arange(1, acts + 1, device=dev, dtype=torch.float64) ** 1.1
    cdf = torch.cumsum(w / w.sum(), 0)
    return torch.searchsorted(cdf, torch.rand(n, device=dev, generator=gen, dtype=torch.float64)).clamp_(max=acts - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=1 << 24)
    ap.add_argument("--acts", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    A, N = args.acts, args.msgs
    rng = np.random.default_rng(0x7A11)
    ids = np.zeros((A, 3), np.uint64)
    ids[:, 0] = rng.integers(0, 1 << 63, size=A, dtype=np.int64).astype(np.uint64)
    ids[:, 1] = rng.integers(0, 1 << 63, size=A, dtype=np.int64).astype(np.uint64)
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    assert e.actdir_add(ids, np.arange(A, dtype=np.uint32), np.full(A, g.ACTDIR_VALID, np.uint8)).all()
    has = rng.random(A) < 0.3
    fl = (np.where(has, g.CTX_HAS_RUNNING, 0) | np.where(has & (rng.random(A) < 0.5), g.CTX_RUNNING_READ_ONLY, 0) |
          np.where(rng.random(A) < 0.05, g.CTX_REENTRANT, 0)).astype(np.uint8)
    d_fl = torch.from_numpy(fl).to(dev)
    d_nr = torch.from_numpy(has.astype(np.int32)).to(dev)
    d_rc = torch.zeros(A, dtype=torch.int32, device=dev)
    state = e.turn_state_device(d_fl.data_ptr(), d_nr.data_ptr(), d_rc.data_ptr(), 0, 0, 2, False)

    tc = g.calculate_id_hash("BenchmarkGrains.Ping.PingGrain")
    tcd = (CAT_GRAIN << 56) + (tc & 0x00FFFFFFFFFFFFFF)
    gen = torch.Generator(device=dev).manual_seed(0x7A12)
    d_ids = torch.from_numpy(ids.view(np.int64)).to(dev)
    u = torch.rand(N, device=dev, generator=gen)
    direction = torch.where(u < 0.2, 1, 0).to(torch.uint8)
    u = torch.rand(N, device=dev, generator=gen)
    mf = (torch.where(u < 0.3, g.MSG_READ_ONLY, 0) | torch.where(u > 0.98, g.MSG_ALWAYS_INTERLEAVE, 0)).to(torch.uint8)
    ttl = torch.where(torch.rand(N, device=dev, generator=gen) < 0.01, 0, g.TTL_NONE)
    fwd = torch.zeros(N, dtype=torch.uint8, device=dev)
    tg = torch.zeros((N, 3), dtype=torch.int64, device=dev)
    tg[:, 2] = tcd

    i32 = lambda k: torch.empty(max(k, 1), dtype=torch.int32, device=dev)
    u8 = lambda k: torch.empty(max(k, 1), dtype=torch.uint8, device=dev)
    ctx, st, perm, off = i32(N), u8(N), i32(N), i32(A + 3)
    turn, nro, run, start, ns, wp, wo = u8(N), i32(A), i32(A), i32(N), i32(1), i32(N), i32(A + 2)
    half = N * STAGE_BYTES // 2
    src, dst = u8(half), u8(half)
    stream = torch.cuda.Stream(dev)
    e.set_stream(stream.cuda_stream)
    P = lambda t: t.data_ptr()

    result = {"metric": "turn admission of a received batch", "n_gpus": 1, "data": "synthetic",
              "config": {"msgs": N, "acts": A, "rounds": args.rounds, "reps": args.reps,
                         "stage_bytes_per_msg": STAGE_BYTES}, "dist": {}}
    for kind in ("uniform", "zipf"):
        which = targets(kind, N, A, dev, gen)
        tg[:, 1] = which
        ta = d_ids[which].contiguous()
        torch.cuda.synchronize()
        variants = {
            "receive": lambda: e.receive_device(P(tg), P(ta), P(direction), N, A, P(ctx), P(st), P(perm), P(off)),
            "receive_turns": lambda: e.receive_turns_device(
                P(tg), P(ta), P(direction), N, A, P(ctx), P(st), P(perm), P(off), P(ttl), P(fwd), P(mf), None, state,
                P(turn), P(nro), P(run), P(start), P(ns), P(wp), P(wo)),
            "turns": lambda: e.turns_device(P(ctx), P(st), P(direction), P(ttl), P(fwd), P(mf), None, None, N, A, state,
                                            P(turn), P(nro), P(run)),
            "turns_lists": lambda: e.turns_device(P(ctx), P(st), P(direction), P(ttl), P(fwd), P(mf), None, None, N, A,
                                                  state, P(turn), P(nro), P(run), P(start), P(ns), P(wp), P(wo)),
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
        counts = torch.bincount(turn.to(torch.int64), minlength=10).tolist()
        # per-kernel times of the stage with lists, in a pass of its own (events around every launch)
        e.set_kernel_timing(True)
        e.kernel_times_reset()
        for _ in range(3):
            variants["turns_lists"]()
        torch.cuda.synchronize()
        kernels = {name: round(ms / 3, 4) for name, (launches, ms) in e.kernel_times().items()}
        e.set_kernel_timing(False)
        med = {k: float(np.median(v)) for k, v in times.items()}
        result["dist"][kind] = {
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
            "turn_stage_added_ms": round(med["receive_turns"] - med["receive"], 4),
            "turns_frac_of_byte_bound": round(med["copy"] / med["turns"], 4),
            "hottest_context_share": round(float(torch.bincount(which, minlength=A).max()) / N, 4),
            "turn_counts": counts,
            "turns_lists_kernel_ms": kernels,
        }
    d = result["dist"]
    result["zipf_over_uniform"] = {k: round(d["zipf"]["ms_median"][k] / d["uniform"]["ms_median"][k], 4)
                                   for k in ("receive", "receive_turns", "turns", "turns_lists")}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    e.close()


if __name__ == "__main__":
    main()
