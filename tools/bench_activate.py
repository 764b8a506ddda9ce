#!/usr/bin/env python3
"""Activation-stage bench: gd_activate_device and the receive -> activate -> turns chain on device arrays.

Workload: --messages messages against an activation directory of --acts activations, three in four of them Valid.
A fraction of the batch meets no Valid activation (GD_RECV_NULL_CONTEXT): 1 % in the first run, 100 % in the second.
Half of those carry IsNewPlacement and target ids the directory does not hold (two messages an id: one creates, one
finds); the other half target the activations that are not Valid.  The ids a step created are removed again before
the next one (gd_actdir_remove, not timed), so every step does the same work.

Timed in the same run, --reps times over --steps steps, per kernel (gd_set_kernel_timing):
  (a) k_receive on the batch (gd_receive_device, no bucketing);
  (b) gd_activate_device on its outputs: the k_actv_* kernels and the scans;
  (c) gd_receive_turns_device, all kernels;
  (d) gd_receive_activate_turns_device on the same batch, all kernels but the removal's.
Reported: medians over the repetitions, the spread ((max - min) / median), and the two ratios.

usage: python tools/bench_activate.py [--messages 4194304] [--acts 65536] [--steps 5] [--warmup 2] [--reps 3]
                                      [--out profiles/activate.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orleans_amd import graindispatch as g  # noqa: E402

TCD = (3 << 56) + 77
REMOVAL = ("k_ad_find", "k_unreg_commit")


def run_case(args, p_null, rng):
    n, G, dev = args.messages, args.acts, torch.device("cuda:0")
    ids = np.zeros((G, 3), np.uint64)
    ids[:, 0], ids[:, 1], ids[:, 2] = 7, np.arange(G), 1
    flags = np.where(np.arange(G) % 4 == 3, 0, g.ACTDIR_VALID).astype(np.uint8)
    invalid = np.flatnonzero(flags == 0)
    valid = np.flatnonzero(flags != 0)
    null = rng.random(n) < p_null
    newp = null & (rng.random(n) < 0.5)
    n_new_ids = max(1, int(newp.sum()) // 2)
    ta = np.empty((n, 3), np.uint64)
    ta[:] = ids[valid[rng.integers(0, len(valid), n)]]
    ta[null] = ids[invalid[rng.integers(0, len(invalid), int(null.sum()))]]
    new_ids = np.zeros((n_new_ids, 3), np.uint64)
    new_ids[:, 0], new_ids[:, 1], new_ids[:, 2] = 9, np.arange(n_new_ids), 1
    ta[newp] = new_ids[rng.integers(0, n_new_ids, int(newp.sum()))]
    tg = np.zeros((n, 3), np.uint64)
    tg[:, 1], tg[:, 2] = rng.integers(0, 1 << 20, n), TCD
    cap_new = int(newp.sum())
    n_ctx = G + cap_new
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    e.actdir_add(ids, np.arange(G), flags)
    t = lambda a: torch.from_numpy(a).to(dev)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    d_tg, d_ta, d_np = t(tg.view(np.int64)), t(ta.view(np.int64)), t(newp.astype(np.uint8))
    d_ctx, d_st, d_kind = z(n, torch.int32), z(n, torch.uint8), z(n, torch.uint8)
    d_ctx2, d_st2 = z(n, torch.int32), z(n, torch.uint8)
    d_new, d_gone, d_w = z(n, torch.int32), z(n, torch.int32), z(4, torch.int32)
    fl = np.zeros(n_ctx, np.uint8)
    fl[invalid] = 2                                          # GD_CTX_INVALID
    fl[G:] = 1                                               # GD_CTX_NOT_READY: the contexts offered
    d_fl, d_nr, d_rc = t(fl), z(n_ctx, torch.int32), z(n_ctx, torch.int32)
    d_turn, d_nro, d_run = z(n, torch.uint8), z(n_ctx, torch.int32), z(n_ctx, torch.int32)
    state = e.turn_state_device(d_fl.data_ptr(), d_nr.data_ptr(), d_rc.data_ptr())
    w = lambda k: d_w.data_ptr() + 4 * k
    act = e.activate_io_device(cap_new, d_kind.data_ptr(), w(2), ctx_base=G, d_new_placement=d_np.data_ptr(),
                               d_new_idx=d_new.data_ptr(), d_n_new=w(0), d_gone_idx=d_gone.data_ptr(), d_n_gone=w(1))
    s = torch.cuda.Stream(device=dev)
    e.set_stream(s.cuda_stream)

    receive = lambda: e.receive_device(d_tg.data_ptr(), d_ta.data_ptr(), None, n, n_ctx, d_ctx.data_ptr(), d_st.data_ptr(),
                                       None, None)

    def activate():
        e.activate_device(d_ctx.data_ptr(), d_st.data_ptr(), d_ta.data_ptr(), n, n_ctx, cap_new, d_kind.data_ptr(),
                          d_ctx2.data_ptr(), d_st2.data_ptr(), w(2), ctx_base=G, d_new_placement=d_np.data_ptr(),
                          d_new_idx=d_new.data_ptr(), d_n_new=w(0), d_gone_idx=d_gone.data_ptr(), d_n_gone=w(1))
        e.actdir_remove(new_ids)

    turns = lambda: e.receive_turns_device(d_tg.data_ptr(), d_ta.data_ptr(), None, n, n_ctx, d_ctx2.data_ptr(),
                                           d_st2.data_ptr(), None, None, None, None, None, None, state,
                                           d_turn.data_ptr(), d_nro.data_ptr(), d_run.data_ptr())

    def chain():
        e.receive_activate_turns_device(d_tg.data_ptr(), d_ta.data_ptr(), None, n, n_ctx, d_ctx2.data_ptr(),
                                        d_st2.data_ptr(), None, None, None, None, None, None, state, d_turn.data_ptr(),
                                        d_nro.data_ptr(), d_run.data_ptr(), act)
        e.actdir_remove(new_ids)

    def kernels(run):
        e.set_kernel_timing(True)
        e.kernel_times_reset()
        for _ in range(args.steps):
            run()
        e.synchronize()
        kt = e.kernel_times()
        e.set_kernel_timing(False)
        us = {k: ms / args.steps * 1e3 for k, (cnt, ms) in kt.items() if k not in REMOVAL}
        out = {k: v for k, v in us.items() if v > 0 and not k.startswith("k_scan")}   # earlier runs' names stay listed
        out["scan"] = sum(v for k, v in us.items() if k.startswith("k_scan"))
        out["total"] = sum(us.values())
        return out

    with torch.cuda.stream(s):
        receive()
        activate()
        e.synchronize()
        words = d_w.cpu().numpy()
        kinds = np.bincount(d_kind.cpu().numpy(), minlength=7)
        assert int(words[2]) == cap_new and int(words[0]) == len(np.unique(ta[newp][:, 1])), words
        assert kinds[g.GD_ACTV_NONE] == n - int(null.sum()) and kinds[g.GD_ACTV_HOST] == 0, kinds
        for _ in range(args.warmup):
            receive(), activate(), turns(), chain()
        torch.cuda.synchronize()
        reps = []
        for _ in range(args.reps):
            r = {"receive_us": kernels(receive)}
            receive()
            r.update(activate_us=kernels(activate), receive_turns_us=kernels(turns), chain_us=kernels(chain))
            reps.append(r)
    e.close()
    med = lambda f: float(np.median([f(r) for r in reps]))
    spread = lambda f: (max(f(r) for r in reps) - min(f(r) for r in reps)) / med(f)
    stage = {k: {p: round(med(lambda r: r[k].get(p, 0.0)), 1) for p in reps[0][k]} for k in reps[0]}
    rcv, actv = (lambda r: r["receive_us"]["k_receive"]), (lambda r: r["activate_us"]["total"])
    rt, ch = (lambda r: r["receive_turns_us"]["total"]), (lambda r: r["chain_us"]["total"])
    return {"messages": n, "null_context": int(null.sum()), "new_placements": cap_new, "created": int(words[0]),
            "activations": G, **stage,
            "activate_over_k_receive": round(med(actv) / med(rcv), 3),
            "chain_over_receive_turns": round(med(ch) / med(rt), 3),
            "spread": {"k_receive": round(spread(rcv), 4), "activate": round(spread(actv), 4),
                       "receive_turns": round(spread(rt), 4), "chain": round(spread(ch), 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=1 << 22)
    ap.add_argument("--acts", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "activate.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0x5EED0026)
    rec = {"metric": "activation stage: gd_activate_device's kernels against k_receive on the same batch, and the "
                     "receive -> activate -> turns chain against gd_receive_turns_device; us a step, medians",
           "steps": args.steps, "reps": args.reps,
           "one_percent": run_case(args, 0.01, rng), "every_message": run_case(args, 1.0, rng)}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
