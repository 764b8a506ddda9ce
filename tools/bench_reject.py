#!/usr/bin/env python3
"""Forward-rejection bench: gd_forward_reject_frames_device on a device receive buffer.

Workload: the forward writer's bench frames (tools/bench_forward.py: headerLength 122, all Request, bodies 0..63 B,
1 % with one old CacheInvalidationHeader entry).  The frames carry no ForwardCount field, so with
max_forward_count 0 every one of them stands at the limit, and with max_forward_count 1 every one may forward.

Timed in the same run, --reps times over, per kernel:
  dense   every frame FORWARD at ForwardCount == max_forward_count with an old address (one entry appended, empty
          bodies): (a) gd_respond_frames_device under GD_OPT_WALK_INVALIDATION 1, kind REJECTION, on the same frames;
          (b) gd_forward_reject_frames_device.  Each writer's cost is per byte it wrote.
  sparse  1 % of the frames FORWARD (at the limit), the rest not: (c) gd_forward_reject_frames_device, the stage and
          its planner; (d) gd_forward_frames_device's planner on the same batch (it marks the 1 % REJECT).
  may     every frame FORWARD and below the limit (max_forward_count 1): the planner walks every frame and writes
          nothing: (e) this stage's planner, (f) the forward writer's (which then writes them all).
Reported: the median of the repetitions, the writers in ps per output byte and their run-to-run spread
((max - min) / median over the repetitions).

usage: python tools/bench_reject.py [--frames 4194304] [--steps 10] [--warmup 3] [--reps 5]
                                    [--out profiles/reject.json]
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
import bench_encode as BE  # noqa: E402
import bench_forward as BF  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reject.json"))
    args = ap.parse_args()
    n = args.frames
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0x5EED0028)
    buf, off, bytes_in, n_old = BF.build(n, rng)
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    e.set_option(g.OPT_WALK_INVALIDATION, 1)                           # for (a): this stage walks the field anyway
    e.encode_configure(BE.SILOS, ["BenchmarkGrains.Ping.PingGrain"])
    e.respond_configure(["Forwarding failed: tried to forward the message 2 times after a non-existent activation"])
    ids = rng.integers(1, 1 << 62, size=(BE.N_ACT, 3)).astype(np.uint64)
    e.activation_ids_set(np.arange(BE.N_ACT, dtype=np.uint32), ids)
    t = lambda a: torch.from_numpy(a).to(dev)
    d_buf, d_off = t(buf), t(off.view(np.int64))
    d_all = torch.ones(n, dtype=torch.uint8, device=dev)               # GD_FWD_FORWARD
    d_rej = torch.full((n,), 2, dtype=torch.uint8, device=dev)         # GD_RSP_REJECTION
    d_one = t((rng.random(n) < 0.01).astype(np.uint8))                 # 1 % FORWARD
    d_old = t(rng.integers(0, BE.N_ACT, size=n).astype(np.int32))
    d_info = torch.zeros(n, dtype=torch.int32, device=dev)
    cap = bytes_in + 300 * n + 64
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_est = torch.empty(n, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    e.set_stream(s.cuda_stream)
    db = lambda kind, max_fc: {"buf": d_buf.data_ptr(), "buf_len": bytes_in, "frame_off": d_off.data_ptr(),
                               "kind": kind.data_ptr(), "old_act": d_old.data_ptr(), "max_forward_count": max_fc,
                               "local_silo": 0}

    def respond():
        e.respond_frames_device(d_buf.data_ptr(), bytes_in, d_off.data_ptr(), n, d_rej.data_ptr(), None, None,
                                d_info.data_ptr(), None, None, None, d_out.data_ptr(), cap, d_out_off.data_ptr(),
                                d_est.data_ptr())

    def reject(kind, max_fc):
        return lambda: e.forward_reject_frames_device(db(kind, max_fc), n, d_info.data_ptr(), None, None, None,
                                                      d_out.data_ptr(), cap, d_out_off.data_ptr(), d_est.data_ptr())

    def forward(kind, max_fc):
        return lambda: e.forward_frames_device(db(kind, max_fc), n, None, None, None, None, None, None,
                                               d_out.data_ptr(), cap, d_out_off.data_ptr(), d_est.data_ptr(), None)

    def kernels(run, names):
        e.set_kernel_timing(True)
        e.kernel_times_reset()
        for _ in range(args.steps):
            run()
        e.synchronize()
        kt = e.kernel_times()
        e.set_kernel_timing(False)
        us = {k: ms / args.steps * 1e3 for k, (cnt, ms) in kt.items()}
        scan = sum(v for k, v in us.items() if k.startswith("k_scan") or k in ("k_enc_lens", "k_enc_finish"))
        plan = sum(v for k, v in us.items() if k.startswith(names[0]))
        return {"plan": plan, "scan": scan, "write": us[names[1]], "total": plan + scan + us[names[1]],
                "bytes_out": int(d_out_off[n].item())}

    runs = {"dense_respond": (respond, ("k_rsp_plan", "k_rsp_write")),
            "dense_reject": (reject(d_all, 0), ("k_rej_plan", "k_rej_write")),
            "sparse_reject": (reject(d_one, 0), ("k_rej_plan", "k_rej_write")),
            "sparse_forward": (forward(d_one, 0), ("k_fwd_plan", "k_fwd_write")),
            "may_reject": (reject(d_all, 1), ("k_rej_plan", "k_rej_write")),
            "may_forward": (forward(d_all, 1), ("k_fwd_plan", "k_fwd_write"))}
    with torch.cuda.stream(s):
        runs["dense_reject"][0]()
        e.synchronize()
        assert int((d_est != 0).sum().item()) == 0                     # every frame GD_FWDREJ_OK
        for _ in range(args.warmup):
            for run, _ in runs.values():
                run()
        torch.cuda.synchronize()
        reps = [{k: kernels(run, names) for k, (run, names) in runs.items()} for _ in range(args.reps)]
    e.close()
    med = lambda f: float(np.median([f(r) for r in reps]))
    parts = ("plan", "scan", "write", "total")
    stage = {k: {p: round(med(lambda r: r[k][p]), 1) for p in parts} for k in runs}
    outs = {k: reps[0][k]["bytes_out"] for k in runs}
    ps = {k: med(lambda r: r[k]["write"]) * 1e6 / outs[k] for k in ("dense_respond", "dense_reject")}
    spread = {k: (max(r[k]["write"] for r in reps) - min(r[k]["write"] for r in reps)) / med(lambda r: r[k]["write"])
              for k in ps}
    rec = {"metric": "forward rejections: the writer against k_rsp_write on the same frames (dense), the stage and "
                     "its planner against the forward writer's planner (sparse, may-forward); kernel times in us",
           "frames": n, "frames_with_an_old_entry": n_old, "bytes_in": bytes_in, "plan_record_bytes": 192,
           "sparse_forward_frames": int(d_one.sum().item()), "steps": args.steps, "reps": args.reps,
           "bytes_out": outs, "us": stage,
           "write_ps_per_output_byte": {"k_rsp_write": round(ps["dense_respond"], 3),
                                        "k_rej_write": round(ps["dense_reject"], 3)},
           "write_spread": {"k_rsp_write": round(spread["dense_respond"], 4),
                            "k_rej_write": round(spread["dense_reject"], 4)},
           "rej_over_rsp_per_byte": round(ps["dense_reject"] / ps["dense_respond"], 3),
           "repetitions": [{k: {q: (round(x, 1) if isinstance(x, float) else x) for q, x in v.items()}
                            for k, v in r.items()} for r in reps]}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
