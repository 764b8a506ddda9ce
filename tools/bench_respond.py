#!/usr/bin/env python3
"""Response-writer bench: gd_respond_frames_device on a device receive buffer.

Workload: --frames request frames of the encoder's bench shape (tools/bench_encode.py: headerLength 122, all
Request, bodies 0..63 B); 25 % are answered with an Overloaded rejection carrying a 40-byte RejectionInfo, the
rest with a Success response; the answers' bodies are 0..63 B.

Timed in the same run, --reps times over:
  (a) a device-to-device copy that moves the response stage's traffic (it copies (bytes in + bytes out) / 2);
  (b) gd_encode_frames_device on the same frames, per kernel -- the yardstick;
  (c) gd_respond_frames_device, per kernel.
Reported: the median of the repetitions, each kernel of (c) as a ratio to (a) and to its counterpart in (b), the
writers' cost per output byte, and the run-to-run spread of (b)'s writer ((max - min) / median over the
repetitions), which is the margin of the comparison k_rsp_write <= k_enc_write per output byte.

usage: python tools/bench_respond.py [--frames 4194304] [--steps 10] [--warmup 3] [--reps 5]
                                     [--out profiles/respond.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "respond.json"))
    args = ap.parse_args()
    n = args.frames
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0x5EED0022)
    buf, off, bytes_in = BE.build(n, rng)
    enc_out = bytes_in + 52 * n
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    e.encode_configure(BE.SILOS, ["BenchmarkGrains.Ping.PingGrain"])
    e.respond_configure(["i" * 40])
    ids = rng.integers(1, 1 << 62, size=(BE.N_ACT, 3)).astype(np.uint64)
    e.activation_ids_set(np.arange(BE.N_ACT, dtype=np.uint32), ids)
    kind = np.where(rng.random(n) < 0.25, g.RSP_REJECTION, g.RSP_RESPONSE).astype(np.uint8)
    blen = rng.integers(0, 64, size=n).astype(np.int64)
    boff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(blen, out=boff[1:])
    body_bytes = int(boff[n])
    t = lambda a: torch.from_numpy(a).to(dev)
    d_buf, d_off = t(buf), t(off.view(np.int64))
    d_silo = t(rng.integers(0, len(BE.SILOS), size=n).astype(np.int32))
    d_act = t(rng.integers(0, BE.N_ACT, size=n).astype(np.int32))
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_kind = t(kind)
    d_rej = torch.ones(n, dtype=torch.uint8, device=dev)               # Overloaded
    d_info = torch.zeros(n, dtype=torch.int32, device=dev)
    d_body = t(rng.integers(0, 256, size=max(body_bytes, 1), dtype=np.uint8))
    d_boff = t(boff)
    cap = max(enc_out, bytes_in + body_bytes + 64 * n) + 64
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_est = torch.empty(n, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    e.set_stream(s.cuda_stream)

    def encode():
        e.encode_frames_device(d_buf.data_ptr(), bytes_in, d_off.data_ptr(), n, d_silo.data_ptr(), d_act.data_ptr(),
                               d_st.data_ptr(), None, None, None, d_out.data_ptr(), cap, d_out_off.data_ptr(),
                               d_est.data_ptr())

    def respond():
        e.respond_frames_device(d_buf.data_ptr(), bytes_in, d_off.data_ptr(), n, d_kind.data_ptr(), None,
                                d_rej.data_ptr(), d_info.data_ptr(), d_body.data_ptr(), d_boff.data_ptr(), None,
                                d_out.data_ptr(), cap, d_out_off.data_ptr(), d_est.data_ptr())

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
        return {"plan": us[names[0]], "scan": scan, "write": us[names[1]]}

    with torch.cuda.stream(s):
        respond()
        e.synchronize()
        rsp_out = int(d_out_off[n].item())
        assert int((d_est != 0).sum().item()) == 0
        half = (bytes_in + body_bytes + rsp_out) // 2
        c_src = torch.empty(half, dtype=torch.uint8, device=dev)
        c_dst = torch.empty(half, dtype=torch.uint8, device=dev)
        for _ in range(args.warmup):
            encode()
            respond()
            c_dst.copy_(c_src)
        torch.cuda.synchronize()
        reps = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(args.steps):
                c_dst.copy_(c_src)
            b.record(s)
            torch.cuda.synchronize()
            copy_us = a.elapsed_time(b) / args.steps * 1e3
            enc = kernels(encode, ("k_enc_plan", "k_enc_write"))
            assert int(d_out_off[n].item()) == enc_out
            rsp = kernels(respond, ("k_rsp_plan", "k_rsp_write"))
            assert int(d_out_off[n].item()) == rsp_out
            reps.append({"copy_us": copy_us, "encode_us": enc, "respond_us": rsp})
    e.close()
    med = lambda f: float(np.median([f(r) for r in reps]))
    enc_w = [r["encode_us"]["write"] for r in reps]
    copy_us = med(lambda r: r["copy_us"])
    parts = ("plan", "scan", "write")
    enc = {k: med(lambda r: r["encode_us"][k]) for k in parts}
    rsp = {k: med(lambda r: r["respond_us"][k]) for k in parts}
    enc_ps, rsp_ps = enc["write"] * 1e6 / enc_out, rsp["write"] * 1e6 / rsp_out
    spread = (max(enc_w) - min(enc_w)) / float(np.median(enc_w))
    rec = {"metric": "response writer: kernel time against a device-to-device copy (a) and the frame encoder (b)",
           "frames": n, "bytes_in": bytes_in, "body_bytes": body_bytes, "bytes_out": rsp_out,
           "encode_bytes_out": enc_out, "plan_record_bytes": 128, "steps": args.steps, "reps": args.reps,
           "copy_us": round(copy_us, 1), "copy_GBps": round(2 * half / copy_us / 1e3, 1),
           "encode_us": {k: round(v, 1) for k, v in enc.items()},
           "respond_us": {k: round(v, 1) for k, v in rsp.items()},
           "respond_over_copy": {k: round(v / copy_us, 3) for k, v in rsp.items()},
           "respond_over_encode": {k: round(rsp[k] / enc[k], 3) for k in parts},
           "write_ps_per_output_byte": {"k_enc_write": round(enc_ps, 3), "k_rsp_write": round(rsp_ps, 3)},
           "encode_write_spread": round(spread, 4),
           "rsp_write_no_dearer_per_byte_within_spread": bool(rsp_ps <= enc_ps * (1 + spread)),
           "repetitions": [{k: (round(v, 1) if not isinstance(v, dict) else {q: round(x, 1) for q, x in v.items()})
                            for k, v in r.items()} for r in reps]}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
