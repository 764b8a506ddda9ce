#!/usr/bin/env python3
"""Request-writer bench: gd_request_frames_device on device arrays.

Workload: --frames addressed requests whose frames have the sizes of the encoder's bench output
(tools/bench_encode.py: headerLength 122 + the 52 bytes the encoder adds = the request writer's 174-byte header of
an addressed call without strings; bodies 0..63 B, the same lengths frame by frame).

Timed in the same run, --reps times over:
  (a) a device-to-device copy that moves the request stage's traffic (it copies (body bytes in + bytes out) / 2);
  (b) gd_encode_frames_device producing frames of the same sizes, per kernel -- the yardstick;
  (c) gd_request_frames_device, per kernel.
Reported: the median of the repetitions, each kernel of (c) as a ratio to (a) and to its counterpart in (b), the
writers' cost per output byte, and the run-to-run spread of (b)'s writer ((max - min) / median over the
repetitions), which is the margin of the comparison k_req_write <= k_enc_write per output byte.

usage: python tools/bench_request.py [--frames 4194304] [--steps 10] [--warmup 3] [--reps 5]
                                     [--out profiles/request.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "request.json"))
    args = ap.parse_args()
    n = args.frames
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0x5EED0023)
    buf, off, bytes_in = BE.build(n, rng)
    enc_out = bytes_in + 52 * n
    ends = np.append(off[1:], np.uint64(bytes_in))
    hl = int(buf[int(off[0]):int(off[0]) + 4].view("<i4")[0])         # the frames share one headerLength
    blen = (ends - off).astype(np.int64) - (8 + hl)
    assert blen.min() >= 0
    boff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(blen, out=boff[1:])
    body_bytes = int(boff[n])
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    e.encode_configure(BE.SILOS, ["BenchmarkGrains.Ping.PingGrain"])
    e.request_configure([])
    ids = rng.integers(1, 1 << 62, size=(BE.N_ACT, 3)).astype(np.uint64)
    e.activation_ids_set(np.arange(BE.N_ACT, dtype=np.uint32), ids)
    t = lambda a: torch.from_numpy(a).to(dev)
    d_buf, d_off = t(buf), t(off.view(np.int64))
    d_silo = t(rng.integers(0, len(BE.SILOS), size=n).astype(np.int32))
    d_act = t(rng.integers(0, BE.N_ACT, size=n).astype(np.int32))
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    keys = lambda: t(np.stack([rng.integers(0, 1 << 62, size=n), rng.integers(0, 1 << 62, size=n),
                               np.full(n, 0x0300000000000011)], axis=1).astype(np.int64))
    d_target, d_sender = keys(), keys()
    d_sact = t(rng.integers(0, BE.N_ACT, size=n).astype(np.int32))
    d_body = t(rng.integers(0, 256, size=max(body_bytes, 1), dtype=np.uint8))
    d_boff = t(boff)
    batch = {"target": d_target.data_ptr(), "sender_grain": d_sender.data_ptr(), "sender_act": d_sact.data_ptr(),
             "id_base": 1 << 40, "body": d_body.data_ptr(), "body_off": d_boff.data_ptr()}
    cap = enc_out + 64
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_est = torch.empty(n, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    e.set_stream(s.cuda_stream)

    def encode():
        e.encode_frames_device(d_buf.data_ptr(), bytes_in, d_off.data_ptr(), n, d_silo.data_ptr(), d_act.data_ptr(),
                               d_st.data_ptr(), None, None, None, d_out.data_ptr(), cap, d_out_off.data_ptr(),
                               d_est.data_ptr())

    def request():
        e.request_frames_device(batch, n, d_silo.data_ptr(), d_act.data_ptr(), d_st.data_ptr(), None, None, None,
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
        request()
        e.synchronize()
        req_out = int(d_out_off[n].item())
        assert int((d_est != 0).sum().item()) == 0
        half = (body_bytes + req_out) // 2
        c_src = torch.empty(half, dtype=torch.uint8, device=dev)
        c_dst = torch.empty(half, dtype=torch.uint8, device=dev)
        for _ in range(args.warmup):
            encode()
            request()
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
            req = kernels(request, ("k_req_plan", "k_req_write"))
            assert int(d_out_off[n].item()) == req_out
            reps.append({"copy_us": copy_us, "encode_us": enc, "request_us": req})
    e.close()
    med = lambda f: float(np.median([f(r) for r in reps]))
    enc_w = [r["encode_us"]["write"] for r in reps]
    req_w = [r["request_us"]["write"] for r in reps]
    copy_us = med(lambda r: r["copy_us"])
    parts = ("plan", "scan", "write")
    enc = {k: med(lambda r: r["encode_us"][k]) for k in parts}
    req = {k: med(lambda r: r["request_us"][k]) for k in parts}
    enc_ps, req_ps = enc["write"] * 1e6 / enc_out, req["write"] * 1e6 / req_out
    spread = (max(enc_w) - min(enc_w)) / float(np.median(enc_w))
    rec = {"metric": "request writer: kernel time against a device-to-device copy (a) and the frame encoder (b)",
           "frames": n, "body_bytes": body_bytes, "bytes_out": req_out, "encode_bytes_in": bytes_in,
           "encode_bytes_out": enc_out, "plan_record_bytes": 32, "steps": args.steps, "reps": args.reps,
           "copy_us": round(copy_us, 1), "copy_GBps": round(2 * half / copy_us / 1e3, 1),
           "encode_us": {k: round(v, 1) for k, v in enc.items()},
           "request_us": {k: round(v, 1) for k, v in req.items()},
           "request_over_copy": {k: round(v / copy_us, 3) for k, v in req.items()},
           "request_over_encode": {k: round(req[k] / enc[k], 3) for k in parts},
           "write_ps_per_output_byte": {"k_enc_write": round(enc_ps, 3), "k_req_write": round(req_ps, 3)},
           "encode_write_spread": round(spread, 4),
           "request_write_spread": round((max(req_w) - min(req_w)) / float(np.median(req_w)), 4),
           "req_write_no_dearer_per_byte": bool(req_ps <= enc_ps),
           "repetitions": [{k: (round(v, 1) if not isinstance(v, dict) else {q: round(x, 1) for q, x in v.items()})
                            for k, v in r.items()} for r in reps]}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
