#!/usr/bin/env python3
"""Forward-writer bench: gd_forward_frames_device on a device receive buffer.

Workload: --frames request frames of the encoder's bench shape (tools/bench_encode.py: headerLength 122, all
Request, bodies 0..63 B); 1 % of them carry one old CacheInvalidationHeader entry (84 B more); every frame is
forwarded with an old address (one entry appended), half of them with a forwarding address, the rest unaddressed.

Timed in the same run, --reps times over:
  (a) a device-to-device copy of the forward writer's output bytes;
  (b) gd_encode_frames_device on the same frames, per kernel;
  (c) gd_respond_frames_device on the same frames (empty bodies, Success), per kernel;
  (d) gd_forward_frames_device, per kernel (plan, scan, write).
(b) and (c) leave the 1 % with an invalidation header to C# (FALLBACK); each writer's cost is per byte it wrote.
Reported: the median of the repetitions, the three writers in ps per output byte, and the run-to-run spread of
each writer ((max - min) / median over the repetitions).

usage: python tools/bench_forward.py [--frames 4194304] [--steps 10] [--warmup 3] [--reps 5]
                                     [--out profiles/forward.json]
"""
import argparse
import json
import os
import struct
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from orleans_amd import graindispatch as g  # noqa: E402
import bench_encode as BE  # noqa: E402
import frames_synth as FS  # noqa: E402

ENTRY = 4 + 80          # the count and one long-keyed entry


def build(n, rng, p_old=0.01):
    """bench_encode.build's frames, a fraction p_old of them with one old invalidation entry."""
    keys = np.zeros((n, 3), dtype=np.uint64)
    keys[:, 1] = rng.integers(0, 1 << 20, size=n)
    keys[:, 2] = np.uint64((3 << 56) + 77)
    hdr, _, hlen = FS.build_frames(keys, rng, body_len=0)
    hdr = hdr.reshape(n, hlen)
    bl = rng.integers(0, 64, size=n).astype(np.int64)
    hdr[:, 4:8] = bl.astype("<i4").view(np.uint8).reshape(n, 4)
    old = rng.random(n) < p_old
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(hlen + bl + ENTRY * old, out=off[1:])
    buf = rng.integers(0, 256, size=int(off[n]), dtype=np.uint8)
    entry = np.frombuffer(struct.pack("<i", 1) + bytes(range(24)) + struct.pack("<QQQi", 5, 6, (3 << 56) + 77, -1) +
                          struct.pack("<QQQi", 8, 9, 0, -1), np.uint8)
    for sel, cols, src in ((~old, np.arange(hlen), hdr), (old, np.arange(12), hdr[:, :12]),
                           (old, 12 + ENTRY + np.arange(hlen - 12), hdr[:, 12:])):
        idx = np.flatnonzero(sel)
        for a in range(0, len(idx), 1 << 18):
            i = idx[a:a + (1 << 18)]
            buf[(off[i, None] + cols).reshape(-1)] = src[i].reshape(-1)
    io = np.flatnonzero(old)
    buf[(off[io, None] + 12 + np.arange(ENTRY)).reshape(-1)] = np.tile(entry, len(io))
    hl = hdr[io, 0:4].copy().view("<i4").reshape(-1) + ENTRY
    buf[(off[io, None] + np.arange(4)).reshape(-1)] = hl.astype("<i4").view(np.uint8)
    buf[off[io] + 8] |= 2                                              # Headers.CACHE_INVALIDATION_HEADER
    return buf, off[:n].astype(np.uint64), int(off[n]), int(old.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward.json"))
    args = ap.parse_args()
    n = args.frames
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0x5EED0024)
    buf, off, bytes_in, n_old = build(n, rng)
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    e.encode_configure(BE.SILOS, ["BenchmarkGrains.Ping.PingGrain"])
    e.respond_configure([])
    ids = rng.integers(1, 1 << 62, size=(BE.N_ACT, 3)).astype(np.uint64)
    e.activation_ids_set(np.arange(BE.N_ACT, dtype=np.uint32), ids)
    t = lambda a: torch.from_numpy(a).to(dev)
    d_buf, d_off = t(buf), t(off.view(np.int64))
    d_silo = t(rng.integers(0, len(BE.SILOS), size=n).astype(np.int32))
    d_act = t(rng.integers(0, BE.N_ACT, size=n).astype(np.int32))
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_kind = torch.ones(n, dtype=torch.uint8, device=dev)              # GD_RSP_RESPONSE and GD_FWD_FORWARD are both 1
    d_old = t(rng.integers(0, BE.N_ACT, size=n).astype(np.int32))
    fs = rng.integers(0, len(BE.SILOS), size=n).astype(np.int32)
    fs[rng.random(n) < 0.5] = -1                                       # GD_NO_SILO: no forwarding address
    d_fs = t(fs)
    cap = bytes_in + 200 * n + 64
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_est = torch.empty(n, dtype=torch.uint8, device=dev)
    d_tg = torch.empty((n, 3), dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(device=dev)
    e.set_stream(s.cuda_stream)
    db = {"buf": d_buf.data_ptr(), "buf_len": bytes_in, "frame_off": d_off.data_ptr(), "kind": d_kind.data_ptr(),
          "old_act": d_old.data_ptr(), "fwd_silo": d_fs.data_ptr(), "fwd_act": d_act.data_ptr(),
          "max_forward_count": 2, "local_silo": 0}

    def encode():
        e.encode_frames_device(d_buf.data_ptr(), bytes_in, d_off.data_ptr(), n, d_silo.data_ptr(), d_act.data_ptr(),
                               d_st.data_ptr(), None, None, None, d_out.data_ptr(), cap, d_out_off.data_ptr(),
                               d_est.data_ptr())

    def respond():
        e.respond_frames_device(d_buf.data_ptr(), bytes_in, d_off.data_ptr(), n, d_kind.data_ptr(), None, None, None,
                                None, None, None, d_out.data_ptr(), cap, d_out_off.data_ptr(), d_est.data_ptr())

    def forward():
        e.forward_frames_device(db, n, None, None, None, None, None, None, d_out.data_ptr(), cap,
                                d_out_off.data_ptr(), d_est.data_ptr(), d_tg.data_ptr())

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
        return {"plan": us[names[0]], "scan": scan, "write": us[names[1]], "bytes_out": int(d_out_off[n].item())}

    with torch.cuda.stream(s):
        forward()
        e.synchronize()
        fwd_out = int(d_out_off[n].item())
        assert int((d_est > 1).sum().item()) == 0                      # every frame OK_ADDRESSED or OK_UNADDRESSED
        c_src = torch.empty(fwd_out, dtype=torch.uint8, device=dev)
        c_dst = torch.empty(fwd_out, dtype=torch.uint8, device=dev)
        for _ in range(args.warmup):
            encode()
            respond()
            forward()
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
            reps.append({"copy_us": copy_us, "encode_us": kernels(encode, ("k_enc_plan", "k_enc_write")),
                         "respond_us": kernels(respond, ("k_rsp_plan", "k_rsp_write")),
                         "forward_us": kernels(forward, ("k_fwd_plan", "k_fwd_write"))})
            assert reps[-1]["forward_us"]["bytes_out"] == fwd_out
    e.close()
    med = lambda f: float(np.median([f(r) for r in reps]))
    parts = ("plan", "scan", "write")
    stage = {k: {p: med(lambda r: r[k][p]) for p in parts} for k in ("encode_us", "respond_us", "forward_us")}
    outs = {k: reps[0][k]["bytes_out"] for k in stage}
    ps = {k: stage[k]["write"] * 1e6 / outs[k] for k in stage}
    spread = {k: (max(r[k]["write"] for r in reps) - min(r[k]["write"] for r in reps)) / stage[k]["write"] for k in stage}
    copy_us = med(lambda r: r["copy_us"])
    rnd = lambda d: {q: (round(x, 1) if isinstance(x, float) else x) for q, x in d.items()}
    rec = {"metric": "forward writer: kernel time against a device-to-device copy of its output and the two other "
                     "source-frame writers on the same frames",
           "frames": n, "frames_with_an_old_entry": n_old, "bytes_in": bytes_in, "bytes_out": fwd_out,
           "encode_bytes_out": outs["encode_us"], "respond_bytes_out": outs["respond_us"], "plan_record_bytes": 128,
           "steps": args.steps, "reps": args.reps, "copy_us": round(copy_us, 1),
           "copy_GBps": round(2 * fwd_out / copy_us / 1e3, 1),
           "encode_us": rnd(stage["encode_us"]), "respond_us": rnd(stage["respond_us"]),
           "forward_us": rnd(stage["forward_us"]),
           "forward_over_copy": {k: round(v / copy_us, 3) for k, v in stage["forward_us"].items()},
           "write_ps_per_output_byte": {"k_enc_write": round(ps["encode_us"], 3), "k_rsp_write": round(ps["respond_us"], 3),
                                        "k_fwd_write": round(ps["forward_us"], 3)},
           "write_spread": {"k_enc_write": round(spread["encode_us"], 4), "k_rsp_write": round(spread["respond_us"], 4),
                            "k_fwd_write": round(spread["forward_us"], 4)},
           "fwd_over_rsp_per_byte": round(ps["forward_us"] / ps["respond_us"], 3),
           "repetitions": [{k: (round(v, 1) if not isinstance(v, dict) else rnd(v)) for k, v in r.items()} for r in reps]}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
