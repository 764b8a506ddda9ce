#!/usr/bin/env python3
"""Frame-encoder bench: gd_encode_frames_device on a device receive buffer.

Workload: --frames request frames of the decoder's bench shape (tools/frames_synth.py: headerLength 122, no
TargetActivation / TargetSilo yet) with bodies of 0..63 B, every frame routed (GD_ROUTE_OK) to one of 8 silos
and an activation with an id, so every frame grows by 52 B.  Two runs: batch order, and the order of
gd_send_queues with 16 queues (each queue's frames contiguous; the reads become per-frame gathers).

Reported per run: the HIP-event time of every kernel of the stage (k_enc_plan, k_enc_lens + the scan +
k_enc_finish as "scan", k_enc_write), and beside them a device-to-device copy measured live in the same run
that moves the same traffic as the frames themselves (it copies (bytes in + bytes out) / 2, so it reads and
writes bytes in + bytes out in all); each kernel as a share of that copy.

usage: python tools/bench_encode.py [--frames 4194304] [--steps 10] [--warmup 3] [--out profiles/encode.json]
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
import frames_synth as FS  # noqa: E402

SILOS = [(f"10.0.0.{i + 1}", 11111, gen) for i, gen in
         enumerate([138558, 165678, 215136, 61804, 17808, 48728, 207265, 76820])]
N_ACT = 1 << 16


def build(n, rng):
    """Frames with bodies of 0..63 B: (buffer u8, offsets u64)."""
    keys = np.zeros((n, 3), dtype=np.uint64)
    keys[:, 1] = rng.integers(0, 1 << 20, size=n)
    keys[:, 2] = np.uint64((3 << 56) + 77)
    hdr, _, hlen = FS.build_frames(keys, rng, body_len=0)
    hdr = hdr.reshape(n, hlen)
    bl = rng.integers(0, 64, size=n).astype(np.int64)
    hdr[:, 4:8] = bl.astype("<i4").view(np.uint8).reshape(n, 4)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(hlen + bl, out=off[1:])
    buf = rng.integers(0, 256, size=int(off[n]), dtype=np.uint8)
    col = np.arange(hlen, dtype=np.int64)
    for a in range(0, n, 1 << 18):
        b = min(n, a + (1 << 18))
        buf[(off[a:b, None] + col).reshape(-1)] = hdr[a:b].reshape(-1)
    return buf, off[:n].astype(np.uint64), int(off[n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode.json"))
    args = ap.parse_args()
    n = args.frames
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0x5EED0014)
    buf, off, bytes_in = build(n, rng)
    bytes_out = bytes_in + 52 * n
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    e.encode_configure(SILOS, ["BenchmarkGrains.Ping.PingGrain"])
    ids = rng.integers(1, 1 << 62, size=(N_ACT, 3)).astype(np.uint64)
    e.activation_ids_set(np.arange(N_ACT, dtype=np.uint32), ids)
    e.send_configure([g.silo_consistent_hash(*s) for s in SILOS], 16)
    d_buf = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_silo = torch.from_numpy(rng.integers(0, len(SILOS), size=n).astype(np.int32)).to(dev)
    d_act = torch.from_numpy(rng.integers(0, N_ACT, size=n).astype(np.int32)).to(dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_sst = torch.empty(n, dtype=torch.uint8, device=dev)
    d_perm = torch.empty(n, dtype=torch.int32, device=dev)
    d_qoff = torch.empty(16 + 5, dtype=torch.int32, device=dev)
    d_out = torch.empty(bytes_out + 64, dtype=torch.uint8, device=dev)
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_est = torch.empty(n, dtype=torch.uint8, device=dev)
    half = (bytes_in + bytes_out) // 2
    c_src = torch.empty(half, dtype=torch.uint8, device=dev)
    c_dst = torch.empty(half, dtype=torch.uint8, device=dev)
    e.send_queues_device(d_silo.data_ptr(), d_st.data_ptr(), None, None, n, d_sst.data_ptr(), None, d_perm.data_ptr(),
                         d_qoff.data_ptr())
    e.synchronize()
    s = torch.cuda.Stream(device=dev)
    e.set_stream(s.cuda_stream)

    def encode(order):
        e.encode_frames_device(d_buf.data_ptr(), bytes_in, d_off.data_ptr(), n, d_silo.data_ptr(), d_act.data_ptr(),
                               d_st.data_ptr(), None, None, order, d_out.data_ptr(), bytes_out + 64,
                               d_out_off.data_ptr(), d_est.data_ptr())

    rec = {"metric": "frame encoder: kernel time as a share of a device-to-device copy of the same traffic",
           "frames": n, "bytes_in": bytes_in, "bytes_out": bytes_out, "plan_record_bytes": 32,
           "steps": args.steps, "runs": {}}
    with torch.cuda.stream(s):
        for name, order in (("batch_order", None), ("queue_order_16", d_perm.data_ptr())):
            for _ in range(args.warmup):
                encode(order)
                c_dst.copy_(c_src)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(args.steps):
                c_dst.copy_(c_src)
            b.record(s)
            torch.cuda.synchronize()
            copy_us = a.elapsed_time(b) / args.steps * 1e3
            a.record(s)
            for _ in range(args.steps):
                encode(order)
            b.record(s)
            torch.cuda.synchronize()
            stage_us = a.elapsed_time(b) / args.steps * 1e3
            e.set_kernel_timing(True)
            e.kernel_times_reset()
            for _ in range(args.steps):
                encode(order)
            e.synchronize()
            kt = e.kernel_times()
            e.set_kernel_timing(False)
            assert int(d_out_off[n].item()) == bytes_out and int((d_est != 0).sum().item()) == 0
            us = {k: ms / args.steps * 1e3 for k, (cnt, ms) in kt.items()}
            scan_us = sum(v for k, v in us.items() if k.startswith("k_scan") or k in ("k_enc_lens", "k_enc_finish"))
            parts = {"k_enc_plan": us["k_enc_plan"], "scan": scan_us, "k_enc_write": us["k_enc_write"]}
            rec["runs"][name] = {
                "copy_us": round(copy_us, 1), "copy_GBps": round((bytes_in + bytes_out) / copy_us / 1e3, 1),
                "stage_us": round(stage_us, 1), "frames_per_s": round(n / stage_us * 1e6, 1),
                "kernel_us": {k: round(v, 1) for k, v in parts.items()},
                "share_of_copy": {k: round(v / copy_us, 3) for k, v in parts.items()},
                "write_GBps": round((bytes_in + bytes_out) / parts["k_enc_write"] / 1e3, 1)}
    e.close()
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
