#!/usr/bin/env python3
"""The frame-fed chain on one MI355X: receive buffer -> decode -> ReceiveMessage -> ReceiveRequest.

A silo hosting --acts activations receives --frames addressed request / response frames, TargetActivation uniform
over the activations.  The frames have the tools/frames_synth.py layout with the turn headers and the address
present (little-endian, BinaryTokenStreamWriter):

  [int32 hl][int32 bl] | mask | cat u8 | dir u8 | ttl i64 | fwd i32 | corr i64 | AlwaysInterleave token |
  ReadOnly token | SendingActivation 24+4 | SendingGrain 24+4 | SendingSilo 24 | TargetActivation 24+4 |
  TargetGrain 24+4 | TargetSilo 24 | body

hl = 188; with the default 16-byte body a frame is 212 bytes.  30% read-only, 2% always-interleave, 1% expired,
20% responses; context state as tools/bench_turns.py.  Buffer, offsets and every side array are resident in HBM.
Timed, alternating within each round, device events on the handle's stream:
  fused          gd_receive_turns_frames_device (lists included)
  two_calls      gd_receive_frames_device, then gd_turns_device fed with the side arrays (ttl, forward count, flags)
                 already in HBM: the parent's path if decoding them in C# were free
  decode         gd_decode_frames_device: flags, TargetGrain, TargetActivation, Direction (what two_calls decodes)
  decode_turn    gd_decode_frames_turn_device: the same plus ttl, forward count, flags (what fused decodes)
Algorithmic bytes of the decode kernel per frame: 8 (offset) + 8 + hl (prefix and header, read once) + 4 + 24 + 24
+ 1 written = 257 B; the turn instantiation writes 8 + 1 + 1 more = 267 B.
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
TRUE_TOKEN, FALSE_TOKEN = 3, 4
MASK = (1 << 0) | (1 << 2) | (1 << 3) | (1 << 5) | (1 << 6) | (1 << 7) | (1 << 13) | (1 << 15) | (1 << 16) | (1 << 17) | \
       (1 << 19) | (1 << 20) | (1 << 21)
HEADER_LEN = 4 + 1 + 1 + 8 + 4 + 8 + 1 + 1 + 28 + 28 + 24 + 28 + 28 + 24
PEAK_HBM = 8000.0  # GB/s


def build_frames(dev, gen, ta, tg, direction, ttl, fwd, mf, body_len):
    """The frames on the device: (buffer u8[n * frame_len], offsets i64[n], frame_len)."""
    n = ta.shape[0]
    fl = 8 + HEADER_LEN + body_len
    rec = torch.zeros((n, fl), dtype=torch.uint8, device=dev)
    col = 0

    def put(t):
        nonlocal col
        b = t.contiguous().view(torch.uint8).reshape(n, -1)
        rec[:, col:col + b.shape[1]] = b
        col += b.shape[1]

    i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)
    put(i32(HEADER_LEN))
    put(i32(body_len))
    put(i32(MASK))
    put(torch.full((n,), 2, dtype=torch.uint8, device=dev))                 # Category.Application
    put(direction)
    put(ttl)
    put(fwd.to(torch.int32))
    put(torch.arange(1, n + 1, dtype=torch.int64, device=dev))              # CorrelationId
    put(torch.where((mf & g.MSG_ALWAYS_INTERLEAVE) != 0, TRUE_TOKEN, FALSE_TOKEN).to(torch.uint8))
    put(torch.where((mf & g.MSG_READ_ONLY) != 0, TRUE_TOKEN, FALSE_TOKEN).to(torch.uint8))
    sa = torch.randint(0, 1 << 62, (n, 3), device=dev, generator=gen)
    sa[:, 2] = 0
    put(sa)
    put(i32(-1))
    put(tg[torch.randint(0, n, (n,), device=dev, generator=gen)])           # SendingGrain
    put(i32(-1))
    silo = torch.zeros((n, 24), dtype=torch.uint8, device=dev)
    silo[:, 12:16] = torch.tensor([10, 0, 0, 1], dtype=torch.uint8, device=dev)
    silo[:, 16:20] = torch.tensor(list(np.int32(11111).tobytes()), dtype=torch.uint8, device=dev)
    silo[:, 20:24] = torch.tensor(list(np.int32(138558).tobytes()), dtype=torch.uint8, device=dev)
    put(silo)
    put(ta)
    put(i32(-1))
    put(tg)
    put(i32(-1))
    put(silo)
    assert col == 8 + HEADER_LEN
    off = torch.arange(n, dtype=torch.int64, device=dev) * fl
    return rec.reshape(-1), off, fl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--acts", type=int, default=1 << 20)
    ap.add_argument("--body", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    A, N = args.acts, args.frames
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
    ttl = torch.where(torch.rand(N, device=dev, generator=gen) < 0.01, 0, 10_000_000 * 30)   # expired, or 30 s
    fwd = torch.zeros(N, dtype=torch.uint8, device=dev)
    which = torch.randint(0, A, (N,), device=dev, generator=gen)
    tg = torch.zeros((N, 3), dtype=torch.int64, device=dev)
    tg[:, 1] = which
    tg[:, 2] = tcd
    ta = d_ids[which].contiguous()
    d_buf, d_off, frame_len = build_frames(dev, gen, ta, tg, direction, ttl, fwd, mf, args.body)
    del tg, ta
    torch.cuda.synchronize()

    i32 = lambda k: torch.empty(max(k, 1), dtype=torch.int32, device=dev)
    u8 = lambda k: torch.empty(max(k, 1), dtype=torch.uint8, device=dev)
    key = lambda: torch.empty((N, 3), dtype=torch.int64, device=dev)
    out = [dict(ctx=i32(N), st=u8(N), perm=i32(N), off=i32(A + 3), turn=u8(N), nro=i32(A), run=i32(A), start=i32(N),
                ns=i32(1), wp=i32(N), wo=i32(A + 2)) for _ in range(2)]
    P = lambda t: t.data_ptr()
    d_f = {"flags": i32(N), "target_grain": key(), "target_activation": key(), "direction": u8(N)}
    fields = {k: P(v) for k, v in d_f.items()}
    d_t = {"ttl": torch.empty(N, dtype=torch.int64, device=dev), "forward_count": u8(N), "msg_flags": u8(N)}
    tfields = {k: P(v) for k, v in d_t.items()}
    lib, V = g.lib, lambda t: g.C.c_void_p(t.data_ptr())
    ff = g.gd_frame_fields(**{k: g.C.c_void_p(v) for k, v in fields.items()})
    stream = torch.cuda.Stream(dev)
    e.set_stream(stream.cuda_stream)
    blen = d_buf.numel()

    def fused():
        o = out[0]
        e.receive_turns_frames_device(P(d_buf), blen, P(d_off), N, A, None, None, P(o["ctx"]), P(o["st"]), P(o["perm"]),
                                      P(o["off"]), 0, None, state, P(o["turn"]), P(o["nro"]), P(o["run"]), P(o["start"]),
                                      P(o["ns"]), P(o["wp"]), P(o["wo"]))

    def two_calls():
        o = out[1]
        e._c(lib.gd_receive_frames_device(e.h, V(d_buf), blen, V(d_off), N, A, None, g.C.byref(ff), V(o["ctx"]),
                                          V(o["st"]), V(o["perm"]), V(o["off"])))
        e.turns_device(P(o["ctx"]), P(o["st"]), P(d_f["direction"]), P(ttl), P(fwd), P(mf), None, None, N, A, state,
                       P(o["turn"]), P(o["nro"]), P(o["run"]), P(o["start"]), P(o["ns"]), P(o["wp"]), P(o["wo"]))

    variants = {
        "fused": fused,
        "two_calls": two_calls,
        "decode": lambda: e.decode_frames_device(P(d_buf), blen, P(d_off), N, fields),
        "decode_turn": lambda: e.decode_frames_turn_device(P(d_buf), blen, P(d_off), N, fields, tfields),
    }
    times = {k: [] for k in variants}
    with torch.cuda.stream(stream):
        for f in variants.values():                    # warm every shape (and the bucketing's variant choice)
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
    # the two paths agree, and the decoder gave back the side arrays the frames were built from
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]) or k in ("start", "perm", "wp"), k
    ns = int(out[0]["ns"][0])
    assert torch.equal(out[0]["start"][:ns], out[1]["start"][:ns]) and torch.equal(out[0]["perm"], out[1]["perm"])
    assert torch.equal(out[0]["wp"], out[1]["wp"])
    assert torch.equal(d_t["ttl"], ttl) and torch.equal(d_t["msg_flags"], mf) and torch.equal(d_t["forward_count"], fwd)
    counts = torch.bincount(out[0]["turn"].to(torch.int64), minlength=10).tolist()
    e.set_kernel_timing(True)
    e.kernel_times_reset()
    for _ in range(3):
        fused()
    torch.cuda.synchronize()
    kernels = {name: round(ms / max(launches, 1), 4) for name, (launches, ms) in e.kernel_times().items()}
    e.set_kernel_timing(False)
    med = {k: float(np.median(v)) for k, v in times.items()}
    alg = {"decode": 8 + 8 + HEADER_LEN + 4 + 24 + 24 + 1}
    alg["decode_turn"] = alg["decode"] + 8 + 1 + 1
    gbps = {k: round(alg[k] * N / (med[k] * 1e-3) / 1e9, 1) for k in alg}
    result = {"metric": "frame-fed turn admission: receive buffer to InvokeWorkItem list", "n_gpus": 1,
              "data": "synthetic",
              "config": {"frames": N, "acts": A, "frame_bytes": frame_len, "header_len": HEADER_LEN, "rounds": args.rounds,
                         "reps": args.reps},
              "ms_median": {k: round(v, 4) for k, v in med.items()},
              "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
              "fused_over_two_calls": round(med["fused"] / med["two_calls"], 4),
              "decode_turn_over_decode": round(med["decode_turn"] / med["decode"], 4),
              "frames_per_s_fused": round(N / (med["fused"] * 1e-3), 1),
              "decode_alg_bytes_per_frame": alg, "decode_achieved_GBps": gbps,
              "decode_frac_of_hbm_peak": {k: round(v / PEAK_HBM, 3) for k, v in gbps.items()},
              "turn_counts": counts, "fused_kernel_ms": kernels}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    e.close()


if __name__ == "__main__":
    main()
