#!/usr/bin/env python3
"""The callback table on one MI355X.

--msgs requests are added to a table of 2 x msgs slots (load 0.5 when all are in), then answered.  CorrelationIds
are a counter's run in a random order.  Timed, alternating within each round, inputs resident in HBM, device events
on the handle's stream; the table is cleared (untimed) before each add:
  add              gd_callbacks_add_device into the empty table
  respond          gd_callbacks_respond_device, all Success, with fire_idx (max_resend_count 0: one round)
  add_r / respond_r    the same with max_resend_count 1 and 1 % transient rejections (RESEND, the entry stays)
  add_churn        the add after a respond without the clear: the table is all tombstones, so the add reads the
                   counters back and rebuilds the table first (the steady state of a request/response cycle)
  expire           one gd_callbacks_expire_device scan over the full table with 1 % of the deadlines due
  actdir           gd_receive_device without buckets over an ActivationDirectory of msgs entries: the nearest probe
                   the library already has (24-B keys, 32-B slots)
  copy_add / copy_respond / copy_expire   device-to-device copies moving each call's own bytes (ADD_BYTES,
                   RESP_BYTES a message, SCAN_BYTES a slot), measured live
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

# add: id 8 + handle 4 + deadline 8 in, added 1 out, the 16-B slot and its 8-B deadline written
ADD_BYTES = 8 + 4 + 8 + 1 + 16 + 8
# respond: id 8 + result 1 in, outcome 1 + flags 1 + handle 4 + fire_idx 4 out, one 64-B group read, the meta written
RESP_BYTES = 8 + 1 + 1 + 1 + 4 + 4 + 64 + 4
# expire, per slot: the 16-B slot and 8-B deadline read, the flag written, read and rewritten by the scan, read again
SCAN_BYTES = 16 + 8 + 4 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=1 << 24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    N = args.msgs
    cap = 2 * N
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    gen = torch.Generator(device=dev).manual_seed(0xCB01)
    ids = (torch.randperm(N, device=dev, generator=gen) + 1).to(torch.int64)
    handles = torch.arange(N, dtype=torch.int32, device=dev)
    u = torch.rand(N, device=dev, generator=gen)
    deadlines = torch.where(u < 0.01, 100, 1 << 40).to(torch.int64)
    result_ok = torch.zeros(N, dtype=torch.uint8, device=dev)
    result_r = torch.where(torch.rand(N, device=dev, generator=gen) < 0.01, 2, 0).to(torch.uint8)
    rej = torch.zeros(N, dtype=torch.uint8, device=dev)

    # the ActivationDirectory probe at the same n: every message targets its own activation
    rng = np.random.default_rng(0xCB02)
    act = np.zeros((N, 3), np.uint64)
    act[:, 0] = rng.integers(0, 1 << 63, size=N, dtype=np.int64).astype(np.uint64)
    act[:, 1] = rng.integers(0, 1 << 63, size=N, dtype=np.int64).astype(np.uint64)
    assert e.actdir_add(act, np.arange(N, dtype=np.uint32), np.full(N, g.ACTDIR_VALID, np.uint8)).all()
    ta = torch.from_numpy(act.view(np.int64)).to(dev)[torch.randperm(N, device=dev, generator=gen)].contiguous()
    tg = torch.zeros((N, 3), dtype=torch.int64, device=dev)
    tg[:, 1] = torch.arange(N, device=dev)
    tg[:, 2] = (3 << 56) + (g.calculate_id_hash("BenchmarkGrains.Ping.PingGrain") & 0x00FFFFFFFFFFFFFF)   # a Grain
    del act

    i32 = lambda k: torch.empty(max(k, 1), dtype=torch.int32, device=dev)
    u8 = lambda k: torch.empty(max(k, 1), dtype=torch.uint8, device=dev)
    added, outcome, oflags, ohandle, fire, nfire = u8(N), u8(N), u8(N), i32(N), i32(N), i32(1)
    x_id, x_h, x_k, x_n = torch.empty(N, dtype=torch.int64, device=dev), i32(N), u8(N), i32(1)
    ctx, st = i32(N), u8(N)
    copies = {k: (u8(b // 2), u8(b // 2)) for k, b in (("copy_add", N * ADD_BYTES), ("copy_respond", N * RESP_BYTES),
                                                       ("copy_expire", cap * SCAN_BYTES))}
    stream = torch.cuda.Stream(dev)
    e.set_stream(stream.cuda_stream)
    P = lambda t: t.data_ptr()

    def add():
        e.callbacks_add_device(P(ids), P(handles), P(deadlines), N, P(added))

    def respond(res):
        e.callbacks_respond_device(P(ids), P(res), P(rej), None, None, N, P(outcome), P(oflags), P(ohandle), P(fire),
                                   P(nfire))

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        f()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    names = ["add", "respond", "add_churn", "add_r", "respond_r", "expire", "actdir", "copy_add", "copy_respond",
             "copy_expire"]
    times = {k: [] for k in names}
    checks = {}
    with torch.cuda.stream(stream):
        for rnd in range(args.rounds + 1):               # round 0 warms every shape and is dropped
            t = {}
            e.callbacks_configure(cap, 0)
            e.callbacks_clear()
            t["add"] = timed(add)
            t["respond"] = timed(lambda: respond(result_ok))
            checks["fired"] = int(nfire.item())
            t["add_churn"] = timed(add)
            e.callbacks_configure(cap, 1)
            e.callbacks_clear()
            t["add_r"] = timed(add)
            t["respond_r"] = timed(lambda: respond(result_r))
            checks["fired_r"], checks["resent_r"] = int(nfire.item()), int((outcome == g.CB_RESEND).sum().item())
            e.callbacks_clear()
            add()
            t["expire"] = timed(lambda: e.callbacks_expire_device(100, N, P(x_id), P(x_h), P(x_k), P(x_n)))
            checks["expired"] = int(x_n.item())
            t["actdir"] = timed(lambda: e.receive_device(P(tg), P(ta), None, N, N, P(ctx), P(st), None, None))
            for k, (src, dst) in copies.items():
                t[k] = timed(lambda: dst.copy_(src))
            if rnd:
                for k in names:
                    times[k].append(t[k])
        checks["capacity"] = e.callbacks_count()[1]
        # per-kernel times of one add / respond pair with a resend round, in a pass of its own
        e.callbacks_clear()
        e.set_kernel_timing(True)
        e.kernel_times_reset()
        add()
        respond(result_r)
        torch.cuda.synchronize()
        kernels = {name: round(ms, 4) for name, (launches, ms) in e.kernel_times().items()}
        e.set_kernel_timing(False)
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {"metric": "callback table: add, respond, expire", "n_gpus": 1, "data": "synthetic",
           "config": {"msgs": N, "slots": cap, "rounds": args.rounds, "add_bytes_per_msg": ADD_BYTES,
                      "respond_bytes_per_msg": RESP_BYTES, "scan_bytes_per_slot": SCAN_BYTES},
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
           "frac_of_byte_bound": {"add": round(med["copy_add"] / med["add"], 4),
                                  "respond": round(med["copy_respond"] / med["respond"], 4),
                                  "expire": round(med["copy_expire"] / med["expire"], 4)},
           "respond_over_actdir_probe": round(med["respond"] / med["actdir"], 4),
           "checks": checks, "add_respond_r_kernel_ms": kernels}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    e.close()


if __name__ == "__main__":
    main()
