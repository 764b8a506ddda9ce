#!/usr/bin/env python3
"""The stateless-worker stage on one MI355X: gd_workers_select_device.

--msgs messages (default 2^24) over --sets worker sets (default 1,024) of MaxLocal 16, each set full:
  all_idle   every worker idle (the first 16 messages of a set are IDLE, the rest RANDOM)
  all_busy   every worker running (all RANDOM)
  hot_half   all busy, half the batch on one set
and --new all-new grains (default 2^20, MaxLocal 1: every message NEW; the table is cleared before each run).
Each beside two yardsticks on the same keys: a device-to-device copy moving the bytes a message must read and write
(24-B key + 4-B draw in, 4-B ctx + 1-B pick out), and gd_route_bucket_device with the grains registered in the
directory, one activation each.  Device events on the handle's stream; one warm-up round, then --reps interleaved
rounds (every shape and yardstick once a round); median and min..max.  Prints one JSON line; --out also writes it.
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

MAX_LOCAL, SLOT_CAPACITY = 16, 16
IO_BYTES = 24 + 4 + 4 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=1 << 24)
    ap.add_argument("--sets", type=int, default=1024)
    ap.add_argument("--new", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    n, S = args.msgs, args.sets
    stream = torch.cuda.Stream()
    gen = torch.Generator(device=dev).manual_seed(0x57A7)
    tcd = (3 << 56) | (77 << 32)

    def keys(ids):
        k = torch.zeros((ids.numel(), 3), dtype=torch.int64, device=dev)
        k[:, 1] = ids
        k[:, 2] = tcd
        return k.contiguous()

    silos = [("10.0.0.%d" % (i + 1), 11111, 1) for i in range(8)]
    e = g.GrainDispatch(device=0, table_capacity=1 << 22, my_silo=0)
    e.ring_set_silos("D", silos)
    e.set_stream(stream.cuda_stream)
    e.workers_configure(max(S, args.new), SLOT_CAPACITY, MAX_LOCAL)
    n_ctx = S * MAX_LOCAL
    host_keys = np.zeros((S, 3), np.uint64)
    host_keys[:, 1] = np.arange(1, S + 1)
    host_keys[:, 2] = tcd
    e.register(host_keys, np.arange(S), e.ring_owner(host_keys))
    new_host = np.zeros((args.new, 3), np.uint64)
    new_host[:, 1] = (1 << 32) + np.arange(args.new)
    new_host[:, 2] = tcd

    def fill():
        st = e.workers_add(np.repeat(host_keys, MAX_LOCAL, axis=0), np.arange(n_ctx, dtype=np.uint32),
                           np.full(n_ctx, MAX_LOCAL, np.int32))
        assert (st == g.WK_ADDED).all()

    res = {"metric": "stateless-worker select", "n_gpus": 1, "data": "synthetic",
           "config": {"msgs": n, "sets": S, "max_local": MAX_LOCAL, "new": args.new, "reps": args.reps,
                      "io_bytes_per_message": IO_BYTES}, "shapes": {}}
    with torch.cuda.stream(stream):
        uniform = torch.randint(1, S + 1, (n,), device=dev, generator=gen)
        hot = torch.where(torch.rand(n, device=dev, generator=gen) < 0.5, torch.ones_like(uniform), uniform)
        batches = {"all_idle": (keys(uniform), n, 0), "all_busy": (keys(uniform), n, 1), "hot_half": (keys(hot), n, 1),
                   "all_new": (torch.from_numpy(new_host.view(np.int64)).to(dev).contiguous(), args.new, 1)}
        draw = torch.randint(0, 0x7FFFFFFF, (n,), device=dev, generator=gen).to(torch.int32)
        fl = torch.zeros(n_ctx, dtype=torch.uint8, device=dev)
        running = [torch.zeros(n_ctx, dtype=torch.int32, device=dev), torch.ones(n_ctx, dtype=torch.int32, device=dev)]
        ctx, perm, silo, act = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
        pick, status = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
        off = torch.empty(n_ctx + 2, dtype=torch.int32, device=dev)
        one = torch.ones(args.new, dtype=torch.int32, device=dev)
        src = {m: torch.empty(max(m * IO_BYTES // 2, 1), dtype=torch.uint8, device=dev) for m in {n, args.new}}
        dst = {m: torch.empty_like(v) for m, v in src.items()}

    def select(name):
        k, m, busy = batches[name]
        ml = one.data_ptr() if name == "all_new" else None
        e.workers_select_device(k.data_ptr(), m, ml, draw.data_ptr(), n_ctx, n_ctx, fl.data_ptr(),
                                running[busy].data_ptr(), None, ctx.data_ptr(), pick.data_ptr())

    def timed(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    ms = {}
    for rep in range(args.reps + 1):                       # round 0 warms up
        for name, (k, m, _) in batches.items():
            e.synchronize()
            e.workers_clear()                              # outside the timed window
            if name != "all_new":
                fill()
            with torch.cuda.stream(stream):
                t = {"select": timed(lambda: select(name)),
                     "copy": timed(lambda: dst[m].copy_(src[m])),
                     "route_bucket": timed(lambda: e.route_bucket_device(k.data_ptr(), m, n_ctx, silo.data_ptr(),
                                                                         act.data_ptr(), status.data_ptr(),
                                                                         perm.data_ptr(), off.data_ptr()))}
            if rep:
                for what, v in t.items():
                    ms.setdefault(name, {}).setdefault(what, []).append(v)
            if rep == args.reps:
                e.synchronize()
                res["shapes"].setdefault(name, {})["picks"] = np.bincount(pick[:m].cpu().numpy(), minlength=5).tolist()
    for name, d in ms.items():
        r = res["shapes"][name]
        r["messages"] = batches[name][1]
        for what, v in d.items():
            r[what + "_ms_median"] = round(float(np.median(v)), 4)
            r[what + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    e.set_kernel_timing(1)
    e.kernel_times_reset()
    e.workers_clear()
    fill()
    with torch.cuda.stream(stream):
        select("hot_half")
    e.synchronize()
    res["kernels_hot_half_ms"] = {k: round(v[1], 4) for k, v in sorted(e.kernel_times().items(), key=lambda kv: -kv[1][1])
                                  if v[1] >= 0.001}
    e.set_stream(None)
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
