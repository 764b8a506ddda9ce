#!/usr/bin/env python3
"""The gateway stage on one MI355X.

For --clients open clients (default 2^16 and 2^20; a third of them disconnected) and --msgs messages (default 2^24)
of which 1 %, 50 % and 100 % target a client (the rest target grains; a tenth of all senders are clients):
  deliver      gd_gateway_deliver_device with perm / offsets over 8 gateway senders
  send_queues  gd_gateway_send_queues_device over 8 silos, 4 sender queues and the 8 gateway senders
  ingress      gd_gateway_ingress_device with route_idx / n_route / route_keys, a third of the messages Responses
Each is the median of --reps runs with the spread (device events on the handle's stream, after one warm-up run that
also records the routes), beside a device-to-device copy that moves the bytes the pass must read and write:
deliver 8 B (the target's TypeCodeData) + 9 B out + 8 B of bucket ids and perm a message, and 16 B more of the key,
a 32-B slot, a 16-B client value and the sender's 8 B for a client-targeted one, 24 + 32 + 8 B for a recorded route;
send_queues 13 B more (silo, status, category, ttl is absent); ingress 17 B in + 5 B out + 8 B of flags a message,
16 + 32 B for a route lookup, 28 B for a rerouted one.  The copy is that byte count measured live, not a bound on a
pass whose accesses are gathers.  Prints one JSON line; --out also writes it to a file.
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

N_SENDERS, N_SILOS, N_QUEUES = 8, 8, 4


def timed(stream, reps, call):
    ms = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = ms[1:]                                              # the first run warms up
    return round(float(np.median(ms)), 4), [round(min(ms), 4), round(max(ms), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--msgs", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    n = args.msgs
    res = {"metric": "gateway stage", "n_gpus": 1, "data": "synthetic",
           "config": {"msgs": n, "reps": args.reps, "n_senders": N_SENDERS, "n_queues": N_QUEUES}, "clients": {}}
    stream = torch.cuda.Stream()
    gen = torch.Generator(device=dev).manual_seed(0x6A7E)

    def keys(ids, cat):
        k = torch.zeros((ids.numel(), 3), dtype=torch.int64, device=dev)
        k[:, 1] = ids
        k[:, 2] = (cat << 56) | 77
        return k

    for C_ in args.clients:
        e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
        e.set_stream(stream.cuda_stream)
        e.gateway_configure(N_SENDERS, 10_000_000, 50_000_000, 2 * C_)
        e.send_configure(np.arange(N_SILOS, dtype=np.int32) * 7919 + 1, N_QUEUES)
        r = {}
        with torch.cuda.stream(stream):
            cl = keys(torch.arange(1, C_ + 1, device=dev), 4)
            hd = torch.arange(C_, dtype=torch.int32, device=dev)
            e.gateway_open_device(cl.data_ptr(), hd.data_ptr(), C_, None, None, None, None)
            e.gateway_close_device(cl[::3].contiguous().data_ptr(), None, (C_ + 2) // 3, 1000, None)
            sender_is_client = torch.rand(n, device=dev, generator=gen) < 0.1
            who = torch.randint(1, C_ + 1, (n,), device=dev, generator=gen)
            sending = torch.where(sender_is_client[:, None], keys(who, 4), keys(who, 3)).contiguous()
            ssilo = torch.randint(0, N_SILOS, (n,), device=dev, generator=gen).to(torch.int32)
            silo = torch.randint(0, N_SILOS, (n,), device=dev, generator=gen).to(torch.int32)
            direction = (torch.rand(n, device=dev, generator=gen) < 1 / 3).to(torch.uint8)
            st, hd_o = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
            sd, q, perm = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
            off = torch.empty(N_QUEUES + N_SENDERS + 5, dtype=torch.int32, device=dev)
            o_silo, r_idx = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
            r_n, r_keys = torch.empty(1, dtype=torch.int32, device=dev), torch.empty((n, 3), dtype=torch.int64, device=dev)

            def copy_ms(nbytes):
                src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                return timed(stream, args.reps, lambda: dst.copy_(src))

            for pct in (1, 50, 100):
                to_client = torch.rand(n, device=dev, generator=gen) < pct / 100
                tid = torch.randint(1, C_ + 1, (n,), device=dev, generator=gen)
                target = torch.where(to_client[:, None], keys(tid, 4), keys(tid, 3)).contiguous()
                k = int(to_client.sum())
                routes = int((to_client & sender_is_client).sum())
                resp = int((to_client & sender_is_client & (direction == 1)).sum())
                calls = {
                    "deliver": (lambda: e.gateway_deliver_device(target.data_ptr(), sending.data_ptr(), ssilo.data_ptr(), None, n, 2000, st.data_ptr(),
                        hd_o.data_ptr(), sd.data_ptr(), perm.data_ptr(), off.data_ptr()),
                        25 * n + 72 * k + 64 * routes),
                    "send_queues": (lambda: e.gateway_send_queues_device(target.data_ptr(), sending.data_ptr(), ssilo.data_ptr(), silo.data_ptr(), None, None,
                        None, n, 2000, st.data_ptr(), q.data_ptr(), hd_o.data_ptr(), perm.data_ptr(), off.data_ptr()),
                        38 * n + 72 * k + 64 * routes),
                    "ingress": (lambda: e.gateway_ingress_device(target.data_ptr(), sending.data_ptr(), direction.data_ptr(), None, n, 0, st.data_ptr(),
                        o_silo.data_ptr(), r_idx.data_ptr(), r_n.data_ptr(), r_keys.data_ptr()),
                        30 * n + 48 * resp + 28 * (n - resp)),
                }
                for name, (call, nbytes) in calls.items():
                    med, spread = timed(stream, args.reps, call)
                    cmed, cspread = copy_ms(nbytes)
                    r[f"{name}_{pct}"] = {"ms_median": med, "ms_min_max": spread, "bytes": int(nbytes),
                                          "copy_ms_median": cmed, "copy_ms_min_max": cspread,
                                          "client_targeted": k, "routes_recorded": routes}
        e.synchronize()
        r["count"] = list(e.gateway_count())
        e.set_stream(None)
        e.close()
        res["clients"][str(C_)] = r
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
