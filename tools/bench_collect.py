#!/usr/bin/env python3
"""The activation collector on one MI355X.

For --acts contexts (default 2^20 and 2^24), every context Valid, inactive and scheduled, one-minute quantum:
  idle_10 / idle_100         gd_collect_idle_device with 10 % / 100 % of the event bytes BECAME_IDLE
  stale_{1,50}_q{1,8}        gd_collect_scan_stale_device with 1 % / 50 % of the contexts due, over 1 and 8 quanta
                             (8: the list is ordered by the bucketing); half of the due are condemned
  touch_uniform / touch_zipf gd_collect_touch_device for --msgs messages (default 16M), uniform and Zipf(1.1)
Each is the median of --reps runs with the spread (device events on the handle's stream, the state restored from a
pristine copy before every run, untimed), beside a device-to-device copy that moves the bytes the pass must read
and write: 1 B a context + 25 B an idle one; 9 B a context + 55 B a due one + 4 B a condemned one; 6 B a message +
17 B a message's context words, 8 B more where the ticket moves.  The copy is the byte count measured live, not a
bound on a pass whose accesses are gathers.  Prints one JSON line; --out also writes it to a file.
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

Q = 600_000_000
T0 = 636_000_000_000_000_000


def zipf(n, acts, dev, gen):
    w = 1.0 / torch.arange(1, acts + 1, device=dev, dtype=torch.float64) ** 1.1
    cdf = torch.cumsum(w / w.sum(), 0)
    return torch.searchsorted(cdf, torch.rand(n, device=dev, generator=gen, dtype=torch.float64)).clamp_(max=acts - 1)


def timed(stream, reps, restore, call):
    ms = []
    for _ in range(reps + 1):
        restore()
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
    ap.add_argument("--acts", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--msgs", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(0xC011)
    res = {"metric": "activation collector", "n_gpus": 1, "data": "synthetic",
           "config": {"msgs": args.msgs, "reps": args.reps, "quantum_ticks": Q}, "acts": {}}
    with torch.cuda.stream(stream):
        for A in args.acts:
            now = T0 + 12345
            nxt = ((now - 1) // Q + 1) * Q
            i64 = lambda v: torch.full((A,), v, dtype=torch.int64, device=dev)
            age, idle0, flags0 = i64(2 * Q), i64(now - 10 * Q), torch.zeros(A, dtype=torch.uint8, device=dev)
            cf0, nr = torch.zeros(A, dtype=torch.uint8, device=dev), torch.zeros(A, dtype=torch.int32, device=dev)
            t_w, bi_w, fl_w, cf_w = i64(0), i64(0), flags0.clone(), cf0.clone()
            st = e.collect_state(t_w.data_ptr(), bi_w.data_ptr(), None, age.data_ptr(), fl_w.data_ptr())
            out, out_n = torch.empty(A, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
            verdict = torch.empty(A, dtype=torch.uint8, device=dev)
            u = torch.rand(A, device=dev, generator=gen)
            r = {}

            def copy_ms(nbytes):
                src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                return timed(stream, args.reps, lambda: None, lambda: dst.copy_(src))

            def case(name, ticket0, call, nbytes, next_ticket):
                def restore():
                    t_w.copy_(ticket0), bi_w.copy_(idle0), fl_w.copy_(flags0), cf_w.copy_(cf0)
                    e.collect_configure(Q, next_ticket)
                med, spread = timed(stream, args.reps, restore, call)
                cmed, cspread = copy_ms(nbytes)
                r[name] = {"ms_median": med, "ms_min_max": spread, "bytes": int(nbytes), "copy_ms_median": cmed,
                           "copy_ms_min_max": cspread}

            # idle: every context holds the ticket a touch at `now` gives, so the rule ends at "same ticket"
            held = i64(((now + 2 * Q - 1) // Q + 1) * Q)
            for pct in (10, 100):
                ev = (u < pct / 100).to(torch.uint8)
                k = int(ev.sum())
                case(f"idle_{pct}", held, lambda ev=ev: e.collect_idle_device(st, A, ev.data_ptr(), now, None),
                     A + 25 * k, nxt)
            # scan_stale: due tickets spread over the n_q quanta behind `now`; half of the due are stale
            for n_q in (1, 8):
                nxt_q = nxt - n_q * Q
                for pct in (1, 50):
                    due = u < pct / 100
                    k = int(due.sum())
                    which = torch.randint(0, n_q, (A,), device=dev, generator=gen)
                    ticket0 = torch.where(due, nxt_q + which * Q, nxt + 5 * Q)
                    idle_half = torch.where(torch.rand(A, device=dev, generator=gen) < 0.5, now - 10 * Q, now)
                    idle0.copy_(idle_half)
                    case(f"stale_{pct}_q{n_q}", ticket0,
                         lambda: e.collect_scan_stale_device(st, A, cf_w.data_ptr(), nr.data_ptr(), None, now,
                                                             out.data_ptr(), out_n.data_ptr(), verdict.data_ptr()),
                         9 * A + 55 * k + 4 * (k // 2), nxt_q)
            idle0.fill_(now - 10 * Q)
            # touch: every context scheduled one quantum ago, so each touched ticket moves
            n = args.msgs
            prev = i64(((now + Q - 1) // Q + 1) * Q)
            turn = torch.full((n,), 1, dtype=torch.uint8, device=dev)
            for kind in ("uniform", "zipf"):
                ctx = (torch.randint(0, A, (n,), device=dev, generator=gen) if kind == "uniform"
                       else zipf(n, A, dev, gen)).to(torch.int32)
                distinct = int(torch.unique(ctx).numel())
                case(f"touch_{kind}", prev,
                     lambda ctx=ctx: e.collect_touch_device(st, A, cf_w.data_ptr(), ctx.data_ptr(), turn.data_ptr(), n,
                                                            now + Q, None),
                     6 * n + 17 * n + 8 * distinct, nxt)
                r[f"touch_{kind}"]["distinct_contexts"] = distinct
            res["acts"][str(A)] = r
    e.synchronize()
    e.set_stream(None)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
