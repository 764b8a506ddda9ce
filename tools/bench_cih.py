#!/usr/bin/env python3
"""GD_OPT_WALK_INVALIDATION bench: what stepping over a CacheInvalidationHeader costs the decoder and
the two planners, per launch (gd_set_kernel_timing events), medians of --reps runs of --steps launches.

Workload: --frames request frames of the forward writer's bench shape (tools/bench_forward.py: headerLength 122, all
Request, bodies 0..63 B).  A fraction of them carries an invalidation field in front of Category: one long-keyed entry
(84 B, which pushes the last 22 header bytes past the 192 B a stage keeps of a frame in LDS), or -- to tell the walk
from the reads past the window -- a count of 0 (4 B, everything stays inside the window).

  (1) option off, this library against --parent-lib (the parent commit's build) on the field-free batch: the same
      code, so the ratio must lie inside the parent's own run-to-run spread.  The parent is measured in two processes,
      one before and one after this library's; its spread is the larger of the repetitions' (max - min) / median and
      the two processes' difference.
  (2) option on with 0 %, 1 % and 100 % of the frames carrying one entry, and 100 % carrying a count of 0, against
      option off on the same batch with the field cut out (the field-free batch: same seed, same frames).

Kernels: k_decode_frames<false>, k_decode_frames<true> (the turn headers), k_enc_plan, k_rsp_plan.  Every
measurement runs in a child process of its own, one at a time.

usage: python tools/bench_cih.py [--frames 4194304] [--steps 5] [--warmup 2] [--reps 5] [--parent-lib PATH]
                                 [--out profiles/cih.json]
"""
import argparse
import json
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_decode_frames", "k_decode_frames_turn", "k_enc_plan", "k_rsp_plan")
ONE_ENTRY = struct.pack("<i", 1) + bytes(range(24)) + struct.pack("<QQQi", 5, 6, (3 << 56) + 77, -1) + \
    struct.pack("<QQQi", 8, 9, 0, -1)
NO_ENTRY = struct.pack("<i", 0)
CASES = (("one_entry_0pct", 0.0, ONE_ENTRY), ("one_entry_1pct", 0.01, ONE_ENTRY), ("one_entry_100pct", 1.0, ONE_ENTRY),
         ("count_zero_100pct", 1.0, NO_ENTRY))


def build(n, seed, p, field):
    """tools/bench_forward.py's frames; a fraction p of them with `field` behind the mask.  The same seed gives the
    same frames whatever p and field are."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import frames_synth as FS
    rng = np.random.default_rng(seed)
    keys = np.zeros((n, 3), dtype=np.uint64)
    keys[:, 1] = rng.integers(0, 1 << 20, size=n)
    keys[:, 2] = np.uint64((3 << 56) + 77)
    hdr, _, hlen = FS.build_frames(keys, rng, body_len=0)
    hdr = hdr.reshape(n, hlen)
    bl = rng.integers(0, 64, size=n).astype(np.int64)
    hdr[:, 4:8] = bl.astype("<i4").view(np.uint8).reshape(n, 4)
    has = rng.random(n) < p
    fb = len(field)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(hlen + bl + fb * has, out=off[1:])
    buf = np.zeros(int(off[n]), dtype=np.uint8)
    for sel, cols, src in ((~has, np.arange(hlen), hdr), (has, np.arange(12), hdr[:, :12]),
                           (has, 12 + fb + np.arange(hlen - 12), hdr[:, 12:])):
        idx = np.flatnonzero(sel)
        for a in range(0, len(idx), 1 << 18):
            i = idx[a:a + (1 << 18)]
            buf[(off[i, None] + cols).reshape(-1)] = src[i].reshape(-1)
    ih = np.flatnonzero(has)
    for a in range(0, len(ih), 1 << 18):
        i = ih[a:a + (1 << 18)]
        buf[(off[i, None] + 12 + np.arange(fb)).reshape(-1)] = np.tile(np.frombuffer(field, np.uint8), len(i))
        hl = hdr[i, 0:4].copy().view("<i4").reshape(-1) + fb
        buf[(off[i, None] + np.arange(4)).reshape(-1)] = hl.astype("<i4").view(np.uint8)
        buf[off[i] + 8] |= 2                                          # Headers.CACHE_INVALIDATION_HEADER
    return buf, off[:n].astype(np.uint64), int(off[n]), int(has.sum())


def measure(args, case, walk):
    """One batch, one option value: per kernel the repetitions' medians (us a launch)."""
    import torch
    from orleans_amd import graindispatch as g
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_encode as BE
    name, p, field = case
    n = args.frames
    dev = torch.device("cuda:0")
    buf, off, nbytes, n_has = build(n, 0x5EED0027, p, field)
    rng = np.random.default_rng(1)
    e = g.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=0)
    if walk:
        e.set_option(18, 1)                                           # GD_OPT_WALK_INVALIDATION
    e.encode_configure(BE.SILOS, ["BenchmarkGrains.Ping.PingGrain"])
    e.respond_configure([])
    e.activation_ids_set(np.arange(BE.N_ACT, dtype=np.uint32), rng.integers(1, 1 << 62, size=(BE.N_ACT, 3)).astype(np.uint64))
    t = lambda a: torch.from_numpy(a).to(dev)
    d_buf, d_off = t(buf), t(off.view(np.int64))
    d_silo = t(rng.integers(0, len(BE.SILOS), size=n).astype(np.int32))
    d_act = t(rng.integers(0, BE.N_ACT, size=n).astype(np.int32))
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_kind = torch.ones(n, dtype=torch.uint8, device=dev)
    cap = nbytes + 64 * n + 64
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_est = torch.empty(n, dtype=torch.uint8, device=dev)
    size = lambda dt, sh: n * np.dtype(dt).itemsize * int(np.prod(sh, dtype=np.int64))
    ff = {k: torch.empty(size(dt, sh), dtype=torch.uint8, device=dev) for k, (dt, sh) in g.FRAME_FIELDS.items()}
    tf = {k: torch.empty(size(dt, ()), dtype=torch.uint8, device=dev) for k, dt in g.FRAME_TURN_FIELDS.items()}
    pf, pt = {k: v.data_ptr() for k, v in ff.items()}, {k: v.data_ptr() for k, v in tf.items()}
    suffix = "_cih" if walk else ""

    def run():
        e.decode_frames_device(d_buf.data_ptr(), nbytes, d_off.data_ptr(), n, pf)
        e.decode_frames_turn_device(d_buf.data_ptr(), nbytes, d_off.data_ptr(), n, pf, pt)
        e.encode_frames_device(d_buf.data_ptr(), nbytes, d_off.data_ptr(), n, d_silo.data_ptr(), d_act.data_ptr(),
                               d_st.data_ptr(), None, None, None, d_out.data_ptr(), cap, d_out_off.data_ptr(), d_est.data_ptr())
        e.respond_frames_device(d_buf.data_ptr(), nbytes, d_off.data_ptr(), n, d_kind.data_ptr(), None, None, None, None,
                                None, None, d_out.data_ptr(), cap, d_out_off.data_ptr(), d_est.data_ptr())

    for _ in range(args.warmup):
        run()
    e.synchronize()
    flags = ff["flags"].cpu().numpy().view(np.uint32)
    decoded = int((flags & 1).sum())
    reps = []
    for _ in range(args.reps):
        e.set_kernel_timing(True)
        e.kernel_times_reset()
        for _ in range(args.steps):
            run()
        e.synchronize()
        kt = e.kernel_times()
        e.set_kernel_timing(False)
        reps.append({k: kt[k + suffix][1] / kt[k + suffix][0] * 1e3 for k in KERNELS})
    e.close()
    med = {k: float(np.median([r[k] for r in reps])) for k in KERNELS}
    spread = {k: (max(r[k] for r in reps) - min(r[k] for r in reps)) / med[k] for k in KERNELS}
    return {"case": name, "walk": int(walk), "frames": n, "frames_with_field": n_has, "bytes": nbytes,
            "frames_decoded": decoded, "us": {k: round(v, 2) for k, v in med.items()},
            "rep_spread": {k: round(v, 4) for k, v in spread.items()}}


def child(args, case, walk, lib=None):
    env = dict(os.environ)
    if lib:
        env["GRAINDISPATCH_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", case, "--walk", str(int(walk)), "--frames", str(args.frames),
           "--steps", str(args.steps), "--warmup", str(args.warmup), "--reps", str(args.reps)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"# {case} walk={int(walk)} lib={lib or 'this'}: {out['us']}", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cih.json"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--walk", type=int, default=0)
    args = ap.parse_args()
    assert args.reps >= 5, "medians of at least 5 runs"
    if args.worker:
        sys.path.insert(0, ROOT)
        print(json.dumps(measure(args, next(c for c in CASES if c[0] == args.worker), bool(args.walk))), flush=True)
        return
    free = CASES[0][0]                                                # the field-free batch
    rec = {"metric": "GD_OPT_WALK_INVALIDATION: kernel time a launch (us), medians of the repetitions",
           "frames": args.frames, "steps": args.steps, "reps": args.reps}
    parent = [child(args, free, False, args.parent_lib)] if args.parent_lib else []
    off = child(args, free, False)
    if args.parent_lib:
        parent.append(child(args, free, False, args.parent_lib))
        same = {}
        for k in KERNELS:
            a, b = parent[0]["us"][k], parent[1]["us"][k]
            pm = (a + b) / 2
            spread = max(abs(a - b) / pm, parent[0]["rep_spread"][k], parent[1]["rep_spread"][k])
            ratio = off["us"][k] / pm
            same[k] = {"parent_us": [a, b], "branch_us": off["us"][k], "ratio": round(ratio, 4),
                       "parent_spread": round(spread, 4), "inside": bool(abs(ratio - 1) <= spread)}
        rec["option_off_against_parent"] = same
    rec["option_off_field_free"] = off
    rec["option_on"] = []
    for case in CASES:
        on = child(args, case[0], True)
        on["over_option_off_cut"] = {k: round(on["us"][k] / off["us"][k], 4) for k in KERNELS}
        rec["option_on"].append(on)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
