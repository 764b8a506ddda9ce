"""GPU parity for the turn completion and message pump: gd_turns_complete / gd_wait_list_merge
and their device forms through the C ABI against the literal restatement of
Dispatcher.OnActivationCompletedRequest (_pump_ref.pump_loop / merge_loop), every output bit for bit, dtype
included."""
import ctypes as C

import numpy as np
import pytest

import _pump_ref as P
import _turns_ref as R
from test_pump_ref import Lifecycle

pytestmark = pytest.mark.gpu

THIN = 32                        # gd_pump.h PUMP_THIN: completions + list length below it = one lane a context
TILE = 4096                      # the bucketing's and the scan's tile; k_pump_starts' is 2048
V, HAS, RRO, REENT = R.CTX_VALID, R.CTX_HAS_RUNNING, R.CTX_RUNNING_READ_ONLY, R.CTX_REENTRANT
RO, AI, CC = R.MSG_READ_ONLY, R.MSG_ALWAYS_INTERLEAVE, P.MSG_CALL_CHAIN
ISR, PO = P.DONE_IS_RUNNING, P.DONE_PUMP_ONLY


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


@pytest.fixture(scope="module")
def eng(gd):
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        yield e


def _check(got, want, names=P.NAMES):
    assert len(got) == len(want) == len(names)
    for name, a, b in zip(names, got, want):
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a, b, err_msg=name)


def _call(e, b, **kw):
    return e.turns_complete(b.done_ctx, b.n_ctx, b.ctx_flags, b.num_running, b.offsets, b.wflags, b.done_flags, b.wmsg, **kw)


def _run(e, b):
    want = P.pump_loop(b)
    _check(_call(e, b), want)
    return want


@pytest.mark.parametrize("n_ctx", [1, 7, 1025, 70001])
@pytest.mark.parametrize("n_done", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 200003])
def test_shapes_mixed_batch(eng, n_done, n_ctx):
    """Uniform targets for even n_done + n_ctx, Zipf otherwise; done_flags NULL for every third shape."""
    rng = np.random.default_rng(n_done * 31 + n_ctx)
    b = P.mixed_pump(rng, n_done, n_ctx, "zipf" if (n_done + n_ctx) % 2 else "uniform", flags=(n_done + n_ctx) % 3 != 0)
    _run(eng, b)


def test_list_lengths_around_the_wave_and_the_thin_bound(eng):
    """Lists of 0, 1, 63, 64, 65 entries and, with 1 and 2 completions, completions + length = THIN - 1, THIN,
    THIN + 1 -- under four kinds of context: the list drains, stops at a writer, runs on read-only, is idle."""
    lens, flags, nrun, comps = [], [], [], []
    for k in (1, 2):
        for ln in (0, 1, 63, 64, 65, THIN - 1 - k, THIN - k, THIN + 1 - k):
            for f, nr in ((V | HAS | REENT, 2), (V | HAS, 1), (V | HAS | RRO, 3), (V, k)):
                lens.append(ln), flags.append(f), nrun.append(nr), comps.append(k)
    n_ctx = len(lens)
    rng = np.random.default_rng(8)
    off = np.zeros(n_ctx + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    wf = P.wait_flags(rng, int(off[-1]), 0.7, 0.02)
    ctx = rng.permutation(np.repeat(np.arange(n_ctx), comps)).astype(np.uint32)
    df = (rng.random(len(ctx)) < 0.6).astype(np.uint8) * ISR
    want = _run(eng, P.PumpBatch(ctx, n_ctx, flags, nrun, off, wf, df))
    assert (want[2] == np.array(lens)).sum() >= n_ctx // 4 and (want[2] == 0).any()


def test_optional_arrays(eng):
    b = P.mixed_pump(np.random.default_rng(3), 5000, 300, "zipf")
    want = P.pump_loop(b)
    _check(_call(eng, b, started_by=False), want[:5] + want[6:], P.NAMES[:5] + P.NAMES[6:])
    _check(_call(eng, b, starts=False), want[:6], P.NAMES[:6])
    _check(_call(eng, b, started_by=False, starts=False), want[:5], P.NAMES[:5])
    b.done_flags = np.zeros(b.n_done, np.uint8)
    got = _call(eng, b)
    b.done_flags = None
    _check(_call(eng, b), got)                               # NULL = all 0
    _check(got, P.pump_loop(b))
    _check(_call(eng, b, wait_cap=len(b.wflags) + 1000), got)   # a capacity above the lists' length


def _hot(n_done, flags, nr, wflags, done_flags):
    return P.PumpBatch(np.zeros(n_done, np.uint32), 1, [flags], [nr], [0, len(wflags)], wflags, done_flags)


@pytest.mark.parametrize("at", [64 * 70, 64 * 70 + 1, TILE, TILE - 1, 0, 3 * TILE + 16])
def test_hot_context_is_running_in_the_middle(eng, at):
    """One context takes all 3 * 4096 + 17 completions; the one that equals Running sits at a 64 edge / a tile
    edge: the head (a writer) starts there; nr reaches 0 near the end and each later completion starts one more."""
    n = 3 * TILE + 17
    df = np.zeros(n, np.uint8)
    df[at] = ISR
    df[5::97] |= PO
    lowering = int((df & PO == 0).sum())
    wf = np.array([0] + [RO] * 200 + [0] + [RO] * 10, np.uint8)
    want = _run(eng, _hot(n, V | HAS, lowering - 3, wf, df))
    nsb = want[5]
    assert nsb[at] >= 1 and int(nsb.sum()) > int(nsb[at]) and want[4][0] & P.PUMP_BECAME_IDLE


def test_hot_context_inconsistent_counts_walk_serially(eng):
    """num_running far below the completions: nr reaches 0 again and again, one start each time."""
    n = TILE + 65
    wf = np.zeros(3000, np.uint8)
    want = _run(eng, _hot(n, V | HAS, 5, wf, np.zeros(n, np.uint8)))
    assert int(want[2][0]) == 3000 and int(want[5].max()) == 1


@pytest.mark.parametrize("n_list", [200003, 64 * 100, 2048 * 3, 2048 * 3 + 1])
def test_one_completion_of_a_reentrant_context_drains_the_list(eng, n_list):
    """k_pump_starts' balancing: one completion owns every start; lists ending at a 64 and at a tile edge."""
    rng = np.random.default_rng(n_list)
    b = P.PumpBatch([3, 0, 3], 4, [V | HAS, V, V, V | HAS | REENT], [1, 0, 0, 2], [0, 2, 2, 2, 2 + n_list],
                    np.concatenate([[0, 0], P.wait_flags(rng, n_list)]).astype(np.uint8), [ISR, ISR, 0])
    want = _run(eng, b)
    assert want[5].tolist() == [n_list, 1, 0] and want[6].tolist() == list(range(2, 2 + n_list)) + [0]


@pytest.mark.parametrize("stop", [64, 64 * 5, 64 * 5 - 1, 64 * 5 + 1, 2048, 0])
def test_blocked_head_at_a_wave_edge(eng, stop):
    wf = np.full(64 * 40, AI, np.uint8)
    wf[stop] = RO                                            # Running is a writer: the reader waits
    want = _run(eng, _hot(70, V | HAS, 80, wf, np.zeros(70, np.uint8)))
    assert int(want[2][0]) == stop and want[5].tolist() == [stop] + [0] * 69


def test_deterministic(eng):
    b = P.mixed_pump(np.random.default_rng(9), 3 * TILE + 17, 40, "zipf", mean_len=40.0)
    _check(_call(eng, b), _call(eng, b))


# ---- gd_wait_list_merge ----------------------------------------------------------------------------

def _merge_case(rng, n_ctx, n, old=True, all_dequeued=False, keys=False, ids=True):
    lens = rng.poisson(2.0, n_ctx)
    off = np.zeros(n_ctx + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    omsg = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
    ofl = rng.integers(0, 16, total).astype(np.uint8)
    ndq = lens.astype(np.uint32) if all_dequeued else rng.integers(0, lens + 1).astype(np.uint32)
    key = np.where(rng.random(n) < 0.6, rng.integers(0, n_ctx, n), n_ctx)
    wperm = np.argsort(key, kind="stable").astype(np.uint32)
    woff = np.zeros(n_ctx + 2, np.uint32)
    woff[1:] = np.cumsum(np.bincount(key, minlength=n_ctx + 1))
    kw = dict(msg_id=rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) if ids else None, id_base=77,
              msg_flags=rng.integers(0, 8, n).astype(np.uint8))
    if keys:
        ta = rng.integers(0, 1 << 60, (n, 3), dtype=np.uint64)
        sa = ta.copy()
        d = rng.random(n) < 0.5
        sa[d, rng.integers(0, 3, int(d.sum()))] += np.uint64(1)
        kw.update(target_activation=ta, sending_activation=sa, chain=True)
    head = (n_ctx, off, omsg, ofl, ndq) if old else (n_ctx, None, None, None, None)
    return head + (wperm, woff), kw


def _merge_check(e, args, kw, cap=None):
    off, msg, fl, total = P.merge_loop(*args, cap=cap, **kw)
    g_off, g_msg, g_fl, g_total = e.wait_list_merge(*args, cap=cap, **kw)
    keep = len(msg)
    assert g_total == total and g_off.dtype == off.dtype and g_msg.dtype == msg.dtype and g_fl.dtype == fl.dtype
    np.testing.assert_array_equal(g_off, off)
    np.testing.assert_array_equal(g_msg[:keep], msg)
    np.testing.assert_array_equal(g_fl[:keep], fl)
    return total


@pytest.mark.parametrize("n_ctx,n", [(1, 0), (7, 65), (1025, TILE + 1), (70001, 200003)])
def test_merge_shapes(eng, n_ctx, n):
    rng = np.random.default_rng(n_ctx + n)
    _merge_check(eng, *_merge_case(rng, n_ctx, n, ids=n % 2 == 1))


def test_merge_edges(eng):
    rng = np.random.default_rng(12)
    _merge_check(eng, *_merge_case(rng, 300, 2000, old=False))                 # empty old list
    args, kw = _merge_case(rng, 300, 2000, all_dequeued=True)                  # everything dequeued
    total = _merge_check(eng, args, kw)
    assert total == int(args[6][300])                                          # = the batch's WAIT messages
    args, kw = _merge_case(rng, 300, 2000, keys=True)                          # the call-chain bit from keys
    _merge_check(eng, args, kw)
    assert (P.merge_loop(*args, **kw)[2] & CC).any()
    kw["chain"] = False                                                        # ... only when the option is on
    _merge_check(eng, args, kw)
    args, kw = _merge_case(rng, 300, 2000)                                     # n_dequeued NULL
    _merge_check(eng, args[:4] + (None,) + args[5:], kw)


def test_merge_capacity_one_short(eng, gd):
    """Device form: nothing is written at or past the capacity, and the needed total is reported."""
    import torch
    rng = np.random.default_rng(13)
    args, kw = _merge_case(rng, 200, 3000)
    n_ctx, off, omsg, ofl, ndq, wperm, woff = args
    w_off, w_msg, w_fl, total = P.merge_loop(*args, **kw)
    cap = total - 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_in = [dev(a) for a in (off, omsg, ofl, ndq, wperm, woff, kw["msg_id"], kw["msg_flags"])]
    d_off = torch.zeros((n_ctx + 1) * 4, dtype=torch.uint8, device="cuda")
    d_msg = torch.full(((total + 8) * 4,), 0xAB, dtype=torch.uint8, device="cuda")
    d_fl = torch.full((total + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    d_total = torch.zeros(4, dtype=torch.uint8, device="cuda")
    old = eng.wait_list_device(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr())
    eng.wait_list_merge_device(old, d_in[3].data_ptr(), n_ctx, d_in[4].data_ptr(), d_in[5].data_ptr(), len(wperm),
                               d_in[6].data_ptr(), 0, d_in[7].data_ptr(), None, None, False, cap, d_off.data_ptr(),
                               d_msg.data_ptr(), d_fl.data_ptr(), d_total.data_ptr())
    eng.synchronize()
    assert int(d_total.cpu().numpy().view(np.uint32)[0]) == total
    np.testing.assert_array_equal(d_off.cpu().numpy().view(np.uint32), w_off)
    msg, fl = d_msg.cpu().numpy().view(np.uint32), d_fl.cpu().numpy()
    np.testing.assert_array_equal(msg[:cap], w_msg[:cap])
    np.testing.assert_array_equal(fl[:cap], w_fl[:cap])
    assert (msg[cap:] == 0xABABABAB).all() and (fl[cap:] == 0xAB).all()


# ---- the cycle on the device -------------------------------------------------------------------------

def test_cycle_on_the_device(eng, gd):
    """Four steps of gd_turns_device -> gd_wait_list_merge_device -> gd_turns_complete_device on device arrays,
    nothing read back between the calls; the inputs are those of the reference lifecycle (run first, on the
    CPU, beside the Activation objects), the results are compared with it at the end."""
    import torch
    n_ctx, sizes = 500, (4000, 700, 6000, 3000)
    life = Lifecycle(41, n_ctx)
    flags0, nr0 = life.flags.copy(), life.nr.copy()
    for n in sizes:
        life.step(n)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    z = lambda count, width: torch.zeros(max(count, 1) * width, dtype=torch.uint8, device="cuda")
    ins = [{k: dev(v) for k, v in s.items() if k in ("ctx", "msg_flags", "ta", "sa", "ids", "done_ctx", "done_flags")}
           for s in life.log]
    flips = [torch.from_numpy(s["flips"]).cuda() for s in life.log]
    cap = sum(sizes)
    d_flags, d_nr = dev(flags0), dev(nr0)
    old, d_ndq, keep = None, None, []
    # the calls and the arithmetic between them on one stream
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            keep, d_flags, d_nr = _cycle_steps(eng, torch, life, ins, flips, n_ctx, cap, d_flags, d_nr, z)
        eng.synchronize()
    finally:
        eng.set_stream(None)
    _cycle_compare(life, keep, d_flags, d_nr, n_ctx, cap)


def _cycle_steps(eng, torch, life, ins, flips, n_ctx, cap, d_flags, d_nr, z):
    old, d_ndq, keep = None, None, []
    for s, d, flip in zip(life.log, ins, flips):
        n, n_done = len(s["ctx"]), len(s["done_ctx"])
        d_turn, d_nro, d_run = z(n, 1), z(n_ctx, 4), z(n_ctx, 4)
        d_start, d_ns, d_wp, d_wo = z(n, 4), z(1, 4), z(n, 4), z(n_ctx + 2, 4)
        st = eng.turn_state_device(d_flags.data_ptr(), d_nr.data_ptr(), None, 0, 0, 2, True)
        eng.turns_device(d["ctx"].data_ptr(), None, None, None, None, d["msg_flags"].data_ptr(), d["ta"].data_ptr(),
                         d["sa"].data_ptr(), n, n_ctx, st, d_turn.data_ptr(), d_nro.data_ptr(), d_run.data_ptr(),
                         d_start.data_ptr(), d_ns.data_ptr(), d_wp.data_ptr(), d_wo.data_ptr())
        # the host's part between the calls, as device arithmetic: Running's flags of the contexts gd_turns gave a
        # Running, and the activations that turned Valid
        run = d_run.view(torch.int32)
        has = run != -1
        ro = (d["msg_flags"][run.clamp(min=0).long()] & 1) != 0
        d_flags = d_flags | (has * 4).to(torch.uint8) | ((has & ro) * 8).to(torch.uint8)
        d_flags[flip] &= 0xFC
        n_off, n_msg, n_fl, d_tot = z(n_ctx + 1, 4), z(cap, 4), z(cap, 1), z(1, 4)
        eng.wait_list_merge_device(old, None if d_ndq is None else d_ndq.data_ptr(), n_ctx, d_wp.data_ptr(),
                                   d_wo.data_ptr(), n, d["ids"].data_ptr(), 0, d["msg_flags"].data_ptr(),
                                   d["ta"].data_ptr(), d["sa"].data_ptr(), True, cap, n_off.data_ptr(), n_msg.data_ptr(),
                                   n_fl.data_ptr(), d_tot.data_ptr())
        old = eng.wait_list_device(n_off.data_ptr(), n_msg.data_ptr(), n_fl.data_ptr())
        o_fl, o_nr, d_ndq, d_rp, d_ev = z(n_ctx, 1), z(n_ctx, 4), z(n_ctx, 4), z(n_ctx, 4), z(n_ctx, 1)
        d_nsb, d_sp, d_nsp = z(n_done, 4), z(cap, 4), z(1, 4)
        eng.turns_complete_device(d["done_ctx"].data_ptr(), d["done_flags"].data_ptr(), n_done, n_ctx,
                                  d_flags.data_ptr(), d_nro.data_ptr(), old, cap, o_fl.data_ptr(), o_nr.data_ptr(),
                                  d_ndq.data_ptr(), d_rp.data_ptr(), d_ev.data_ptr(), d_nsb.data_ptr(), d_sp.data_ptr(),
                                  d_nsp.data_ptr())
        keep.append((d_start, d_ns, n_off, n_msg, n_fl, d_tot, d_sp, d_nsp, d_ndq, d_wp, d_wo, d_turn, d_run, d_flags,
                     d_nr, d_nro, d_nsb, d_rp, d_ev))
        d_flags, d_nr = o_fl, o_nr
    return keep, d_flags, d_nr


def _cycle_compare(life, keep, d_flags, d_nr, n_ctx, cap):
    host = lambda t, dt: t.cpu().numpy().view(dt)
    for s, k in zip(life.log, keep):
        d_start, d_ns, n_off, n_msg, n_fl, d_tot, d_sp, d_nsp = k[:8]
        np.testing.assert_array_equal(host(d_start, np.uint32)[:int(host(d_ns, np.uint32)[0])], s["turn_start"])
        assert int(host(d_tot, np.uint32)[0]) <= cap
        sp = host(d_sp, np.uint32)[:int(host(d_nsp, np.uint32)[0])]
        np.testing.assert_array_equal(host(n_msg, np.uint32)[sp], s["pump_start_ids"])
    assert any(len(s["pump_start_ids"]) for s in life.log)
    np.testing.assert_array_equal(host(d_nr, np.uint32), life.nr)
    np.testing.assert_array_equal(host(d_flags, np.uint8), life.flags)
    # the lists that are left: the last merge's, less what the last pump dequeued
    k = keep[-1]
    tot = int(host(k[5], np.uint32)[0])
    off, msg, fl, _ = P.merge_loop(n_ctx, host(k[2], np.uint32), host(k[3], np.uint32)[:tot], host(k[4], np.uint8)[:tot],
                                   host(k[8], np.uint32), np.zeros(0, np.uint32), np.zeros(n_ctx + 2, np.uint32))
    np.testing.assert_array_equal(off, life.off)
    np.testing.assert_array_equal(msg, life.wmsg)
    np.testing.assert_array_equal(fl, life.wfl)


# ---- argument errors and the capture refusal ---------------------------------------------------------

def test_argument_errors_and_capture_refusal(gd):
    import torch
    Pt = lambda a: C.c_void_p(a.ctypes.data)
    n_ctx = 4
    ctx, fl, nr = np.zeros(3, np.uint32), np.zeros(n_ctx, np.uint8), np.ones(n_ctx, np.uint32)
    off, wf = np.array([0, 1, 2, 2, 3], np.uint32), np.zeros(3, np.uint8)
    o8, o32 = [np.zeros(n_ctx, np.uint8) for _ in range(2)], [np.zeros(n_ctx, np.uint32) for _ in range(3)]
    lst, one = np.zeros(8, np.uint32), np.zeros(1, np.uint32)
    wl = gd.gd_wait_list(off.ctypes.data, None, wf.ctypes.data)
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        def call(h=e.h, wait=C.byref(wl), cap=3, flags=Pt(fl), start=None, n_start=None, done=Pt(ctx)):
            return gd.lib.gd_turns_complete(h, done, None, 3, n_ctx, flags, Pt(nr), wait, cap, Pt(o8[0]), Pt(o32[0]),
                                            Pt(o32[1]), Pt(o32[2]), Pt(o8[1]), None, start, n_start)
        assert call() == gd.GD_OK
        assert call(h=None) == gd.GD_EINVAL
        assert call(wait=None) == gd.GD_EINVAL
        assert call(cap=2) == gd.GD_EINVAL                   # the lists hold 3
        assert call(flags=None) == gd.GD_EINVAL
        assert call(done=None) == gd.GD_EINVAL
        assert call(start=Pt(lst)) == gd.GD_EINVAL           # start_pos without n_start
        assert call(n_start=Pt(one)) == gd.GD_EINVAL
        assert call(start=Pt(lst), n_start=Pt(one)) == gd.GD_OK
        nowf = gd.gd_wait_list(off.ctypes.data, None, None)
        assert call(wait=C.byref(nowf)) == gd.GD_EINVAL
        # the merge: one key array of the pair, an old list without its arrays, a NULL output
        wp, wo = np.zeros(2, np.uint32), np.array([0, 1, 1, 1, 2, 2], np.uint32)
        ta = np.zeros((2, 3), np.uint64)
        no, nm, nf = np.zeros(n_ctx + 1, np.uint32), np.zeros(8, np.uint32), np.zeros(8, np.uint8)

        def merge(old=None, t=None, s=None, out=Pt(no), tot=Pt(one)):
            return gd.lib.gd_wait_list_merge(e.h, old, None, n_ctx, Pt(wp), Pt(wo), 2, None, 0, None, t, s, 1, 8, out,
                                             Pt(nm), Pt(nf), tot)
        assert merge() == gd.GD_OK and int(one[0]) == 2
        assert merge(t=Pt(ta)) == gd.GD_EINVAL and merge(s=Pt(ta)) == gd.GD_EINVAL
        assert merge(old=C.byref(gd.gd_wait_list(off.ctypes.data, None, None))) == gd.GD_EINVAL
        assert merge(out=None) == gd.GD_EINVAL and merge(tot=None) == gd.GD_EINVAL
        # inside a stream capture the completion is refused before anything is launched
        dev = torch.device("cuda:0")
        d = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)
        d_ctx, d_fl, d_nr, d_off, d_wf = d(ctx), d(fl), d(nr), d(off), d(wf)
        outs = [torch.zeros(64, dtype=torch.uint8, device=dev) for _ in range(5)]
        mine = torch.zeros(4, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        e.set_stream(s.cuda_stream)
        e.set_kernel_timing(True)
        e.kernel_times_reset()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            mine.add_(1)                                     # the capture holds one node of the test's own
            with pytest.raises(gd.GrainDispatchError) as ei:
                e.turns_complete_device(d_ctx.data_ptr(), None, 3, n_ctx, d_fl.data_ptr(), d_nr.data_ptr(),
                                        e.wait_list_device(d_off.data_ptr(), None, d_wf.data_ptr()), 3,
                                        *[t.data_ptr() for t in outs])
            code = ei.value.code
        e.set_stream(None)
        assert code == gd.GD_ESTATE
        assert not any(k.startswith("k_") for k in e.kernel_times())
