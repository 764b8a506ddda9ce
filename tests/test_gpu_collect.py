"""GPU parity for the activation collector: gd_collect_* and their device forms through the C ABI
against the array form _collect_ref.Arrays (held to the literal ActivationCollector.cs transcription by
tests/test_collect_ref.py, which also asserts what the generators used here cover) -- every output and every state
array bit for bit, dtype included."""
import ctypes as C
import inspect

import numpy as np
import pytest

import _collect_ref as K
import _pump_ref as P
import _turns_ref as R

pytestmark = pytest.mark.gpu

TILE = 4096                      # gd_collect.h COL_TILE
Q = K.Q
DENSE = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 70001]
FILL = 0xAB


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


def _up(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _fill(n, dtype=np.uint8):
    import torch
    return torch.from_numpy(np.full(max(n, 1), FILL, np.uint8).repeat(np.dtype(dtype).itemsize).view(dtype).copy()).cuda()


def _eq(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, name
    np.testing.assert_array_equal(got, want, err_msg=name)


class Dev:
    """An Arrays state on the device, the handle's nextTicket set to its."""

    def __init__(self, eng, arr):
        self.eng, self.n_ctx = eng, arr.n_ctx
        self.t, self.bi, self.ka, self.age, self.fl = (_up(x) for x in (arr.ticket, arr.became_idle,
                                                                         arr.keep_alive_until, arr.age_limit, arr.flags))
        self.st = eng.collect_state(*(_p(x) or None for x in (self.t, self.bi, self.ka, self.age, self.fl)))
        eng.collect_configure(arr.quantum, arr.next)         # roundup(next) == next
        assert eng.collect_next_ticket() == arr.next

    def check(self, arr):
        """The whole state against (b) after the same call."""
        self.eng.synchronize()
        _eq("ticket", self.t.cpu().numpy(), arr.ticket)
        _eq("became_idle", self.bi.cpu().numpy(), arr.became_idle)
        _eq("flags", self.fl.cpu().numpy(), arr.flags)
        assert self.eng.collect_next_ticket() == arr.next


def _scan(eng, w, all_limit=None, verdict=True, wait=True, now=None):
    """scan_stale (or scan_all with all_limit) on the device against (b) on a copy of world w."""
    now = w.now if now is None else now
    arr, cf = w.arrays.copy(), w.ctx_flags.copy()
    wo = w.wait_offsets if wait else None
    if all_limit is None:
        want_list, want_v = arr.scan_stale(cf, w.num_running, now, wo)
    else:
        want_list, want_v = arr.scan_all(cf, w.num_running, now, all_limit, wo)
    d = Dev(eng, w.arrays)
    d_cf, d_nr, d_wo = _up(w.ctx_flags), _up(w.num_running), _up(wo)
    d_out, d_n, d_v = _fill(w.n_ctx, np.uint32), _fill(1, np.uint32), _fill(w.n_ctx) if verdict else None
    if all_limit is None:
        eng.collect_scan_stale_device(d.st, w.n_ctx, _p(d_cf), _p(d_nr), _p(d_wo), now, _p(d_out), _p(d_n), _p(d_v))
    else:
        eng.collect_scan_all_device(d.st, w.n_ctx, _p(d_cf), _p(d_nr), _p(d_wo), now, all_limit, _p(d_out), _p(d_n),
                                    _p(d_v))
    d.check(arr)
    n_out = int(d_n.cpu().numpy()[0])
    assert n_out == len(want_list)
    _eq("out_ctx", d_out.cpu().numpy()[:n_out], want_list)
    if verdict:
        _eq("verdict", d_v.cpu().numpy()[:w.n_ctx], want_v)
    _eq("ctx_flags", d_cf.cpu().numpy(), cf)
    return want_list, want_v


# ---- dense passes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_q", [0, 1, 2, 1000])
@pytest.mark.parametrize("n_ctx", DENSE)
def test_scan_stale_shapes(eng, n_ctx, n_q):
    """n_q = 2 and 1000: the list is by ticket, then by context (the bucketing's path)."""
    w = K.World(np.random.default_rng(n_ctx * 7 + n_q), n_ctx, n_q)
    _scan(eng, w)


@pytest.mark.parametrize("n_ctx", DENSE)
def test_idle_scan_all_count_shapes(eng, n_ctx):
    rng = np.random.default_rng(n_ctx)
    w = K.World(rng, n_ctx, 2)
    _scan(eng, w, all_limit=3 * Q)
    # idle
    ev = rng.integers(0, 8, n_ctx).astype(np.uint8)
    arr, d = w.arrays.copy(), Dev(eng, w.arrays)
    d_ok = _fill(n_ctx)
    eng.collect_idle_device(d.st, n_ctx, _p(_up(ev)), w.now, _p(d_ok))
    want = arr.idle(ev, w.now)
    d.check(arr)
    _eq("ok", d_ok.cpu().numpy()[:n_ctx], want)
    # count_recent: the state is untouched
    for shortest, rec in ((0, 0), (Q, 2 * Q)):
        d_cnt = _fill(1, np.uint64)
        eng.collect_count_recent_device(d.st, n_ctx, w.now, shortest, rec, _p(d_cnt))
        d.check(arr)
        assert int(d_cnt.cpu().numpy()[0]) == arr.count_recent(w.now, shortest, rec)


@pytest.mark.parametrize("due", ["all", "none", [0], [63], [64], [TILE - 1], [TILE], [2 * TILE - 1, 2 * TILE],
                                 [63, 64, TILE - 1, TILE, 3 * TILE + 16]])
def test_scan_due_variants(eng, due):
    """Everything due (and condemned), nothing due, and the only due contexts at a 64-lane edge and at a tile edge."""
    for n_q in (1, 2):
        w = K.World(np.random.default_rng(17), 3 * TILE + 17, n_q, due)
        lst, v = _scan(eng, w)
        if due == "all":
            assert len(lst) == w.n_ctx
        elif due == "none":
            assert len(lst) == 0 and not v.any()
        else:
            assert np.flatnonzero(v).tolist() == due
    w = K.World(np.random.default_rng(18), 3 * TILE + 17, 1, due)
    _scan(eng, w, all_limit=0)


# ---- list forms --------------------------------------------------------------------------------------

def _lists(eng, w, ctx, turn, now=None, outputs=True):
    """schedule, cancel and touch on the device, each from world w's state, against (b)."""
    now, n = w.now if now is None else now, len(ctx)
    d_ctx, d_turn, d_cf = _up(ctx), _up(turn), _up(w.ctx_flags)
    out = lambda: _fill(n) if outputs else None
    got = []
    for op in ("schedule", "cancel", "touch"):
        arr, d, d_o = w.arrays.copy(), Dev(eng, w.arrays), out()
        if op == "schedule":
            eng.collect_schedule_device(d.st, w.n_ctx, _p(d_ctx), n, now, _p(d_o))
            want = arr.schedule(ctx, now)
        elif op == "cancel":
            eng.collect_cancel_device(d.st, w.n_ctx, _p(d_ctx), n, _p(d_o))
            want = arr.cancel(ctx)
        else:
            eng.collect_touch_device(d.st, w.n_ctx, _p(d_cf), _p(d_ctx), _p(d_turn), n, now, _p(d_o))
            want = arr.touch(w.ctx_flags, ctx, now, turn)
        d.check(arr)
        if outputs:
            _eq(op, d_o.cpu().numpy()[:n], want)
        got.append(want)
    return got


@pytest.mark.parametrize("kind", ["uniform", "zipf"])
@pytest.mark.parametrize("n_ctx", [1, 7, 1025, 70001])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE, TILE + 1, 3 * TILE + 17, 200003])
def test_list_forms_shapes(eng, n, n_ctx, kind):
    """Uniform and Zipf targets at every shape, ctx >= n_ctx entries among them; random turn bytes and turn NULL."""
    rng = np.random.default_rng(n * 31 + n_ctx + (kind == "zipf"))
    w = K.World(rng, n_ctx, 2)
    ctx = K.targets(rng, n, n_ctx, kind)
    turn = rng.integers(0, 10, n).astype(np.uint8)
    _lists(eng, w, ctx, turn)
    _lists(eng, w, ctx, None)
    _lists(eng, w, ctx, turn, now=w.now - 50 * Q)            # a batch stamped long before: the :372 throw


@pytest.mark.parametrize("first", [0, 64, 63, TILE, TILE - 1])
def test_hot_context(eng, first):
    """One context takes all 3 * 4096 + 17 entries but those before `first`, which are out of range: its deciding
    first occurrence sits at index 0, at a 64 edge, at a tile edge."""
    n = 3 * TILE + 17
    rng = np.random.default_rng(first)
    w = K.World(rng, 9, 1)
    w.arrays.ticket[5], w.arrays.flags[5], w.arrays.age_limit[5], w.ctx_flags[5] = 0, 0, 2 * Q, K.VALID
    ctx = np.full(n, 5, np.uint32)
    ctx[:first] = 9
    sch, _, _ = _lists(eng, w, ctx, None)
    assert sch[first] == K.SCHEDULED and (sch[first + 1:] == K.THROWS_TICKETED).all()
    w.arrays.ticket[5] = w.arrays.next + 3 * Q               # scheduled: the first cancel wins; a touch moves it
    _, can, tch = _lists(eng, w, ctx, None)
    assert can[first] == 1 and can.sum() == 1 and (tch[first:] == K.TRUE).all()


def test_turn_null_is_every_message(eng):
    rng = np.random.default_rng(2)
    w = K.World(rng, 300, 1)
    ctx = K.targets(rng, 5000, 300)
    a = _lists(eng, w, ctx, None)[2]
    b = _lists(eng, w, ctx, np.full(5000, R.TURN_WAIT, np.uint8))[2]
    _eq("touch", a, b)
    none = _lists(eng, w, ctx, np.full(5000, R.TURN_EXPIRED, np.uint8))[2]
    assert (none == K.NO_PART).all()


def test_optional_arrays(eng):
    rng = np.random.default_rng(3)
    w = K.World(rng, 5000, 2)
    ctx = K.targets(rng, 3000, 5000)
    _lists(eng, w, ctx, None, outputs=False)                 # the state alone
    _scan(eng, w, verdict=False)
    _scan(eng, w, wait=False)
    _scan(eng, w, all_limit=Q, verdict=False, wait=False)
    w2 = K.World(np.random.default_rng(3), 5000, 2, keep_alive=False)
    lst, v = _scan(eng, w2)
    assert not (v & 0x7F == K.KEPT_ALIVE).any() and len(lst)
    arr, d = w.arrays.copy(), Dev(eng, w.arrays)             # idle without out_ok
    ev = rng.integers(0, 2, 5000).astype(np.uint8)
    eng.collect_idle_device(d.st, 5000, _p(_up(ev)), w.now, None)
    arr.idle(ev, w.now)
    d.check(arr)


# ---- errors ------------------------------------------------------------------------------------------

def test_errors(gd):
    w = K.World(np.random.default_rng(5), 100, 1)
    arr = w.arrays.copy()
    st = gd.GrainDispatch.collect_state(arr.ticket, arr.became_idle, arr.keep_alive_until, arr.age_limit, arr.flags)
    ctx, out, cf = np.zeros(4, np.uint32), np.zeros(100, np.uint8), w.ctx_flags.copy()
    lst, one, cnt = np.zeros(100, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    Pt = lambda a: C.c_void_p(a.ctypes.data)
    nxt = C.c_int64(0)
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        L, h, S = gd.lib, e.h, C.byref(st)
        calls = [lambda: L.gd_collect_next_ticket(h, C.byref(nxt)),
                 lambda: L.gd_collect_schedule(h, S, 100, Pt(ctx), 4, w.now, Pt(out)),
                 lambda: L.gd_collect_cancel(h, S, 100, Pt(ctx), 4, Pt(out)),
                 lambda: L.gd_collect_touch(h, S, 100, Pt(cf), Pt(ctx), None, 4, w.now, Pt(out)),
                 lambda: L.gd_collect_idle(h, S, 100, Pt(out), w.now, None),
                 lambda: L.gd_collect_scan_stale(h, S, 100, Pt(cf), Pt(w.num_running), None, w.now, Pt(lst), Pt(one), None),
                 lambda: L.gd_collect_scan_all(h, S, 100, Pt(cf), Pt(w.num_running), None, w.now, Q, Pt(lst), Pt(one), None),
                 lambda: L.gd_collect_count_recent(h, S, 100, w.now, 0, 0, Pt(cnt))]
        assert [c() for c in calls] == [gd.GD_ESTATE] * len(calls)         # before configure
        assert L.gd_collect_configure(h, 0, w.now) == gd.GD_EINVAL
        assert L.gd_collect_configure(h, -5, w.now) == gd.GD_EINVAL
        assert L.gd_collect_configure(None, Q, w.now) == gd.GD_EINVAL
        assert calls[0]() == gd.GD_ESTATE
        e.collect_configure(Q, arr.next)
        assert L.gd_collect_schedule(h, None, 100, Pt(ctx), 4, w.now, Pt(out)) == gd.GD_EINVAL
        assert L.gd_collect_schedule(h, S, 100, None, 4, w.now, Pt(out)) == gd.GD_EINVAL
        assert L.gd_collect_scan_stale(h, S, 100, Pt(cf), Pt(w.num_running), None, w.now, Pt(lst), None, None) == gd.GD_EINVAL
        # more than 2^28 quanta: GD_EINVAL, state and nextTicket unchanged
        far = arr.next + Q * ((1 << 28) + 1)
        assert L.gd_collect_scan_stale(h, S, 100, Pt(cf), Pt(w.num_running), None, far, Pt(lst), Pt(one), None) == gd.GD_EINVAL
        assert e.collect_next_ticket() == arr.next
        _eq("ticket", arr.ticket, w.arrays.ticket), _eq("flags", arr.flags, w.arrays.flags), _eq("cf", cf, w.ctx_flags)
        assert [c() for c in calls] == [gd.GD_OK] * len(calls)
        assert L.gd_collect_schedule(h, S, 0, Pt(ctx), 4, w.now, Pt(out)) == gd.GD_OK and (out[:4] == K.OUT_OF_RANGE).all()


def test_too_many_quanta_device_form_changes_nothing(eng, gd):
    """gd_collect_scan_stale_device over more than 2^28 quanta: GD_EINVAL, the state arrays, ctx_flags, the outputs
    and nextTicket as they were."""
    w = K.World(np.random.default_rng(6), TILE + 1, 2)
    d = Dev(eng, w.arrays)
    d_cf, d_nr, d_wo = _up(w.ctx_flags), _up(w.num_running), _up(w.wait_offsets)
    d_out, d_n, d_v = _fill(w.n_ctx, np.uint32), _fill(1, np.uint32), _fill(w.n_ctx)
    far = w.arrays.next + Q * ((1 << 28) + 1)
    with pytest.raises(gd.GrainDispatchError) as ei:
        eng.collect_scan_stale_device(d.st, w.n_ctx, _p(d_cf), _p(d_nr), _p(d_wo), far, _p(d_out), _p(d_n), _p(d_v))
    assert ei.value.code == gd.GD_EINVAL
    d.check(w.arrays)
    _eq("ctx_flags", d_cf.cpu().numpy(), w.ctx_flags)
    assert (d_out.cpu().numpy().view(np.uint8) == FILL).all() and (d_n.cpu().numpy().view(np.uint8) == FILL).all()
    assert (d_v.cpu().numpy() == FILL).all()


# ---- host forms against the device forms -------------------------------------------------------------

@pytest.mark.parametrize("n", [65, TILE + 1])
def test_host_forms(eng, gd, n):
    rng = np.random.default_rng(n)
    w = K.World(rng, n, 2)
    ctx = K.targets(rng, n, n)
    turn = rng.integers(0, 10, n).astype(np.uint8)
    ev = rng.integers(0, 8, n).astype(np.uint8)

    def host(op):
        arr, cf = w.arrays.copy(), w.ctx_flags.copy()
        st = eng.collect_state(arr.ticket, arr.became_idle, arr.keep_alive_until, arr.age_limit, arr.flags)
        eng.collect_configure(Q, arr.next)
        ref = w.arrays.copy()
        if op == "schedule":
            _eq(op, eng.collect_schedule(st, n, ctx, w.now), ref.schedule(ctx, w.now))
        elif op == "cancel":
            _eq(op, eng.collect_cancel(st, n, ctx), ref.cancel(ctx))
        elif op == "touch":
            _eq(op, eng.collect_touch(st, n, cf, ctx, w.now, turn), ref.touch(cf, ctx, w.now, turn))
        elif op == "idle":
            _eq(op, eng.collect_idle(st, n, ev, w.now), ref.idle(ev, w.now))
        elif op == "count":
            assert eng.collect_count_recent(st, n, w.now, Q, 2 * Q) == ref.count_recent(w.now, Q, 2 * Q)
        else:
            rcf = w.ctx_flags.copy()
            if op == "stale":
                got = eng.collect_scan_stale(st, n, cf, w.num_running, w.now, w.wait_offsets)
                want = ref.scan_stale(rcf, w.num_running, w.now, w.wait_offsets)
            else:
                got = eng.collect_scan_all(st, n, cf, w.num_running, w.now, 3 * Q, w.wait_offsets)
                want = ref.scan_all(rcf, w.num_running, w.now, 3 * Q, w.wait_offsets)
            _eq("list", got[0], want[0]), _eq("verdict", got[1], want[1]), _eq("ctx_flags", cf, rcf)
            assert eng.collect_next_ticket() == ref.next
        for name in ("ticket", "became_idle", "flags"):
            _eq(name, getattr(arr, name), getattr(ref, name))

    for op in ("schedule", "cancel", "touch", "idle", "count", "stale", "all"):
        host(op)
    # the device forms give (b) too (the tests above); here at the same shapes
    _scan(eng, w)
    _lists(eng, w, ctx, turn)


# ---- the turn cycle with the collector, on the device ------------------------------------------------

class _Hooked:
    """The engine with a collector call enqueued after gd_turns_device and after gd_turns_complete_device."""

    def __init__(self, eng, after_turns, after_complete):
        self._eng, self._after_turns, self._after_complete = eng, after_turns, after_complete

    def __getattr__(self, k):
        return getattr(self._eng, k)

    def turns_device(self, *a, **kw):
        self._eng.turns_device(*a, **kw)
        b = inspect.signature(self._eng.turns_device).bind(*a, **kw).arguments
        self._after_turns(b["d_ctx"], b["n"], b["state"].ctx_flags, b["d_turn"])   # the flags the turns read

    def turns_complete_device(self, *a, **kw):
        self._eng.turns_complete_device(*a, **kw)
        self._after_complete(inspect.signature(self._eng.turns_complete_device).bind(*a, **kw).arguments["d_event"])


def test_cycle_with_the_collector_on_the_device(eng, gd):
    """turns_device -> collect_touch_device -> wait_list_merge_device -> turns_complete_device ->
    collect_idle_device, four rounds with the clock advancing, then collect_scan_stale_device; nothing is read back
    between the calls.  The reference: test_pump_ref.Lifecycle beside the Activation objects, its turn bytes and
    events fed message by message to the literal Collector (a)."""
    import torch
    import test_gpu_pump as TP
    from test_pump_ref import Lifecycle
    n_ctx, sizes = 2000, (4000, 700, 6000, 3000)
    rec ={"turns": [], "events": []}

    def turns(b):
        out = R.turns_loop(b)
        rec["turns"].append((np.array(b.ctx_flags, np.uint8).copy(), out[0].copy()))
        return out

    def pump(pb):
        out = P.pump_loop(pb)
        rec["events"].append(out[4].copy())
        return out

    life = Lifecycle(41, n_ctx, turns=turns, pump=pump)
    flags0, nr0 = life.flags.copy(), life.nr.copy()
    for n in sizes:
        life.step(n)
    # (a): every context scheduled at t0, then the rounds message by message
    rng = np.random.default_rng(77)
    t0 = K.T0 + 999
    nows = [t0 + Q // 2, t0 + Q + 5, t0 + Q + 5, t0 + 3 * Q]
    t_scan = t0 + 12 * Q                                     # every ticket is due; most activations are still running
    age = K.AGES[rng.choice(len(K.AGES), n_ctx, p=[0.05, 0.0, 0.25, 0.3, 0.4, 0.0])]
    exempt = rng.random(n_ctx) < 0.05
    acts = [K.Act(c, int(age[c]), bool(exempt[c])) for c in range(n_ctx)]
    lit = K.Collector(Q, t0)
    for a in acts:
        K.literal_call(lit.schedule, a, t0)
    arr0 = K.Arrays(Q, t0, [a.ticket for a in acts], np.zeros(n_ctx), None, age, np.where(exempt, K.EXEMPT, 0))
    for (cf, turn), ev, s, now in zip(rec["turns"], rec["events"], life.log, nows):
        for c, t in zip(s["ctx"].tolist(), turn.tolist()):
            if t in K.TURN_TAKES_PART and cf[c] & K.STATE_MASK == K.VALID:
                K.literal_call(lit.try_reschedule, acts[c], now)
        for c in np.flatnonzero(ev & K.IDLE).tolist():
            acts[c].became_idle = now
            if not acts[c].exempt:
                K.literal_call(lit.try_reschedule, acts[c], now)
    for c, a in enumerate(acts):
        a.state, a.other_bits = int(life.flags[c] & K.STATE_MASK), int(life.flags[c] & ~np.uint8(K.STATE_MASK))
        a.num_running, a.n_waiting = P._i32(life.nr[c]), int(life.off[c + 1] - life.off[c])
    want_list, want_v = lit.scan_stale(t_scan)
    assert 0 < len(want_list) < n_ctx and lit.members()
    # the device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    z = lambda count, width: torch.zeros(max(count, 1) * width, dtype=torch.uint8, device="cuda")
    ins = [{k: dev(v) for k, v in s.items() if k in ("ctx", "msg_flags", "ta", "sa", "ids", "done_ctx", "done_flags")}
           for s in life.log]
    flips = [torch.from_numpy(s["flips"]).cuda() for s in life.log]
    cap = sum(sizes)
    d = Dev(eng, arr0)
    clock = iter(nows)
    now = [None]

    def after_turns(d_ctx, n, d_cf, d_turn):
        now[0] = next(clock)
        eng.collect_touch_device(d.st, n_ctx, d_cf, d_ctx, d_turn, n, now[0], None)

    hooked = _Hooked(eng, after_turns, lambda d_ev: eng.collect_idle_device(d.st, n_ctx, d_ev, now[0], None))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            keep, d_flags, d_nr = TP._cycle_steps(hooked, torch, life, ins, flips, n_ctx, cap, dev(flags0), dev(nr0), z)
            # the lists that are left: the last merge's, less what the last pump dequeued
            k = keep[-1]
            old = eng.wait_list_device(k[2].data_ptr(), k[3].data_ptr(), k[4].data_ptr())
            f_off, f_msg, f_fl, f_tot = z(n_ctx + 1, 4), z(cap, 4), z(cap, 1), z(1, 4)
            eng.wait_list_merge_device(old, k[8].data_ptr(), n_ctx, None, z(n_ctx + 2, 4).data_ptr(), 0, None, 0, None,
                                       None, None, False, cap, f_off.data_ptr(), f_msg.data_ptr(), f_fl.data_ptr(),
                                       f_tot.data_ptr())
            d_out, d_n, d_v = z(n_ctx, 4), z(1, 4), z(n_ctx, 1)
            eng.collect_scan_stale_device(d.st, n_ctx, d_flags.data_ptr(), d_nr.data_ptr(), f_off.data_ptr(), t_scan,
                                          d_out.data_ptr(), d_n.data_ptr(), d_v.data_ptr())
        eng.synchronize()
    finally:
        eng.set_stream(None)
    host = lambda t, dt: t.cpu().numpy().view(dt)
    n_out = int(host(d_n, np.uint32)[0])
    assert host(d_out, np.uint32)[:n_out].tolist() == want_list
    assert host(d_v, np.uint8)[:n_ctx].tolist() == [want_v.get(c, 0) for c in range(n_ctx)]
    assert d.t.cpu().numpy().tolist() == [a.ticket for a in acts]
    assert d.bi.cpu().numpy().tolist() == [a.became_idle for a in acts]
    assert [bool(f & K.CANCELLED) for f in d.fl.cpu().numpy()] == [a.cancelled for a in acts]
    assert host(d_flags, np.uint8)[:n_ctx].tolist() == [a.ctx_flag_byte() for a in acts]
    assert eng.collect_next_ticket() == lit.next_ticket
