"""GPU parity for the turn admission of a received batch: gd_turns / gd_turns_device /
gd_receive_turns_device through the C ABI against the literal restatement of Dispatcher.ReceiveRequest
(_turns_ref.turns_loop), every output bit for bit, dtype included."""
import ctypes as C

import numpy as np
import pytest

import _turns_ref as R
import oracle as o

pytestmark = pytest.mark.gpu

TILE = 4096                      # k_turn_classify's / k_turn_decide's messages per workgroup (gd_turns.h TN_TILE)
NAMES = ("turn", "num_running_out", "running_idx", "start_idx", "wait_perm", "wait_offsets")


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


def _check(got, want, names=NAMES):
    for name, a, b in zip(names, got, want):
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a, b, err_msg=name)


def _call(e, b, lists=True):
    return e.turns(b.ctx, b.n_ctx, b.ctx_flags, b.num_running, b.request_count, b.recv_status, b.direction, b.ttl,
                   b.forward_count, b.msg_flags, b.target_activation, b.sending_activation, b.hard_limit,
                   b.hard_limit_sw, b.max_forward_count, b.chain, lists=lists)


def _run(e, b):
    want = R.turns_loop(b)
    _check(_call(e, b), want)
    return want


SHAPES = [(0, 1), (0, 1025), (1, 1), (1, 7), (63, 7), (63, 1024), (64, 1), (64, 1025), (65, 7), (65, 70001),
          (255, 1), (255, 1024), (256, 7), (256, 1025), (257, 1024), (257, 70001), (TILE - 1, 7), (TILE - 1, 1025),
          (TILE, 1), (TILE, 1024), (TILE + 1, 7), (TILE + 1, 70001), (3 * TILE + 17, 1), (3 * TILE + 17, 1024),
          (3 * TILE + 17, 1025), (200003, 7), (200003, 70001)]


@pytest.mark.parametrize("n,n_ctx", SHAPES)
def test_shapes_mixed_batch(eng, n, n_ctx):
    """Every n with two or more n_ctx; limits on for odd n + n_ctx, off otherwise."""
    rng = np.random.default_rng(n * 31 + n_ctx)
    _run(eng, R.mixed_batch(rng, n, n_ctx, limits=(n + n_ctx) % 2 == 1))


def _hot(rng, n, flags, num_running, request_count, limit, msg_flags=None):
    return R.Batch(np.zeros(n, np.uint32), 1, [flags], [num_running], [request_count], msg_flags=msg_flags,
                   hard_limit=limit, hard_limit_sw=limit)


@pytest.mark.parametrize("limits", [False, True])
@pytest.mark.parametrize("kind", ["hot_idle", "hot_busy", "hot_reentrant", "own", "uniform", "zipf", "none",
                                  "invalid", "mix"])
def test_distributions(eng, kind, limits):
    n = 3 * TILE + 17
    rng = np.random.default_rng(11)
    ro = (rng.integers(0, 2, n) * R.MSG_READ_ONLY).astype(np.uint8)
    # the hot context's reject / wait boundary inside the batch: past a wave edge (rank 64 * 70 + 3) and, with the
    # other count, past a workgroup edge (rank TILE + 5)
    limit = 100 if limits else 0
    if kind == "hot_idle":
        b = _hot(rng, n, R.CTX_VALID, 0, 100 + 64 * 70 + 3, limit, ro)
    elif kind == "hot_busy":
        b = _hot(rng, n, R.CTX_VALID | R.CTX_HAS_RUNNING, 1, 100 + TILE + 5, limit, ro)
    elif kind == "hot_reentrant":
        b = _hot(rng, n, R.CTX_VALID | R.CTX_HAS_RUNNING | R.CTX_REENTRANT, 3, 100 + TILE + 5, limit)
    elif kind == "own":
        fl, nr = R.context_state(rng, n)
        b = R.Batch(rng.permutation(n).astype(np.uint32), n, fl, nr, rng.integers(0, 4, n), msg_flags=ro,
                    hard_limit=1 if limits else 0, hard_limit_sw=2 if limits else 0)
    elif kind in ("uniform", "zipf"):
        b = R.mixed_batch(rng, n, 1024, kind, limits=limits)
        b.recv_status = b.direction = b.ttl = b.forward_count = None
    elif kind == "none":
        b = R.mixed_batch(rng, n, 7, limits=limits)
        b.recv_status = np.full(n, 2, np.uint8)
    elif kind == "invalid":
        b = R.mixed_batch(rng, n, 1025, limits=limits)
        b.ctx_flags = ((b.ctx_flags & ~np.uint8(R.CTX_STATE_MASK)) | np.uint8(R.CTX_INVALID)).astype(np.uint8)
    else:
        b = R.mixed_batch(rng, n, 300, limits=limits)
    want = _run(eng, b)
    turn = want[0]
    if kind == "mix":
        assert set(np.unique(turn).tolist()) == set(range(R.N_TURNS)) - (set() if limits else {R.TURN_REJECT_OVERLOADED})
        assert set(np.unique(b.ctx_flags & R.CTX_STATE_MASK).tolist()) == {0, 1, 2}
    if kind == "none":
        assert not turn.any()
    if kind in ("hot_idle", "hot_busy") and limits:
        w = np.flatnonzero(turn == R.TURN_WAIT)
        r = np.flatnonzero(turn == R.TURN_REJECT_OVERLOADED)
        assert len(w) and len(r) and r.max() < w.min()
    if kind == "hot_reentrant":
        assert (turn == R.TURN_START).all() and want[1][0] == 3 + n


def test_hot_boundary_on_the_edges(eng):
    """The first waiting message exactly at a wave edge and exactly at a workgroup edge."""
    n = 2 * TILE + 100
    for edge in (64 * 5, TILE):
        b = _hot(None, n, R.CTX_VALID | R.CTX_HAS_RUNNING, 1, 10 + edge, 10)
        turn = _run(eng, b)[0]
        assert int(np.flatnonzero(turn == R.TURN_WAIT).min()) == edge
        assert (turn[:edge] == R.TURN_REJECT_OVERLOADED).all()


def test_optional_arrays(eng, gd):
    rng = np.random.default_rng(3)
    n, n_ctx = 5000, 64
    fl, nr = R.context_state(rng, n_ctx)
    b = R.Batch(rng.integers(0, n_ctx, n), n_ctx, fl, nr, rng.integers(0, 200, n_ctx), hard_limit=90, hard_limit_sw=60)
    got = _call(eng, b)
    _check(got, R.turns_loop(b))
    _check(_call(eng, b.explicit()), got)                    # all NULL = the explicit defaults
    _check(_call(eng, b, lists=False), got[:3], NAMES[:3])   # lists NULL: the same turn[] and context outputs
    ta = rng.integers(0, 1 << 60, (n, 3), dtype=np.uint64)
    for t, s in ((ta, None), (None, ta)):                    # one key array of the pair
        with pytest.raises(gd.GrainDispatchError):
            eng.turns(b.ctx, n_ctx, fl, nr, b.request_count, target_activation=t, sending_activation=s, chain=True)
    # one array of a list pair, through the C ABI
    c = np.zeros(4, np.uint32)
    st = gd.gd_turn_state(fl.ctypes.data, nr.ctypes.data, None, 0, 0, 2, 0)
    turn, nro, run, lst = np.zeros(4, np.uint8), np.zeros(n_ctx, np.uint32), np.zeros(n_ctx, np.uint32), np.zeros(4, np.uint32)
    P = lambda a: C.c_void_p(a.ctypes.data)
    for tail in ((P(lst), None, None, None), (None, None, P(lst), None)):
        rc = gd.lib.gd_turns(eng.h, P(c), None, None, None, None, None, None, None, 4, n_ctx, C.byref(st), P(turn),
                             P(nro), P(run), *tail)
        assert rc == gd.GD_EINVAL
    # a limit without request_count
    st.hard_limit = 5
    assert gd.lib.gd_turns(eng.h, P(c), None, None, None, None, None, None, None, 4, n_ctx, C.byref(st), P(turn),
                           P(nro), P(run), None, None, None, None) == gd.GD_EINVAL


def test_deterministic(eng):
    b = R.mixed_batch(np.random.default_rng(9), 3 * TILE + 17, 40, "zipf")
    _check(_call(eng, b), _call(eng, b))


def test_large_zipf_through_the_msd_bucketing(eng):
    """2^20 + 5 messages: the rank and the wait lists come from the two-level bucketing; closed form as the
    reference (proved equal to the loop on the CPU)."""
    rng = np.random.default_rng(4)
    b = R.mixed_batch(rng, (1 << 20) + 5, 50000, "zipf")
    _check(_call(eng, b), R.turns_np(b))


def _recv_world(rng, n_act, n):
    aid = np.zeros((n_act, 3), np.uint64)
    aid[:, 0] = rng.integers(1, 1 << 62, size=n_act, dtype=np.int64).astype(np.uint64)
    aid[:, 1] = rng.integers(0, 1 << 62, size=n_act, dtype=np.int64).astype(np.uint64)
    st_key = np.array([[0, 7, o.type_code_data(o.CAT_SYSTEM_TARGET, 12)]], np.uint64)
    keys = np.concatenate([aid, st_key])
    ctxs = rng.permutation(n_act + 1).astype(np.uint32)
    adf = np.concatenate([np.where(rng.random(n_act) < 0.9, 1, 0) | np.where(rng.random(n_act) < 0.3, 4, 0), [3]])
    which = rng.integers(0, n_act + 1 + n_act // 8, size=n)
    ta = np.zeros((n, 3), np.uint64)
    known = which < n_act + 1
    ta[known] = keys[which[known]]
    ta[~known, 0] = rng.integers(1, 1 << 62, size=int((~known).sum()), dtype=np.int64).astype(np.uint64)
    tg = o.grain_keys(o.grain_type_code(o.PING_GRAIN_CLASS), rng.integers(0, 1000, size=n))
    tg[which == n_act, 2] = np.uint64(o.type_code_data(o.CAT_SYSTEM_TARGET, 12))
    return keys, ctxs, adf.astype(np.uint8), tg, ta


def test_fused_receive_turns(gd):
    """gd_receive_turns_device == gd_receive then gd_turns, with system-target, null-context and
    overload-rejected messages in the batch (all GD_TURN_NONE)."""
    import torch
    rng = np.random.default_rng(21)
    n_act, n = 400, 3 * TILE + 17
    keys, ctxs, adf, tg, ta = _recv_world(rng, n_act, n)
    n_ctx = n_act + 1
    direction = rng.choice(np.array([0, 1, 2, 0xFF], np.uint8), size=n, p=[0.6, 0.2, 0.1, 0.1])
    m = R.mixed_batch(rng, n, n_ctx)
    sa = m.sending_activation.copy()
    eq = rng.random(n) < 0.2
    sa[eq] = ta[eq]
    rc0 = rng.integers(0, 30, n_ctx).astype(np.uint32)
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        assert e.actdir_add(keys, ctxs, adf).all()
        ctx, st, perm, off = e.receive(tg, ta, direction, n_ctx, rc0, 45, 35)
        assert {gd.RECV_ACTIVATION, gd.RECV_SYSTEM_TARGET, gd.RECV_NULL_CONTEXT, gd.RECV_REJECT_OVERLOADED} <= \
            set(np.unique(st).tolist())
        rc = R.request_count_after_receive(rc0, off, n_ctx)
        b = R.Batch(ctx, n_ctx, m.ctx_flags, m.num_running, rc, st, direction, m.ttl, m.forward_count, m.msg_flags, ta, sa,
                    40, 30, 2, True)
        want = _call(e, b)
        _check(want, R.turns_loop(b))
        assert not want[0][st != gd.RECV_ACTIVATION].any()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        d_tg, d_ta, d_sa, d_dir = dev(tg), dev(ta), dev(sa), dev(direction)
        d_ttl, d_fw, d_mf = dev(m.ttl), dev(m.forward_count), dev(m.msg_flags)
        d_fl, d_nr, d_rc0, d_rc = dev(m.ctx_flags), dev(m.num_running), dev(rc0), dev(rc)
        z = lambda count, width: torch.zeros(max(count, 1) * width, dtype=torch.uint8, device="cuda")
        d_ctx, d_st, d_perm, d_off = z(n, 4), z(n, 1), z(n, 4), z(n_ctx + 3, 4)
        d_turn, d_nro, d_run = z(n, 1), z(n_ctx, 4), z(n_ctx, 4)
        d_start, d_ns, d_wp, d_wo = z(n, 4), z(1, 4), z(n, 4), z(n_ctx + 2, 4)
        state = e.turn_state_device(d_fl.data_ptr(), d_nr.data_ptr(), d_rc.data_ptr(), 40, 30, 2, True)
        e.receive_turns_device(d_tg.data_ptr(), d_ta.data_ptr(), d_dir.data_ptr(), n, n_ctx, d_ctx.data_ptr(),
                               d_st.data_ptr(), d_perm.data_ptr(), d_off.data_ptr(), d_ttl.data_ptr(), d_fw.data_ptr(),
                               d_mf.data_ptr(), d_sa.data_ptr(), state, d_turn.data_ptr(), d_nro.data_ptr(),
                               d_run.data_ptr(), d_start.data_ptr(), d_ns.data_ptr(), d_wp.data_ptr(), d_wo.data_ptr(),
                               d_rc0.data_ptr(), 45, 35)
        e.synchronize()
        host = lambda t, dt: t.cpu().numpy().view(dt)
        np.testing.assert_array_equal(host(d_ctx, np.uint32), ctx)
        np.testing.assert_array_equal(host(d_st, np.uint8), st)
        np.testing.assert_array_equal(host(d_perm, np.uint32), perm)
        np.testing.assert_array_equal(host(d_off, np.uint32), off)
        ns = int(host(d_ns, np.uint32)[0])
        got = (host(d_turn, np.uint8), host(d_nro, np.uint32), host(d_run, np.uint32), host(d_start, np.uint32)[:ns],
               host(d_wp, np.uint32), host(d_wo, np.uint32))
        _check(got, want)
        # the device-pointer turn stage alone, on the fused call's own ctx / status
        d_turn2, d_nro2, d_run2 = z(n, 1), z(n_ctx, 4), z(n_ctx, 4)
        e.turns_device(d_ctx.data_ptr(), d_st.data_ptr(), d_dir.data_ptr(), d_ttl.data_ptr(), d_fw.data_ptr(),
                       d_mf.data_ptr(), d_ta.data_ptr(), d_sa.data_ptr(), n, n_ctx, state, d_turn2.data_ptr(),
                       d_nro2.data_ptr(), d_run2.data_ptr())
        e.synchronize()
        _check((host(d_turn2, np.uint8), host(d_nro2, np.uint32), host(d_run2, np.uint32)), want[:3], NAMES[:3])
