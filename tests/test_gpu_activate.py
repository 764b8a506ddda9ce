"""GPU parity for the activation stage: gd_activate* and the receive -> activate -> turns chains through
the C ABI against tests/_activate_ref.py (the one-by-one rule over a dict).  Every output array and word is compared
bit for bit, dtype included, and so is the activation directory afterwards (gd_actdir_lookup of every id,
gd_actdir_count).  Device outputs are pre-filled with 0xA5 and carry 64 spare bytes that must stay 0xA5."""
import numpy as np
import pytest

import headers as H
import oracle as o
import receive as RV
import _activate_ref as A
import _frame_turns_ref as F
import _turns_ref as T

pytestmark = pytest.mark.gpu

TC = o.grain_type_code(o.PING_GRAIN_CLASS)
GD_EINVAL = -1
TURN_NAMES = ("turn", "num_running_out", "running_idx", "start_idx", "wait_perm", "wait_offsets")
HOT = [10, 30, 63, 64, 70, 200, 255, 256, 300, 4095, 4096, 4100, 4999]     # one wave, several waves, two workgroups


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    assert g.GD_EINVAL == GD_EINVAL
    return g


@pytest.fixture(scope="module")
def eng(gd):
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        yield e


def _same(got, want, name):
    assert got.dtype == want.dtype, name
    np.testing.assert_array_equal(got, want, err_msg=name)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _a5(count, width):
    import torch
    return torch.full((count * width + 64,), 0xA5, dtype=torch.uint8, device="cuda")


def _host(t, dt, count, written=None):
    """The first `count` elements; everything past the first `written` (default count) must still be 0xA5."""
    raw = t.cpu().numpy()
    w = (count if written is None else written) * np.dtype(dt).itemsize
    assert (raw[w:] == 0xA5).all(), "bytes past the output were written"
    return raw[:count * np.dtype(dt).itemsize].view(dt).copy()


def _load_dir(eng, entries):
    eng.actdir_clear()
    if entries:
        ids = np.array(list(entries), np.uint64)
        added = eng.actdir_add(ids, [v[0] for v in entries.values()], [v[1] for v in entries.values()])
        assert added.all()


def _check_dir(eng, want_entries, ids):
    """Every id the batch or the directory named: found / ctx / flags, and the live count."""
    ids = sorted(set(ids) | set(want_entries))
    if ids:
        c, f, found = eng.actdir_lookup(np.array(ids, np.uint64))
        for k, cc, ff, fo in zip(ids, c.tolist(), f.tolist(), found.tolist()):
            assert (fo, cc, ff) == ((1,) + want_entries[k] if k in want_entries else (0, A.NONE32, 0)), k
    assert eng.actdir_count() == len(want_entries)


def _run_host(gd, eng, b, lists=True):
    kw = dict(ctx_base=b.ctx_base, new_ctx=b.new_ctx, direction=b.direction, ttl=b.ttl, new_placement=b.new_placement,
              terminating=b.terminating, lists=lists)
    try:
        return eng.activate(b.ctx, b.recv_status, b.target_activation, b.n_ctx, b.cap_new, **kw), 0
    except gd.GrainDispatchError as ex:
        return ex.arrays, ex.code


def _run_device(gd, eng, b, alias=False):
    n = b.n
    opt = lambda a: None if a is None else _dev(a)
    d_ctx, d_rs, d_ta = _dev(b.ctx), _dev(b.recv_status), _dev(b.target_activation)
    d_dir, d_ttl, d_np, d_nc = opt(b.direction), opt(b.ttl), opt(b.new_placement), opt(b.new_ctx)
    d_kind = _a5(n, 1)
    d_co, d_so = (d_ctx, d_rs) if alias else (_a5(n, 4), _a5(n, 1))
    d_new, d_gone, d_w = _a5(n, 4), _a5(n, 4), [_a5(1, 4) for _ in range(3)]
    p = lambda t: None if t is None else t.data_ptr()
    rc = 0
    try:
        eng.activate_device(p(d_ctx), p(d_rs), p(d_ta), n, b.n_ctx, b.cap_new, p(d_kind), p(d_co), p(d_so), p(d_w[2]),
                            ctx_base=b.ctx_base, d_new_ctx=p(d_nc), d_direction=p(d_dir), d_ttl=p(d_ttl),
                            d_new_placement=p(d_np), terminating=b.terminating, d_new_idx=p(d_new), d_n_new=p(d_w[0]),
                            d_gone_idx=p(d_gone), d_n_gone=p(d_w[1]))
        eng.synchronize()
    except gd.GrainDispatchError as ex:                       # a proposal / context out of range: the next sync
        rc = ex.code
    n_new, n_gone, n_prop = (int(_host(t, np.uint32, 1)[0]) for t in d_w)
    if alias:
        co, so = d_co.cpu().numpy().view(np.uint32)[:n].copy(), d_so.cpu().numpy()[:n].copy()
    else:
        co, so = _host(d_co, np.uint32, n), _host(d_so, np.uint8, n)
    return dict(kind=_host(d_kind, np.uint8, n), ctx=co, status=so, n_proposed=n_prop,
                new_idx=_host(d_new, np.uint32, n_new), gone_idx=_host(d_gone, np.uint32, n_gone)), rc


def _check(gd, eng, b, form, alias=False, want=None):
    """Load the directory, run the batch, compare every output and the directory.  Returns the reference."""
    want = A.activate_loop(b) if want is None else want
    _load_dir(eng, b.entries)
    got, rc = _run_device(gd, eng, b, alias) if form == "device" else _run_host(gd, eng, b)
    for k in ("kind", "ctx", "status", "new_idx", "gone_idx"):
        _same(got[k], want[k], k)
    assert got["n_proposed"] == want["n_proposed"]
    refused = want["n_proposed"] > b.cap_new or want["err_range"]
    if form == "host" or want["err_range"]:
        assert rc == (GD_EINVAL if refused else 0)
    else:
        assert rc == 0                                      # device form: the caller compares n_proposed with cap_new
    _check_dir(eng, want["entries"], b.keys())
    return want


# ---- gd_activate* ---------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_batch_sizes(gd, eng, n, given, form):
    b, scripted, hot_id = A.scene(np.random.default_rng(1000 + n + given), n, given=given, hot=HOT if n == 5000 else None)
    want = _check(gd, eng, b, form)
    if n >= 257:
        A.assert_scene_cases(b, want, scripted, hot_id if n == 5000 else None)


@pytest.mark.parametrize("form", ["host", "device"])
def test_no_participating_message(gd, eng, form):
    """Outputs are copies, nothing is probed or created; a NULL new_placement, direction and ttl."""
    b, _, _ = A.scene(np.random.default_rng(2), 700, p_part=0.0)
    b.recv_status[:7] = 0
    b.new_placement = None
    want = _check(gd, eng, b, form)
    assert not want["kind"].any() and want["n_proposed"] == 0
    b, _, _ = A.scene(np.random.default_rng(3), 700)
    b.new_placement = b.direction = b.ttl = None
    want = _check(gd, eng, b, form)
    assert want["n_proposed"] == 0 and A.ACTV_NONEXISTENT in want["kind"] and A.ACTV_FOUND in want["kind"]


def test_in_place(gd, eng):
    b, _, _ = A.scene(np.random.default_rng(4), 4200, hot=HOT[:10])
    _check(gd, eng, b, "device", alias=True)


@pytest.mark.parametrize("form", ["host", "device"])
def test_lists_not_wanted_and_terminating(gd, eng, form):
    b, _, _ = A.scene(np.random.default_rng(5), 600, terminating=True)
    want = _check(gd, eng, b, form)
    assert want["n_proposed"] == 0 and A.ACTV_CREATED not in want["kind"] and A.ACTV_NONEXISTENT in want["kind"]
    if form == "host":
        b.terminating = False
        _load_dir(eng, b.entries)
        got, rc = _run_host(gd, eng, b, lists=False)
        want = A.activate_loop(b)
        assert rc == 0 and "new_idx" not in got
        _same(got["kind"], want["kind"], "kind")
        _check_dir(eng, want["entries"], b.keys())


@pytest.mark.parametrize("form", ["host", "device"])
def test_cap_new_exact_and_one_short(gd, eng, form):
    b, _, _ = A.scene(np.random.default_rng(6), 900)
    b.cap_new = A.activate_loop(b)["n_proposed"]
    b.new_ctx = b.new_ctx[:b.cap_new]
    want = _check(gd, eng, b, form)
    assert len(want["new_idx"]) and want["n_proposed"] == b.cap_new
    b.cap_new -= 1
    b.new_ctx = b.new_ctx[:-1]
    want = _check(gd, eng, b, form)                          # refused whole: the directory is unchanged
    assert want["entries"] == b.entries and want["n_proposed"] == b.cap_new + 1 and A.ACTV_HOST in want["kind"]
    assert len(want["new_idx"]) == 0 and len(want["gone_idx"]) == 0


@pytest.mark.parametrize("form", ["host", "device"])
def test_context_out_of_range(gd, eng, form):
    b, _, _ = A.scene(np.random.default_rng(7), 500)
    b.new_ctx[3] = b.n_ctx                                   # a proposal: refused whole, GD_EINVAL
    want = _check(gd, eng, b, form)
    assert want["err_range"] and want["entries"] == b.entries
    b, _, _ = A.scene(np.random.default_rng(8), 500)
    k = next(k for k, v in b.entries.items() if not v[1] & A.AD_SYSTEM_TARGET)
    b.entries[k] = (b.n_ctx + 3, 0)                          # a stored context: that message HOST, GD_EINVAL
    want = _check(gd, eng, b, form)
    assert want["err_range"] and A.ACTV_CREATED in want["kind"]
    if form == "host":                                       # ctx_base + cap_new past n_ctx: refused up front
        b, _, _ = A.scene(np.random.default_rng(9), 100, given=False)
        b.n_ctx = b.ctx_base + b.cap_new - 1
        _load_dir(eng, b.entries)
        assert _run_host(gd, eng, b)[1] == GD_EINVAL
        _check_dir(eng, b.entries, b.keys())


@pytest.mark.parametrize("form", ["host", "device"])
def test_tombstones_reuse_and_grow(gd, form):
    """A directory of 1,024 slots holding tombstones: 120 new ids reuse them (removed ids are created again, claims
    collide on the 8-aligned homes), then 700 more make the table grow."""
    rng = np.random.default_rng(10)
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        ids = A.act_keys(rng, 1500)
        tup = [tuple(int(x) for x in k) for k in ids]
        assert e.actdir_add(ids[:500], np.arange(500), np.zeros(500, np.uint8)).all()
        assert e.actdir_remove(ids[200:500]).all()
        entries = {tup[j]: (j, 0) for j in range(200)}
        n_ctx = 4000
        # ids 250..369 were removed: 200 live + 300 tombstones + cap_new 260 fits 1,024 slots at load 0.75, so the
        # claims reuse tombstones; ids 500.. never existed, and their batch makes the table grow
        for lo, hi, cap in ((250, 370, 260), (500, 1200, None)):
            m = hi - lo
            pick = np.concatenate([np.arange(lo, hi), rng.integers(lo, hi, m), rng.integers(0, 200, 50)])
            rng.shuffle(pick)
            n = len(pick)
            b = A.Batch(np.full(n, n_ctx, np.uint32), np.full(n, A.RECV_NULL_CONTEXT, np.uint8), ids[pick], n_ctx,
                        cap or n, entries, ctx_base=1000 + lo, new_placement=(rng.random(n) < 0.8).astype(np.uint8),
                        direction=rng.integers(0, 2, n).astype(np.uint8))
            want = A.activate_loop(b)
            got, rc = _run_device(gd, e, b) if form == "device" else _run_host(gd, e, b)
            assert rc == 0
            for k in ("kind", "ctx", "status", "new_idx", "gone_idx"):
                _same(got[k], want[k], k)
            assert got["n_proposed"] == want["n_proposed"] and len(want["new_idx"]) > 0.7 * m
            _check_dir(e, want["entries"], tup)
            entries = want["entries"]


# ---- the chains -----------------------------------------------------------------------------------

def _chain_state(rng, b):
    fl, nr = T.context_state(rng, b.n_ctx)
    fl[b.ctx_base:], nr[b.ctx_base:] = T.CTX_NOT_READY, 0    # the contexts offered to new activations
    return fl, nr, np.zeros(b.n_ctx, np.uint32)


def _chain_scene(rng, n):
    """Grain messages against a directory of Valid and not-Valid activations plus absent ids; receive's reference."""
    n_ex, n_ctx = 40, 40 + n + 8
    keys = A.act_keys(rng, n_ex + max(4, n // 5))
    entries = {tuple(int(x) for x in k): (j, (j % 3 != 0) * A.AD_VALID) for j, k in enumerate(keys[:n_ex])}
    ta = keys[rng.integers(0, len(keys), n)]
    tg = o.grain_keys(TC, rng.integers(0, 1000, size=n))
    dr = rng.choice(np.array([0, 0, 0, 1, 2, 0xFF], np.uint8), size=n)
    ttl = np.where(rng.random(n) < 0.8, T.TTL_NONE, rng.integers(-3, 20, n)).astype(np.int64)
    npl = rng.choice(np.array([0, 1, 1, 2], np.uint8), size=n)
    return tg, ta, dr, ttl, npl, entries, n_ex, n_ctx


def _receive_ref(tg, ta, dr, entries, n_ctx):
    ad = RV.ActivationDirectory()
    for k, (c, f) in entries.items():
        ad.add(k, c, f)
    st, ctx, _, _ = RV.receive_batch(tg, ta, dr, ad, n_ctx)
    return st, ctx


def _compare_chain(got, want, names):
    for k in names:
        _same(got[k], want[k], k)
    assert got["n_proposed"] == want["n_proposed"]


CHAIN_NAMES = ("kind", "ctx", "status", "new_idx", "gone_idx", "perm", "offsets") + TURN_NAMES


def _chain_device(gd, eng, n, n_ctx, fl, nr, rc, cap_new, ctx_base, call):
    """The outputs of a device-form chain: call(d_ctx, d_status, d_perm, d_offs, state, turn outs..., act io)."""
    d_fl, d_nr, d_rc = _dev(fl), _dev(nr), _dev(rc)
    state = eng.turn_state_device(d_fl.data_ptr(), d_nr.data_ptr(), d_rc.data_ptr())
    d = dict(ctx=_a5(n, 4), status=_a5(n, 1), perm=_a5(n, 4), offsets=_a5(n_ctx + 3, 4), turn=_a5(n, 1),
             num_running_out=_a5(n_ctx, 4), running_idx=_a5(n_ctx, 4), start_idx=_a5(n, 4), n_start=_a5(1, 4),
             wait_perm=_a5(n, 4), wait_offsets=_a5(n_ctx + 2, 4), kind=_a5(n, 1), new_idx=_a5(n, 4), n_new=_a5(1, 4),
             gone_idx=_a5(n, 4), n_gone=_a5(1, 4), n_proposed=_a5(1, 4))
    p = {k: v.data_ptr() for k, v in d.items()}
    act = eng.activate_io_device(cap_new, p["kind"], p["n_proposed"], ctx_base=ctx_base, d_new_idx=p["new_idx"],
                                 d_n_new=p["n_new"], d_gone_idx=p["gone_idx"], d_n_gone=p["n_gone"])
    call(p, state, act)
    eng.synchronize()
    w = {k: int(_host(d[k], np.uint32, 1)[0]) for k in ("n_start", "n_new", "n_gone", "n_proposed")}
    dt = dict(ctx=np.uint32, status=np.uint8, perm=np.uint32, turn=np.uint8, wait_perm=np.uint32, kind=np.uint8)
    out = {k: _host(d[k], t, n) for k, t in dt.items()}
    out.update(offsets=_host(d["offsets"], np.uint32, n_ctx + 3), wait_offsets=_host(d["wait_offsets"], np.uint32, n_ctx + 2),
               num_running_out=_host(d["num_running_out"], np.uint32, n_ctx),
               running_idx=_host(d["running_idx"], np.uint32, n_ctx), start_idx=_host(d["start_idx"], np.uint32, w["n_start"]),
               new_idx=_host(d["new_idx"], np.uint32, w["n_new"]), gone_idx=_host(d["gone_idx"], np.uint32, w["n_gone"]),
               n_proposed=w["n_proposed"])
    return out, act, (d_fl, d_nr, d_rc)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("n", [0, 65, 4500])
def test_chain_arrays(gd, eng, n, form):
    rng = np.random.default_rng(20 + n)
    tg, ta, dr, ttl, npl, entries, n_ex, n_ctx = _chain_scene(rng, n)
    st, ctx = _receive_ref(tg, ta, dr, entries, n_ctx)
    cap = int((npl == 1).sum())
    b = A.Batch(ctx, st, ta, n_ctx, cap, entries, ctx_base=n_ex, direction=dr, ttl=ttl, new_placement=npl)
    fl, nr, rc = _chain_state(rng, b)
    fwd, mf = rng.integers(0, 4, n).astype(np.uint8), rng.integers(0, 8, n).astype(np.uint8)
    want = A.chain_model(b, fl, nr, rc, fwd, mf)
    _load_dir(eng, entries)
    if form == "host":
        got = eng.receive_activate_turns(tg, ta, n_ctx, fl, nr, rc, cap, ctx_base=n_ex, new_placement=npl, direction=dr,
                                         ttl=ttl, forward_count=fwd, msg_flags=mf)
    else:
        d_in = [_dev(x) for x in (tg, ta, dr, ttl, fwd, mf, npl)]
        q = [t.data_ptr() for t in d_in]

        def call(p, state, act):
            act.new_placement = q[6]
            eng.receive_activate_turns_device(q[0], q[1], q[2], n, n_ctx, p["ctx"], p["status"], p["perm"], p["offsets"],
                                              q[3], q[4], q[5], None, state, p["turn"], p["num_running_out"],
                                              p["running_idx"], act, p["start_idx"], p["n_start"], p["wait_perm"],
                                              p["wait_offsets"])
        got, _, _ = _chain_device(gd, eng, n, n_ctx, fl, nr, rc, cap, n_ex, call)
    _compare_chain(got, want, CHAIN_NAMES)
    _check_dir(eng, want["entries"], b.keys())
    if n >= 4500:
        assert {T.TURN_WAIT, T.TURN_START, T.TURN_FORWARD, T.TURN_RESPONSE} <= set(want["turn"].tolist())
        assert len(want["new_idx"]) and (want["turn"][want["new_idx"]] != T.TURN_NONE).all()


def _np_frames(rng, n, entries_keys, absent_keys):
    """Addressed frames whose IsNewPlacement is true, false with the bit set, or absent; (buffer, offsets, truth)."""
    frames, truth = [], []
    pool = np.concatenate([entries_keys, absent_keys])
    for i in range(n):
        ta = pool[rng.integers(0, len(pool))]
        h = F.turn_frame(rng, o.grain_keys(TC, [int(rng.integers(0, 1000))])[0], ta, sa=ta,
                         direction=int(rng.choice([0, 0, 1, 2, 0xFF])))
        h.pop("is_new_placement", None)
        mode = i % 3
        if mode < 2:
            h["is_new_placement"] = mode == 0
        if i % 17 == 5:                                      # no complete address: left UNDECODED
            h.pop("target_silo")
        truth.append(1 if mode == 0 else 0)
        frames.append(H.encode_frame(h, bytes(int(rng.integers(0, 24)))))
    buf, off = F.join_frames(frames, lead=int(rng.integers(0, 4)))
    return buf, off, np.array(truth, np.uint8)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("n,age", [(0, 0), (300, 0), (1100, 6)])
def test_chain_frames(gd, eng, n, age, form):
    rng = np.random.default_rng(30 + n)
    n_ex, n_ctx = 20, 20 + n + 8
    keys = A.act_keys(rng, n_ex + max(4, n // 5))
    entries = {tuple(int(x) for x in k): (j, (j % 3 != 0) * A.AD_VALID) for j, k in enumerate(keys[:n_ex])}
    buf, off, truth = _np_frames(rng, n, keys[:n_ex], keys[n_ex:])
    f, t = H.decode_frames(buf, off), F.walk_frames(buf, off)
    st, ctx, _, _ = F.receive_frames_ref(f, list(entries), [v[0] for v in entries.values()],
                                         [v[1] for v in entries.values()], n_ctx)
    cap = int(truth.sum())
    b = A.Batch(ctx, st, f["target_activation"], n_ctx, cap, entries, ctx_base=n_ex, direction=f["direction"],
                ttl=F.aged_ttl(t["ttl"], age), new_placement=truth)
    fl, nr, rc = _chain_state(rng, b)
    mor = (rng.random(n) < 0.2).astype(np.uint8) * T.MSG_MAY_INTERLEAVE
    want = A.chain_model(b, fl, nr, rc, t["forward_count"], t["msg_flags"] | mor, f["sending_activation"])
    _load_dir(eng, entries)
    if form == "host":
        got = eng.receive_activate_turns_frames(buf, off, n_ctx, fl, nr, rc, cap, ctx_base=n_ex, ttl_age_ticks=age,
                                                msg_flags_or=mor)
    else:
        d_buf, d_off, d_mor = _dev(np.frombuffer(buf, np.uint8)), _dev(off), _dev(mor)

        def call(p, state, act):
            eng.receive_activate_turns_frames_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n, n_ctx, p["ctx"],
                                                     p["status"], p["perm"], p["offsets"], age, d_mor.data_ptr(), state,
                                                     p["turn"], p["num_running_out"], p["running_idx"], act,
                                                     p["start_idx"], p["n_start"], p["wait_perm"], p["wait_offsets"])
        got, _, _ = _chain_device(gd, eng, n, n_ctx, fl, nr, rc, cap, n_ex, call)
    _compare_chain(got, want, CHAIN_NAMES)
    _check_dir(eng, want["entries"], b.keys())
    if n >= 300:
        assert len(want["new_idx"]) and (truth[want["new_idx"]] == 1).all()
        assert (st == 6).any() or n < 1000                   # frames left UNDECODED never take part
        assert (want["kind"][st != A.RECV_NULL_CONTEXT] == A.ACTV_NONE).all()


def test_chain_refuses_hard_limits(gd, eng):
    rng = np.random.default_rng(40)
    tg, ta, dr, ttl, npl, entries, n_ex, n_ctx = _chain_scene(rng, 50)
    fl, nr, rc = np.zeros(n_ctx, np.uint8), np.zeros(n_ctx, np.uint32), np.zeros(n_ctx, np.uint32)
    _load_dir(eng, entries)
    for kw in (dict(hard_limit=1), dict(hard_limit_sw=1)):
        with pytest.raises(gd.GrainDispatchError) as ex:
            eng.receive_activate_turns(tg, ta, n_ctx, fl, nr, rc, 50, ctx_base=n_ex, new_placement=npl, **kw)
        assert ex.value.code == GD_EINVAL
        buf, off, _ = _np_frames(rng, 10, ta[:5], ta[5:10])
        with pytest.raises(gd.GrainDispatchError) as ex:
            eng.receive_activate_turns_frames(buf, off, n_ctx, fl, nr, rc, 10, ctx_base=n_ex, **kw)
        assert ex.value.code == GD_EINVAL
    _check_dir(eng, entries, [tuple(int(x) for x in k) for k in ta])
