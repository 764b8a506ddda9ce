"""GPU parity for GD_OPT_WALK_INVALIDATION: with the option on, the decoder and every entry point it
feeds, the encoder and the responder step over a frame's CacheInvalidationHeader; with it off nothing changes.
Everything is compared bit for bit with tests/_cih_ref.py (whose two forms tests/test_cih_ref.py proves equal).
Device outputs are pre-filled with 0xA5 and carry 64 spare bytes that must stay 0xA5."""
import struct

import numpy as np
import pytest

import headers as H
import keyext as kx
import oracle as o
import _activate_ref as A
import _cih_ref as X
import _encode_ref as E
import _forward_ref as F
import _frame_turns_ref as FT
import _respond_ref as R
import _sendq_ref as SQ
import _turns_ref as T

pytestmark = pytest.mark.gpu

TC = o.grain_type_code(o.PING_GRAIN_CLASS)
SIZES = [1, 63, 64, 65, 257]                      # the wave and workgroup edges
CFG = E.make_config(np.random.default_rng(9))


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


def _engine(gd, walk, **kw):
    e = gd.GrainDispatch(device=0, table_capacity=1 << 12, **kw)
    if walk:
        e.set_option(gd.OPT_WALK_INVALIDATION, 1)
    e.encode_configure(F.SILO_TUPLES, F.TYPE_NAMES)
    e.activation_ids_set(np.arange(len(CFG.act_ids)), CFG.act_ids)
    e.respond_configure(R.INFOS)
    return e


@pytest.fixture(scope="module")
def eng(gd):
    e = _engine(gd, True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batches():
    """The reference is computed once a batch: (buf, offs, decoder rows as arrays)."""
    rng = np.random.default_rng(1805)
    out = {}
    for n in SIZES:
        buf, offs = X.mixed_batch(n, rng)
        out[n] = (buf, offs, X.decode_batch(buf, offs))
    return out


# ---- device plumbing
def _up(a, dt=None):
    import torch
    a = np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _a5(nbytes):
    import torch
    return torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")


def _down(t, dt, shape):
    raw = t.cpu().numpy()
    nb = int(np.prod(shape)) * np.dtype(dt).itemsize
    assert (raw[nb:] == 0xA5).all(), "bytes past the output were written"
    return raw[:nb].view(dt).reshape(shape).copy()


def _decode_dev(gd, e, d_buf, blen, d_off, n, turn):
    """gd_decode_frames_device / gd_decode_frames_turn_device: every field as a numpy array."""
    sz = lambda dt, sh: n * np.dtype(dt).itemsize * int(np.prod(sh, dtype=np.int64))
    d = {k: _a5(sz(dt, sh)) for k, (dt, sh) in gd.FRAME_FIELDS.items()}
    dtf = {k: _a5(sz(dt, ())) for k, dt in gd.FRAME_TURN_FIELDS.items()} if turn else {}
    if turn:
        e.decode_frames_turn_device(d_buf.data_ptr(), blen, d_off.data_ptr(), n, {k: v.data_ptr() for k, v in d.items()},
                                    {k: v.data_ptr() for k, v in dtf.items()})
    else:
        e.decode_frames_device(d_buf.data_ptr(), blen, d_off.data_ptr(), n, {k: v.data_ptr() for k, v in d.items()})
    e.synchronize()
    out = {k: _down(d[k], dt, (n,) + sh) for k, (dt, sh) in gd.FRAME_FIELDS.items()}
    out.update({k: _down(dtf[k], dt, (n,)) for k, dt in gd.FRAME_TURN_FIELDS.items() if turn})
    return out


def _same_fields(got, want, names):
    for k in names:
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _writer_dev(call, cap, n):
    """A device-form writer: call(d_out, cap, d_out_off, d_status) -> (out bytes, out_off, status)."""
    room, d_off, d_st = _a5(cap + 16), _a5((n + 1) * 8), _a5(n)
    base = (-room.data_ptr()) % 16
    call(room.data_ptr() + base, cap, d_off.data_ptr(), d_st.data_ptr())
    out_off = _down(d_off, np.uint64, (n + 1,))
    total = int(out_off[n])
    whole = room.cpu().numpy()
    assert (whole[:base] == 0xA5).all() and (whole[base + total:] == 0xA5).all(), "bytes outside the output were written"
    return whole[base:base + total].tobytes(), out_off, _down(d_st, np.uint8, (n,))


def _encode_dev(e, buf, offs, routes, order=None):
    n = len(offs)
    silo, act, status, placed, ntype = routes
    t = [_up(np.frombuffer(buf, np.uint8)), _up(offs, np.uint64), _up(silo, np.uint32), _up(act, np.uint32),
         _up(status, np.uint8), _up(placed, np.uint8), _up(ntype, np.uint32)]
    d_od = None if order is None else _up(order, np.uint32)

    def call(out, cap, off, st):
        e.encode_frames_device(t[0].data_ptr(), len(buf), t[1].data_ptr(), n, t[2].data_ptr(), t[3].data_ptr(),
                               t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr(), None if d_od is None else d_od.data_ptr(),
                               out, cap, off, st)
        e.synchronize()
    return _writer_dev(call, len(buf) + n * 128, n)


def _respond_dev(e, d_buf, blen, d_off, n, args, order=None):
    kind, result, rej, info, body, body_off = args
    t = [_up(kind, np.uint8), _up(result, np.uint8), _up(rej, np.uint8), _up(info, np.uint32),
         _up(np.frombuffer(body or b"\0", np.uint8)), _up(body_off, np.uint64)]
    d_od = None if order is None else _up(order, np.uint32)

    def call(out, cap, off, st):
        e.respond_frames_device(d_buf.data_ptr(), blen, d_off.data_ptr(), n, t[0].data_ptr(), t[1].data_ptr(),
                                t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(),
                                None if d_od is None else d_od.data_ptr(), out, cap, off, st)
        e.synchronize()
    return _writer_dev(call, blen + len(body) + n * 96, n)


def _routes(rng, n):
    silo = rng.integers(0, len(CFG.silos), size=n).astype(np.uint32)
    silo[rng.random(n) < 0.03] = len(CFG.silos) + 2
    act = rng.integers(0, len(CFG.act_ids), size=n).astype(np.uint32)
    status = rng.choice([E.ROUTE_OK, E.ROUTE_ADDRESSED, E.ROUTE_MISS], size=n, p=[0.85, 0.1, 0.05]).astype(np.uint8)
    placed = rng.integers(0, 3, size=n).astype(np.uint8)
    ntype = rng.integers(0, len(CFG.type_names) + 1, size=n).astype(np.uint32)
    return silo, act, status, placed, ntype


def _answers(rng, n):
    kind = rng.choice([R.RSP_RESPONSE, R.RSP_REJECTION, R.RSP_NONE], size=n, p=[0.5, 0.45, 0.05]).astype(np.uint8)
    result = rng.integers(0, 2, size=n).astype(np.uint8)
    rej = rng.integers(0, 4, size=n).astype(np.uint8)
    info = rng.integers(0, len(R.INFOS) + 1, size=n).astype(np.uint32)
    body_off = np.zeros(n + 1, np.uint64)
    body_off[1:] = np.cumsum(rng.integers(0, 24, size=n))
    body = bytes(rng.integers(0, 256, size=int(body_off[n]), dtype=np.uint8))
    return kind, result, rej, info, body, body_off


# ---- the option
def test_option_off_is_today(gd):
    """No option set: the FALLBACK statuses of today and never GD_FRAME_INVALIDATION, in all three stages."""
    rng = np.random.default_rng(2)
    buf, offs = X.mixed_batch(257, rng)
    n = len(offs)
    e = _engine(gd, False)
    try:
        got = e.decode_frames(buf, offs)
        _same_fields(got, H.decode_frames(buf, offs), X.DECODE_KEYS)
        assert not (got["flags"] & X.F_INVALIDATION).any()
        has = (H.decode_frames(buf, offs)["mask"] & X.CIH) != 0
        assert has.sum() > 100 and ((got["flags"][has] & H.F_FALLBACK) != 0).all()
        routes = _routes(rng, n)
        out, off, st = _encode_dev(e, buf, offs, routes)
        want = E.encode_batch(buf, offs, *routes, None, CFG)
        assert out == want[0] and np.array_equal(off, want[1]) and np.array_equal(st, want[2])
        assert (st[has & (routes[2] == E.ROUTE_OK)] == E.ENC_FALLBACK).all()
        ans = _answers(rng, n)
        out, off, st = _respond_dev(e, _up(np.frombuffer(buf, np.uint8)), len(buf), _up(offs, np.uint64), n, ans)
        want = R.respond_batch(buf, offs, *ans, None, R.INFOS)
        assert out == want[0] and np.array_equal(off, want[1]) and np.array_equal(st, want[2])
    finally:
        e.close()


def test_option_values(gd, eng):
    assert gd.OPT_WALK_INVALIDATION == 18 and gd.FRAME_INVALIDATION == 0x20
    assert eng.get_option(gd.OPT_WALK_INVALIDATION) == 1
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        assert e.get_option(18) == 0
        for bad in (2, -1):
            with pytest.raises(gd.GrainDispatchError) as ex:
                e.set_option(18, bad)
            assert ex.value.code == gd.GD_EINVAL
        e.set_option(18, 1)
        e.set_option(18, 0)
        assert e.get_option(18) == 0


# ---- decoder
@pytest.mark.parametrize("turn", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_decoder(gd, eng, batches, n, turn):
    buf, offs, want = batches[n]
    got = _decode_dev(gd, eng, _up(np.frombuffer(buf, np.uint8)), len(buf), _up(offs, np.uint64), n, turn)
    _same_fields(got, want, X.DECODE_KEYS + (tuple(FT.TURN_FIELDS) if turn else ()))
    if n == 257:
        f, inv = want["flags"], X.F_INVALIDATION
        assert ((f & inv) != 0).sum() > 100 and (f == H.F_MALFORMED).sum() >= 5
        assert ((f & inv) != 0)[(f & H.F_FALLBACK) != 0].any() and (f == H.F_HAS_TARGET).any()
        assert (f & (inv | H.F_TARGET_KEYEXT) == inv | H.F_TARGET_KEYEXT).any()


@pytest.mark.parametrize("align", range(4))
def test_window_edge(gd, eng, align):
    rng = np.random.default_rng(50 + align)
    buf, offs, what = X.edge_frames(rng, align)
    n = len(offs)
    want = X.decode_batch(buf, offs)
    assert (want["flags"] & (X.F_INVALIDATION | H.F_TARGET_KEYEXT | H.F_MALFORMED) ==
            X.F_INVALIDATION | H.F_TARGET_KEYEXT).all()
    got = _decode_dev(gd, eng, _up(np.frombuffer(buf, np.uint8)), len(buf), _up(offs, np.uint64), n, True)
    _same_fields(got, want, X.DECODE_KEYS + tuple(FT.TURN_FIELDS))
    # the same frames through the two planners
    routes = (np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32) % 7 + 100, np.zeros(n, np.uint8),
              np.ones(n, np.uint8), np.zeros(n, np.uint32))
    routes[1][:] = [a for a in range(len(CFG.act_ids)) if CFG.act_ids[a].any()][:n]
    out, off, st = _encode_dev(eng, buf, offs, routes)
    want_e = E.encode_batch(buf, offs, *routes, None, CFG, form=X.encode_walk)
    assert out == want_e[0] and np.array_equal(st, want_e[2]) and (st == E.ENC_OK).all()
    ans = _answers(rng, n)
    out, off, st = _respond_dev(eng, _up(np.frombuffer(buf, np.uint8)), len(buf), _up(offs, np.uint64), n, ans)
    want_r = R.respond_batch(buf, offs, *ans, None, R.INFOS, form=X.respond_walk)
    assert out == want_r[0] and np.array_equal(st, want_r[2])


def test_target_keyext_offset(gd):
    """A TargetGrain with a KeyExt string behind the entries, routed by that string (gd_route_frames_ext): the
    offset the decoder hands the KeyExt pass is the string's place in the real buffer."""
    silos = o.bench_silos(8)
    spec = o.ring_spec(silos, "D")
    rng = np.random.default_rng(23)
    e = gd.GrainDispatch(device=0, table_capacity=1 << 12, options={gd.OPT_WALK_INVALIDATION: 1})
    try:
        e.ring_set_silos("D", [(s.ip, s.port, s.gen) for s in silos])
        G = 200
        reg = o.grain_keys(TC, np.arange(G))
        own = o.ring_owner_np(spec, o.jenkins_u64x3_np(reg[:, 2], reg[:, 0], reg[:, 1])).astype(np.uint32)
        e.register(reg, np.arange(G), own)
        d = kx.KeyExtDirectory()
        names = [f"device/{i}" + "q" * (i % 41) for i in range(120)]
        tcd = o.type_code_data(o.CAT_KEYEXT_GRAIN, 0x2A2A)
        e.register_ext(np.tile(np.array([[0, 0, tcd]], np.uint64), (80, 1)), names[:80], np.arange(80) + G, np.arange(80) % 8)
        for i in range(80):
            d.add_single_activation((0, 0, tcd), names[i].encode(), G + i, i % 8)
        frames = []
        for i in range(300):
            tg = ((0, 0, tcd), names[int(rng.integers(0, 120))]) if i % 2 else \
                (tuple(int(x) for x in o.grain_keys(TC, [int(rng.integers(0, G + 20))])[0]), None)
            fld = F.w_invalidation([X.entry(rng, grain_ext="e" * int(rng.integers(0, 30))) for _ in range(i % 4)])
            frames.append(X.request(rng, field=fld if i % 5 else None, debug="d" * int(rng.integers(0, 60)), target_grain=tg))
        buf, offs = F.pack_frames(frames, b"\0\0\0")
        cbuf, coffs = X.cut_batch(buf, offs)
        _, wst, wsilo, wact = H.route_frames_ext_np(cbuf, coffs, spec, o.DirectoryArrays(reg, np.arange(G), own), d)
        f, st, silo, act, perm, off = e.route_frames(buf, offs, G + 80, keyext=True)
        np.testing.assert_array_equal(st, wst)
        np.testing.assert_array_equal(silo, wsilo)
        np.testing.assert_array_equal(act, wact)
        wp, wo = o.bucket_stable(wact, G + 80)
        np.testing.assert_array_equal(perm, wp)
        np.testing.assert_array_equal(off, wo)
        kxt = np.array([i % 2 == 1 for i in range(300)])
        assert ((wst == o.ST_OK) & kxt).sum() > 60 and ((f["flags"] & X.F_INVALIDATION) != 0).sum() > 200
    finally:
        e.close()


def test_malformed(gd, eng):
    rng = np.random.default_rng(4)
    bad = X.malformed(rng)
    buf, offs = F.pack_frames([X.request(rng, count=1)] + bad + [X.request(rng, count=2)], b"\0")
    got = eng.decode_frames(buf, offs)
    _same_fields(got, X.decode_batch(buf, offs), X.DECODE_KEYS)
    assert (got["flags"][1:-1] == H.F_MALFORMED).all() and (got["flags"][[0, -1]] & H.F_HAS_TARGET).all()
    # the last frame ends at the last byte of a buffer whose length is no multiple of 4; one byte short it is cut
    buf, offs = X.unaligned_tail(rng)
    assert len(buf) % 4
    for b in (buf, buf[:-1]):
        got = _decode_dev(gd, eng, _up(np.frombuffer(b, np.uint8)), len(b), _up(offs, np.uint64), 2, True)
        _same_fields(got, X.decode_batch(b, offs), X.DECODE_KEYS + tuple(FT.TURN_FIELDS))
    assert got["flags"][1] == H.F_MALFORMED


# ---- encoder and responder
@pytest.mark.parametrize("n", SIZES)
def test_encoder(gd, eng, batches, n):
    buf, offs, _ = batches[n]
    rng = np.random.default_rng(60 + n)
    routes = _routes(rng, n)
    want = E.encode_batch(buf, offs, *routes, None, CFG, form=X.encode_walk)
    out, off, st = _encode_dev(eng, buf, offs, routes)
    assert out == want[0] and np.array_equal(off, want[1]) and np.array_equal(st, want[2])
    if n == 257:
        has = (X.decode_batch(buf, offs)["flags"] & X.F_INVALIDATION) != 0
        assert (st[has] == E.ENC_OK).sum() > 60 and (st[has] == E.ENC_FALLBACK).any() and (st == E.ENC_MALFORMED).any()
        # gd_send_queues' order: each queue's frames are one byte run
        sh = SQ.hashes_with_edges(rng, len(CFG.silos) + 4)
        e = _engine(gd, True, my_silo=1)
        try:
            e.send_configure(sh, 7)
            _, _, perm, _ = e.send_queues(routes[0], routes[2])
            got = _encode_dev(e, buf, offs, routes, perm)
        finally:
            e.close()
        want = E.encode_batch(buf, offs, *routes, perm, CFG, form=X.encode_walk)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("n", SIZES)
def test_responder(gd, eng, batches, n):
    buf, offs, _ = batches[n]
    rng = np.random.default_rng(70 + n)
    ans = _answers(rng, n)
    order = None if n % 2 else rng.permutation(n).astype(np.uint32)
    want = R.respond_batch(buf, offs, *ans, order, R.INFOS, form=X.respond_walk)
    out, off, st = _respond_dev(eng, _up(np.frombuffer(buf, np.uint8)), len(buf), _up(offs, np.uint64), n, ans, order)
    assert out == want[0] and np.array_equal(off, want[1]) and np.array_equal(st, want[2])
    if n == 257:
        kinds = set(ans[0][st == R.ST_OK].tolist())
        assert {R.RSP_RESPONSE, R.RSP_REJECTION} <= kinds and (st == R.ST_FALLBACK).any() and (st == R.ST_MALFORMED).any()


def test_responder_count_zero_and_default_category(gd, eng):
    """Count 0: the answer's mask drops the bit.  Count > 0 with a default-valued Category byte and a DebugContext:
    GD_RSPST_FALLBACK (run 0 of the plan would be two runs); its neighbours are answered."""
    rng = np.random.default_rng(3)
    kws = [dict(count=0), dict(count=0, category=0, debug="kept"), dict(count=1, category=0, debug="kept"),
           dict(count=1, category=0), dict(count=1, category=0, debug=""), dict(count=1, category=None, debug="kept"),
           dict(count=2, category=2, debug="kept"), dict(count=3, category=None)]
    frames = [X.request(rng, **kw) for kw in kws]
    buf, offs = F.pack_frames(frames, b"\0\0")
    n = len(offs)
    for kind in (R.RSP_RESPONSE, R.RSP_REJECTION):
        ans = (np.full(n, kind, np.uint8), np.zeros(n, np.uint8), np.ones(n, np.uint8), np.zeros(n, np.uint32), b"", None)
        out, off, st, _ = eng.respond_frames(buf, offs, *ans)
        want = R.respond_batch(buf, offs, *ans, None, R.INFOS, form=X.respond_walk)
        assert bytes(out[:int(off[n])]) == want[0] and np.array_equal(off, want[1]) and np.array_equal(st, want[2])
        assert st.tolist() == [R.ST_OK, R.ST_OK, R.ST_FALLBACK] + [R.ST_OK] * 5
        masks = [struct.unpack_from("<I", out, int(off[j]) + 8)[0] for j in range(n)]
        assert not masks[0] & X.CIH and not masks[1] & X.CIH and all(m & X.CIH for m in masks[3:])


# ---- host-pointer forms
def test_host_forms(gd, eng, batches):
    buf, offs, want = batches[65]
    n = len(offs)
    _same_fields(eng.decode_frames(buf, offs), want, X.DECODE_KEYS)
    f, t = eng.decode_frames_turn(buf, offs)
    _same_fields(dict(f, **t), want, X.DECODE_KEYS + tuple(FT.TURN_FIELDS))
    rng = np.random.default_rng(11)
    routes = _routes(rng, n)
    out, off, st, total = eng.encode_frames(buf, offs, *routes)
    w = E.encode_batch(buf, offs, *routes, None, CFG, form=X.encode_walk)
    assert bytes(out[:total]) == w[0] and np.array_equal(off, w[1]) and np.array_equal(st, w[2])
    ans = _answers(rng, n)
    out, off, st, total = eng.respond_frames(buf, offs, *ans)
    w = R.respond_batch(buf, offs, *ans, None, R.INFOS, form=X.respond_walk)
    assert bytes(out[:total]) == w[0] and np.array_equal(off, w[1]) and np.array_equal(st, w[2])


# ---- what the feature is for
def test_round_trip(gd):
    """gd_forward_frames_device writes a batch; its output buffer goes, on the device, through the sniff stage, decode
    + route + bucket, and the responder."""
    rng = np.random.default_rng(77)
    n = 300
    silos = o.bench_silos(8)
    e = _engine(gd, True)
    try:
        e.ring_set_silos("D", [(s.ip, s.port, s.gen) for s in silos])
        good = np.array([a for a in range(len(CFG.act_ids)) if CFG.act_ids[a].any()], np.uint32)
        frames = [X.request(rng, count=[None, 0, 1, 2][i % 4], debug="d" * int(rng.integers(0, 70)),
                            tg_ext=None if i % 3 else "g" * (i % 29), body=bytes(i % 13)) for i in range(n)]
        buf, offs = F.pack_frames(frames, b"\0")
        kind = np.full(n, F.FWD_FORWARD, np.uint8)
        old_act, fwd_act = rng.choice(good, n), rng.choice(good, n)
        fwd_silo = rng.integers(0, len(CFG.silos), n).astype(np.uint32)
        t = [_up(np.frombuffer(buf, np.uint8)), _up(offs, np.uint64), _up(kind), _up(old_act), _up(fwd_silo), _up(fwd_act)]
        db = {"buf": t[0].data_ptr(), "buf_len": len(buf), "frame_off": t[1].data_ptr(), "kind": t[2].data_ptr(),
              "old_act": t[3].data_ptr(), "fwd_silo": t[4].data_ptr(), "fwd_act": t[5].data_ptr(),
              "max_forward_count": 2, "local_silo": F.LOCAL_SILO}
        cap = 2 * len(buf) + n * 256
        d_out, d_off, d_fst, d_tg = _a5(cap), _a5((n + 1) * 8), _a5(n), _a5(n * 24)
        e.forward_frames_device(db, n, None, None, None, None, None, None, d_out.data_ptr(), cap, d_off.data_ptr(),
                                d_fst.data_ptr(), d_tg.data_ptr())
        e.synchronize()
        out_off = _down(d_off, np.uint64, (n + 1,))
        total = int(out_off[n])
        assert (_down(d_fst, np.uint8, (n,)) == F.ST_OK_ADDRESSED).all()
        fwd = d_out.cpu().numpy()[:total].tobytes()
        foffs = out_off[:n].copy()
        d_foff = _up(foffs)

        # the sniff stage
        so = {"count": _a5(n * 4), "ent_off": _a5((n + 1) * 4), "status": _a5(n), "flags": _a5(n)}
        e.sniff_frames_device(d_out.data_ptr(), total, d_foff.data_ptr(), n, {k: v.data_ptr() for k, v in so.items()},
                              total // 80)                                     # no entry array is wanted
        e.synchronize()
        count = _down(so["count"], np.uint32, (n,))
        assert (_down(so["status"], np.uint8, (n,)) == 1).all()                # GD_SNIFF_OK
        had = np.array([0 if i % 4 == 0 else i % 4 - 1 for i in range(n)], np.uint32)
        np.testing.assert_array_equal(count, had + 1)                          # the forwarder appended one entry

        # decode + route + bucket
        sz = lambda dt, sh: n * np.dtype(dt).itemsize * int(np.prod(sh, dtype=np.int64))
        d = {k: _a5(sz(dt, sh)) for k, (dt, sh) in gd.FRAME_FIELDS.items()}
        r = {"silo": _a5(n * 4), "act": _a5(n * 4), "status": _a5(n), "perm": _a5(n * 4), "offs": _a5((64 + 2) * 4)}
        e.route_frames_device(d_out.data_ptr(), total, d_foff.data_ptr(), n, 64, {k: v.data_ptr() for k, v in d.items()},
                              r["silo"].data_ptr(), r["act"].data_ptr(), r["status"].data_ptr(), r["perm"].data_ptr(),
                              r["offs"].data_ptr())
        e.synchronize()
        got = {k: _down(d[k], dt, (n,) + sh) for k, (dt, sh) in gd.FRAME_FIELDS.items()}
        _same_fields(got, X.decode_batch(fwd, foffs), X.DECODE_KEYS)
        want_flags = H.F_HAS_TARGET | X.F_INVALIDATION
        assert (got["flags"] & want_flags == want_flags).all() and (got["flags"] & H.F_COMPLETE).all()
        np.testing.assert_array_equal(got["target_activation"], CFG.act_ids[fwd_act])
        np.testing.assert_array_equal(got["target_silo"],
                                      np.frombuffer(b"".join(CFG.silos[s] for s in fwd_silo), np.uint8).reshape(n, 24))
        np.testing.assert_array_equal(got["target_grain"], X.decode_batch(buf, offs)["target_grain"])
        assert (_down(r["status"], np.uint8, (n,)) == H.ROUTE_ADDRESSED).all()
        # the decoder's view and the sniff stage's agree frame by frame
        np.testing.assert_array_equal(((got["flags"] & X.F_INVALIDATION) != 0), count > 0)

        # the answers
        ans = _answers(rng, n)
        ans = (np.where(ans[0] == R.RSP_NONE, R.RSP_RESPONSE, ans[0]).astype(np.uint8),) + ans[1:]
        out, off, st = _respond_dev(e, d_out, total, d_foff, n, ans)
        want = R.respond_batch(fwd, foffs, *ans, None, R.INFOS, form=X.respond_walk)
        assert out == want[0] and np.array_equal(off, want[1]) and np.array_equal(st, want[2])
        assert (st == R.ST_OK).all()
        for j in range(n):
            field = X.cut_frame(fwd, int(foffs[j]))[1]
            a = out[int(off[j]):int(off[j + 1])]
            assert struct.unpack_from("<I", a, 8)[0] & X.CIH and a[12:12 + len(field)] == field
    finally:
        e.close()


# ---- the chain
def test_chain_creates_the_activation_of_a_forwarded_new_placement(gd):
    """gd_receive_activate_turns_frames: addressed frames that carry an invalidation header, IsNewPlacement true, false
    or absent.  The reference is the chain's own on the batch with every field cut out; without the walk in
    k_actv_newp no frame with the header would be a new placement and its activation would be NONEXISTENT."""
    rng = np.random.default_rng(31)
    n, n_ex = 150, 20
    n_ctx = n_ex + n + 8
    keys = A.act_keys(rng, n_ex + 30)
    entries = {tuple(int(x) for x in k): (j, (j % 3 != 0) * A.AD_VALID) for j, k in enumerate(keys[:n_ex])}
    frames, truth = [], []
    for i in range(n):
        ta = keys[rng.integers(0, len(keys))]
        h = FT.turn_frame(rng, o.grain_keys(TC, [int(rng.integers(0, 1000))])[0], ta, sa=ta, direction=int(rng.choice([0, 0, 0, 1])))
        h.pop("is_new_placement", None)
        if i % 3 < 2:
            h["is_new_placement"] = i % 3 == 0
        if i % 7:
            h["cache_invalidation"] = F.w_invalidation([X.entry(rng) for _ in range(i % 3)])
        truth.append(1 if i % 3 == 0 else 0)
        frames.append(H.encode_frame(h, bytes(i % 9)))
    truth = np.array(truth, np.uint8)
    buf, offs = F.pack_frames(frames, b"\0\0\0")
    cbuf, coffs = X.cut_batch(buf, offs)
    f, t = H.decode_frames(cbuf, coffs), FT.walk_frames(cbuf, coffs)
    st, ctx, _, _ = FT.receive_frames_ref(f, list(entries), [v[0] for v in entries.values()],
                                          [v[1] for v in entries.values()], n_ctx)
    cap = int(truth.sum())
    b = A.Batch(ctx, st, f["target_activation"], n_ctx, cap, entries, ctx_base=n_ex, direction=f["direction"],
                ttl=t["ttl"], new_placement=truth)
    fl, nr = T.context_state(rng, n_ctx)
    fl[n_ex:], nr[n_ex:] = T.CTX_NOT_READY, 0
    rc = np.zeros(n_ctx, np.uint32)
    want = A.chain_model(b, fl, nr, rc, t["forward_count"], t["msg_flags"], f["sending_activation"])
    with gd.GrainDispatch(device=0, table_capacity=1024, options={gd.OPT_WALK_INVALIDATION: 1}) as e:
        ids = np.array(list(entries), np.uint64)
        assert e.actdir_add(ids, [v[0] for v in entries.values()], [v[1] for v in entries.values()]).all()
        got = e.receive_activate_turns_frames(buf, offs, n_ctx, fl, nr, rc, cap, ctx_base=n_ex)
    for k in ("kind", "ctx", "status", "new_idx", "gone_idx", "perm", "offsets", "turn", "num_running_out",
              "running_idx", "start_idx", "wait_perm", "wait_offsets"):
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    has = np.array([i % 7 != 0 for i in range(n)])
    created = want["kind"] == A.ACTV_CREATED
    assert (created & has).sum() >= 5 and (truth[want["new_idx"]] == 1).all()
