"""GPU parity for the frame encoder (gd_encode_frames*): Message.SetTargetPlacement +
Message.Serialize for a batch, bit for bit against the reference's literal form (_encode_ref.py): the encode
status of every frame, out_off, and every output byte; and no byte outside the output is written.

Every device run goes into a buffer pre-filled with 0xA5 that has 64 spare bytes: the bytes at or past
out_off[n] must still be 0xA5 (_dev)."""
import struct

import numpy as np
import pytest

import _encode_ref as R
import _sendq_ref as SQ
import headers as H
import oracle as o

pytestmark = pytest.mark.gpu

SILO_TUPLES = [(f"10.0.0.{1 + s}", 11000 + s, 100 + 7 * s) for s in range(5)]
LONG_TYPE = "N" * 200
TILE = 16384                                     # k_enc_write's output bytes a workgroup (gd_encode.h)
CFG = R.make_config(np.random.default_rng(1))
CFG.type_names = R.TYPE_NAMES + [LONG_TYPE]


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


def _configure(e):
    e.encode_configure(SILO_TUPLES, CFG.type_names)
    live = np.flatnonzero(CFG.act_ids.any(axis=1)).astype(np.uint32)
    e.activation_ids_set(live, CFG.act_ids[live])


@pytest.fixture(scope="module")
def eng(gd):
    assert [bytes(gd.silo_addr(*s).ip) + struct.pack("<ii", s[1], s[2]) for s in SILO_TUPLES] == CFG.silos
    e = gd.GrainDispatch(device=0, table_capacity=1 << 12)
    _configure(e)
    yield e
    e.close()


def _dev(e, buf, offs, silo, act, status, placed=None, new_type=None, order=None, lead=0, out_cap=None):
    """gd_encode_frames_device on torch buffers.  Returns (out bytes, out_off, enc_status, whole buffer)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(offs)
    up = lambda a, dt, t: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt)).view(t)).to(dev)
    d_buf = torch.from_numpy(np.frombuffer(buf or b"\0", dtype=np.uint8).copy()).to(dev)
    d_off = up(offs if n else [0], np.uint64, np.int64)
    d_silo, d_act = up(silo if n else [0], np.uint32, np.int32), up(act if n else [0], np.uint32, np.int32)
    d_st = up(status if n else [0], np.uint8, np.uint8)
    d_pl, d_nt, d_od = up(placed, np.uint8, np.uint8), up(new_type, np.uint32, np.int32), up(order, np.uint32, np.int32)
    cap = len(buf) + n * 300 if out_cap is None else out_cap
    room = torch.full((lead + cap + 64 + 16,), 0xA5, dtype=torch.uint8, device=dev)
    base = (-room.data_ptr()) % 16 + lead                          # out pointer = 16-B boundary + lead
    d_out_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_est = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize()
    e.encode_frames_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n, d_silo.data_ptr(), d_act.data_ptr(),
                           d_st.data_ptr(), ptr(d_pl), ptr(d_nt), ptr(d_od), room.data_ptr() + base, cap,
                           d_out_off.data_ptr(), d_est.data_ptr())
    err = None
    try:
        e.synchronize()
    except Exception as ex:                                        # GD_EFULL surfaces here; the caller checks
        err = ex
    whole = room.cpu().numpy()
    out_off = d_out_off.cpu().numpy().view(np.uint64)
    total = int(out_off[n])
    assert (whole[:base] == 0xA5).all(), "bytes before the output were written"
    keep = base + (total if err is None else 0)
    assert (whole[keep:] == 0xA5).all(), "bytes at or past out_off[n] were written"
    if err is not None:
        raise err
    return whole[base:base + total].tobytes(), out_off, d_est.cpu().numpy()[:n], whole


def _same(got, want):
    out, off, est = got[:3]
    wout, woff, west = want
    np.testing.assert_array_equal(est, west, err_msg="enc_status")
    np.testing.assert_array_equal(off, woff, err_msg="out_off")
    if out != wout:
        a, b = np.frombuffer(out, np.uint8), np.frombuffer(wout, np.uint8)
        k = int(np.flatnonzero(a != b)[0])
        j = int(np.searchsorted(woff, k, side="right")) - 1
        raise AssertionError(f"first differing byte {k} (output frame {j}, byte {k - int(woff[j])} of it): "
                             f"{a[k]:#x} != {b[k]:#x}")


def _check(e, batch, order=None, lead=0):
    buf, offs, silo, act, status, placed, new_type = batch
    want = R.encode_batch(buf, offs, silo, act, status, placed, new_type, order, CFG)
    _same(_dev(e, buf, offs, silo, act, status, placed, new_type, order, lead=lead), want)
    return want


def _frames(frames, pad=b""):
    buf, offs = pad, []
    for f in frames:
        offs.append(len(buf))
        buf += f
    return buf, np.array(offs, dtype=np.uint64)


def _ok_routes(n, silo=2, act=None):
    live = np.flatnonzero(CFG.act_ids.any(axis=1))
    a = np.full(n, live[3] if act is None else act, np.uint32)
    return np.full(n, silo, np.uint32), a, np.zeros(n, np.uint8)


K = (7, 8, 0x0300000000000011)
BASE = {"category": 2, "direction": 1, "correlation_id": 99, "target_grain": (K, None),
        "sending_silo": R.SILOS[0], "resend_count": 1}


# ----------------------------------------------------------------------------- batches
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4099])
def test_batch_sizes(eng, n):
    rng = np.random.default_rng(100 + n)
    batch = R.random_batch(n, rng, CFG)
    want = _check(eng, batch)
    if n >= 4099:
        assert set(np.unique(want[2]).tolist()) == set(range(7))
    # the host-pointer form
    buf, offs, silo, act, status, placed, new_type = batch
    out = np.full(len(buf) + n * 128 + 64, 0xA5, np.uint8)
    got, off, est, total = eng.encode_frames(buf, offs, silo, act, status, placed, new_type, out=out)
    assert got is out and total == len(want[0]) and (out[total:] == 0xA5).all()
    _same((out[:total].tobytes(), off, est), want)
    # the optional inputs absent
    want2 = R.encode_batch(buf, offs, silo, act, status, None, None, None, CFG)
    _same(_dev(eng, buf, offs, silo, act, status), want2)


def test_alignment_every_phase(eng):
    rng = np.random.default_rng(7)
    buf, offs, *routes = R.random_batch(65, rng, CFG)
    for pad in range(16):
        b2 = b"\x5a" * pad + buf
        _check(eng, (b2, offs + np.uint64(pad), *routes), lead=(5 * pad + 3) % 16)
    for lead in range(16):                                         # every phase of the output pointer
        _check(eng, (buf, offs, *routes), lead=lead)


def test_frame_at_buffer_end_and_unsorted_offsets(eng):
    rng = np.random.default_rng(8)
    buf, offs, *routes = R.random_batch(130, rng, CFG, p_malformed=0.0)
    last = H.encode_frame(dict(BASE, debug_context="end"), b"tail")
    buf2 = buf + last
    offs2 = np.append(offs, np.uint64(len(buf)))
    live = int(np.flatnonzero(CFG.act_ids.any(axis=1))[0])
    r2 = [np.append(r, v).astype(r.dtype) for r, v in zip(routes, (1, live, 0, 1, 0))]
    assert int(offs2[-1]) + len(last) == len(buf2)
    want = _check(eng, (buf2, offs2, *r2))
    assert want[2][-1] == R.ENC_OK
    rev = slice(None, None, -1)                                    # frame_off in descending order
    _check(eng, (buf2, offs2[rev].copy(), *[r[rev].copy() for r in r2]))


def test_order(eng, gd):
    rng = np.random.default_rng(9)
    n = 1500
    batch = R.random_batch(n, rng, CFG)
    buf, offs, silo, act, status, placed, new_type = batch
    for order in (np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)[::-1].copy(),
                  rng.permutation(n).astype(np.uint32)):
        _check(eng, batch, order=order)
    # gd_send_queues' perm: queue q's byte run = its messages' reference frames in batch order
    nq = 7
    sh = SQ.hashes_with_edges(rng, len(CFG.silos) + 4)
    with gd.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=1) as e:
        _configure(e)
        e.send_configure(sh, nq)
        sst, q, perm, qoff = e.send_queues(silo, status)
        got = _dev(e, buf, offs, silo, act, status, placed, new_type, perm)
    _same(got, R.encode_batch(buf, offs, silo, act, status, placed, new_type, perm, CFG))
    single = R.encode_batch(buf, offs, silo, act, status, placed, new_type, None, CFG)
    fr = lambda i: single[0][int(single[1][i]):int(single[1][i + 1])]
    assert sorted(perm.tolist()) == list(range(n))
    for b in range(len(qoff) - 1):
        members = perm[qoff[b]:qoff[b + 1]]
        assert (np.diff(members.astype(np.int64)) > 0).all()
        run = got[0][int(got[1][qoff[b]]):int(got[1][qoff[b + 1]])]
        assert run == b"".join(fr(int(i)) for i in members)


def test_long_headers_and_long_type(eng):
    frames = [H.encode_frame(BASE, b"a"),
              H.encode_frame(dict(BASE, debug_context="d" * 300), b"bb"),
              H.encode_frame(dict(BASE, debug_context="D" * 5000, is_new_placement=False, new_grain_type="Old"), b"c"),
              H.encode_frame(dict(BASE, sending_grain=((1, 2, 3), "s" * 400), target_activation=((1, 1, 1), "x" * 333))),
              H.encode_frame(dict(BASE, debug_context="e" * 170), b"dddd")]     # the window ends inside the walk
    for pad in (b"", b"\x01", b"\x01\x02\x03"):
        buf, offs = _frames(frames * 3, pad)
        n = len(offs)
        silo, act, st = _ok_routes(n)
        placed = np.tile(np.array([1, 0, 1], np.uint8), n)[:n]
        new_type = np.tile(np.array([len(R.TYPE_NAMES), R.NO_TYPE, 0, 2], np.uint32), n)[:n]   # the 200-B name first
        want = _check(eng, (buf, offs, silo, act, st, placed, new_type))
        assert (want[2] == R.ENC_OK).all()


def test_large_frames(eng):
    rng = np.random.default_rng(12)
    small = lambda k: H.encode_frame(dict(BASE, correlation_id=k), bytes(rng.integers(0, 256, size=k % 50, dtype=np.uint8)))
    big = lambda ln: H.encode_frame(dict(BASE, debug_context="big"), bytes(rng.integers(0, 256, size=ln, dtype=np.uint8)))
    frames = [big(70000)] + [small(k) for k in range(63)] + [big(0), big(1)] + [small(k) for k in range(62)] + \
             [big(300000)] + [small(k) for k in range(70)] + [big(70000)]
    buf, offs = _frames(frames, b"\x09" * 3)
    n = len(offs)
    silo, act, st = _ok_routes(n)
    st[5] = R.ROUTE_ADDRESSED
    st[64 + 63] = R.ROUTE_ADDRESSED                                # the 300,000-B frame copied, then patched
    want = _check(eng, (buf, offs, silo, act, st, np.ones(n, np.uint8), np.zeros(n, np.uint32)), lead=9)
    st[64 + 63] = 0
    _check(eng, (buf, offs, silo, act, st, None, None), order=np.random.default_rng(1).permutation(n).astype(np.uint32))
    assert want[2][64 + 63] == R.ENC_COPIED


def test_tile_edges(eng):
    """Frame boundaries against the writer's 16-KiB output tiles at every residue; runs of zero-length frames,
    also more of them inside one tile than the writer keeps offsets for in LDS; an all-skipped batch."""
    rng = np.random.default_rng(13)
    frames = [H.encode_frame(dict(BASE, correlation_id=k), bytes(rng.integers(0, 256, size=(k * 7) % 61, dtype=np.uint8)))
              for k in range(260)]
    for r in range(16):
        head = H.encode_frame(BASE, b"h" * r)
        buf, offs = _frames([head] + frames)
        n = len(offs)
        silo, act, st = _ok_routes(n)
        want = _check(eng, (buf, offs, silo, act, st, None, None), lead=r)
        assert len(want[0]) > 2 * TILE
    buf, offs = _frames(frames)
    n = len(offs)
    silo, act, st = _ok_routes(n)
    st[100:164] = R.ROUTE_MISS                                     # 64 zero-length frames in a row
    st[0] = st[n - 1] = R.ROUTE_KEYEXT                             # and at both ends
    _check(eng, (buf, offs, silo, act, st, None, None))
    buf, offs = _frames(frames[:40] + [frames[0]] * 1500 + frames[40:80])
    n = len(offs)
    silo, act, st = _ok_routes(n)
    st[40:1540] = R.ROUTE_MULTI_ACT                                # 1,500 zero-length frames inside one tile
    _check(eng, (buf, offs, silo, act, st, None, None))
    st[:] = R.ROUTE_MISS                                           # all skipped: total 0, nothing written
    want = _check(eng, (buf, offs, silo, act, st, None, None))
    assert want[0] == b"" and (want[2] == R.ENC_SKIPPED).all()


def test_non_canonical_inputs(eng):
    own = dict(BASE, target_activation=((9, 9, 9), "old-ext"), target_silo=R.SILOS[4])
    frames = [H.encode_frame(own, b"1"),
              H.encode_frame(dict(BASE, is_new_placement=False, read_only=True), b"22"),
              H.encode_frame(dict(BASE, is_new_placement=False), b"22"),
              H.encode_frame(dict(BASE, new_grain_type="Own.Type"), b"333"),
              H.encode_frame(dict(BASE, new_grain_type="Own.Type"), b"333"),
              H.encode_frame(dict(BASE, target_observer=b"\x07" * 13), b"4"),
              H.encode_frame(dict(BASE, target_observer=b"\x07" * 13, target_silo=R.SILOS[1]), b"4"),
              H.encode_frame(dict(BASE, transaction_info=b"\x05" * 9, is_using_interface_version=True), b"5"),
              H.encode_frame(dict(BASE, target_observer=b"o" * 5, transaction_info=b"t" * 5), b"6"),
              H.encode_frame(dict(own, debug_context="copied"), b"7")]
    buf, offs = _frames(frames, b"\x00")
    n = len(offs)
    silo, act, st = _ok_routes(n)
    st[9] = R.ROUTE_ADDRESSED
    placed = np.array([0, 1, 2, 0, 0, 1, 0, 0, 0, 1], np.uint8)
    new_type = np.array([R.NO_TYPE, R.NO_TYPE, R.NO_TYPE, 0, R.NO_TYPE, 3, 1, 2, 0, 0], np.uint32)
    want = _check(eng, (buf, offs, silo, act, st, placed, new_type))
    assert want[2].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, R.ENC_FALLBACK, R.ENC_COPIED]


def test_round_trip_through_the_decoder(eng):
    rng = np.random.default_rng(14)
    batch = R.random_batch(2000, rng, CFG, p_malformed=0.0)
    buf, offs, silo, act, status, placed, new_type = batch
    out, off, est, _ = _dev(eng, *batch)
    ok = np.flatnonzero(est == R.ENC_OK)
    assert len(ok) > 1000
    before = eng.decode_frames(buf, offs[ok])
    after = eng.decode_frames(out, off[ok])
    assert ((after["flags"] & H.F_COMPLETE) != 0).all() and ((after["flags"] & H.F_MALFORMED) == 0).all()
    np.testing.assert_array_equal(after["target_activation"], CFG.act_ids[act[ok]])
    direct = (after["flags"] & H.F_FALLBACK) == 0                  # TargetObserver: the decoder leaves TargetSilo
    want_silo = np.frombuffer(b"".join(CFG.silos[int(s)] for s in silo[ok]), np.uint8).reshape(-1, 24)
    np.testing.assert_array_equal(after["target_silo"][direct], want_silo[direct])
    for k in ("target_grain", "sending_activation", "sending_grain", "sending_silo", "correlation_id", "category",
              "direction"):
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    set_bits = H.TARGET_ACTIVATION | H.TARGET_SILO | H.IS_NEW_PLACEMENT | H.NEW_GRAIN_TYPE
    np.testing.assert_array_equal(after["mask"] & ~np.uint32(set_bits), before["mask"] & ~np.uint32(set_bits))


def test_capacity(eng, gd):
    rng = np.random.default_rng(15)
    batch = R.random_batch(300, rng, CFG)
    buf, offs, silo, act, status, placed, new_type = batch
    want = R.encode_batch(*batch, None, CFG)
    total = len(want[0])
    out = np.full(total - 1, 0xA5, np.uint8)
    with pytest.raises(gd.GrainDispatchError) as ei:
        eng.encode_frames(*batch, out=out)
    assert ei.value.code == gd.GD_EFULL
    assert (out == 0xA5).all()
    with pytest.raises(gd.GrainDispatchError) as ei:               # the device form: at the next synchronisation,
        _dev(eng, *batch, out_cap=total - 1)                       # out_off complete, nothing written (_dev)
    assert ei.value.code == gd.GD_EFULL
    out = np.full(total, 0xA5, np.uint8)                           # exactly enough; the handle still works
    got, off, est, tot = eng.encode_frames(*batch, out=out)
    assert tot == total
    _same((out.tobytes(), off, est), want)


def test_capacity_out_off_complete(eng, gd):
    rng = np.random.default_rng(16)
    batch = R.random_batch(100, rng, CFG)
    want = R.encode_batch(*batch, None, CFG)
    off = np.zeros(101, np.uint64)
    est = np.zeros(100, np.uint8)
    out = np.full(10, 0xA5, np.uint8)
    buf, offs, silo, act, status, placed, new_type = batch
    b = np.frombuffer(buf, np.uint8)
    tot = gd.C.c_uint64(0)
    rc = gd.lib.gd_encode_frames(eng.h, b.ctypes.data, len(buf), offs.ctypes.data, 100, silo.ctypes.data,
                                 act.ctypes.data, status.ctypes.data, placed.ctypes.data, new_type.ctypes.data, None,
                                 out.ctypes.data, 10, off.ctypes.data, est.ctypes.data, gd.C.byref(tot))
    assert rc == gd.GD_EFULL and tot.value == len(want[0])
    np.testing.assert_array_equal(off, want[1])
    np.testing.assert_array_equal(est, want[2])
    assert (out == 0xA5).all()


def test_device_chain(gd):
    """gd_route_frames_device -> gd_send_queues_device -> gd_encode_frames_device on one handle, nothing read
    back in between, against the oracle's route, the sender-queue reference and the encoder reference."""
    import torch
    G, n, nq, my = 3000, 5000, 5, 3
    silos = o.bench_silos(5)
    spec = o.ring_spec(silos, "D")
    rng = np.random.default_rng(17)
    reg = o.grain_keys(77, np.arange(G))
    owner = o.ring_owner_np(spec, o.jenkins_u64x3_np(reg[:, 2], reg[:, 0], reg[:, 1]))
    acts = rng.permutation(len(CFG.act_ids) * 8)[:G].astype(np.uint32) % np.uint32(len(CFG.act_ids))
    keys = o.grain_keys(77, rng.integers(0, G + 300, size=n))
    buf, offs = H.random_frames(n, keys, rng, p_fallback=0.03, p_complete=0.08, p_malformed=0.01)
    sh = SQ.hashes_with_edges(rng, len(silos))
    dev = torch.device("cuda:0")
    with gd.GrainDispatch(device=0, table_capacity=1 << 13, my_silo=my) as e:
        e.ring_set_silos("D", [(s.ip, s.port, s.gen) for s in silos], 30)
        e.register(reg, acts, owner)
        _configure(e)
        e.send_configure(sh, nq)
        d_buf = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).to(dev)
        d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
        flags, tg = i32(n), torch.empty((n, 3), dtype=torch.int64, device=dev)
        silo, act, perm, qoff = i32(n), i32(n), i32(n), i32(nq + 5)
        st, sst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        cap = len(buf) + 64 * n
        out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=dev)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        est = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        e.route_frames_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n, 0,
                              {"flags": flags.data_ptr(), "target_grain": tg.data_ptr()}, silo.data_ptr(),
                              act.data_ptr(), st.data_ptr(), None, None)
        e.send_queues_device(silo.data_ptr(), st.data_ptr(), None, None, n, sst.data_ptr(), None, perm.data_ptr(),
                             qoff.data_ptr())
        e.encode_frames_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n, silo.data_ptr(), act.data_ptr(),
                               st.data_ptr(), None, None, perm.data_ptr(), out.data_ptr(), cap, out_off.data_ptr(),
                               est.data_ptr())
        e.synchronize()
    d = o.DirectoryArrays(reg, acts, owner)
    f, wst, wsilo, wact = H.route_frames_np(buf, offs, spec, d)
    wst2, wsilo2, wact2 = o.route_batch_np(f["target_grain"], spec, d, my_silo=my)[:3]
    routed = wst < H.ROUTE_ADDRESSED
    wst[routed], wsilo[routed], wact[routed] = wst2[routed], wsilo2[routed], wact2[routed]
    wperm = SQ.send_queues_loop(wsilo, wst, None, None, sh, nq, my)[2]
    want = R.encode_batch(buf, offs, wsilo, wact, wst, None, None, wperm, CFG)
    total = int(want[1][n])
    whole = out.cpu().numpy()
    assert (whole[total:] == 0xA5).all()
    _same((whole[:total].tobytes(), out_off.cpu().numpy().view(np.uint64), est.cpu().numpy()), want)
    assert {R.ENC_OK, R.ENC_COPIED, R.ENC_SKIPPED} <= set(want[2].tolist())


def test_tiled_batch(eng):
    """65,536 frames: a 4,096-frame block 16 times; identity order, so the output is the block's output tiled."""
    rng = np.random.default_rng(18)
    B, T = 4096, 16
    buf, offs, silo, act, status, placed, new_type = R.random_batch(B, rng, CFG)
    wout, woff, west = R.encode_batch(buf, offs, silo, act, status, placed, new_type, None, CFG)
    offs_t = np.concatenate([offs + np.uint64(t * len(buf)) for t in range(T)])
    tile = lambda a: np.tile(a, T)
    got = _dev(eng, buf * T, offs_t, tile(silo), tile(act), tile(status), tile(placed), tile(new_type), lead=6)
    woff_t = np.concatenate([woff[:-1] + np.uint64(t * len(wout)) for t in range(T)] + [[np.uint64(T * len(wout))]])
    _same(got, (wout * T, woff_t.astype(np.uint64), tile(west)))


def test_state_errors(gd, eng):
    with gd.GrainDispatch(device=0, table_capacity=1 << 10) as e:
        for n in (0, 3):
            with pytest.raises(gd.GrainDispatchError) as ei:
                e.encode_frames(b"\0" * 64, np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32),
                                np.zeros(n, np.uint8))
            assert ei.value.code == gd.GD_ESTATE
        with pytest.raises(gd.GrainDispatchError) as ei:
            e.encode_frames_device(0, 0, 0, 0, 0, 0, 0, None, None, None, 0, 0, 8, 0)
        assert ei.value.code == gd.GD_ESTATE
    # an order array with n = 0
    out, off, est, total = eng.encode_frames(b"", [], [], [], [], order=np.zeros(0, np.uint32), out_cap=16)
    assert total == 0 and off.tolist() == [0] and len(est) == 0
    got = _dev(eng, b"", np.zeros(0, np.uint64), [], [], [], order=np.zeros(1, np.uint32))
    assert got[0] == b"" and got[1].tolist() == [0]
    with pytest.raises(gd.GrainDispatchError) as ei:               # totals are 32-bit: the bound is refused
        eng.encode_frames_device(8, (1 << 32) - 100, 8, 2, 8, 8, 8, None, None, None, 8, 0, 8, 8)
    assert ei.value.code == gd.GD_EINVAL
