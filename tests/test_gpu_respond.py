"""GPU parity for the response writer (gd_respond_*): CreateResponseMessage /
CreateRejectionResponse + Message.Serialize for a batch, bit for bit against the reference's literal form
(_respond_ref.py): the status of every frame, out_off, and every output byte; and no byte outside the output is
written.

Every device run goes into a buffer pre-filled with 0xA5 that has 64 spare bytes: the bytes before the output and
at or past out_off[n] must still be 0xA5 (_dev)."""
import struct

import numpy as np
import pytest

import _respond_ref as R
import _sendq_ref as SQ
import headers as H

pytestmark = pytest.mark.gpu

SILO_TUPLES = [(f"10.0.0.{1 + s}", 11000 + s, 100 + 7 * s) for s in range(5)]
WIRE = [bytes(12) + bytes([10, 0, 0, 1 + s]) + struct.pack("<ii", 11000 + s, 100 + 7 * s) for s in range(5)]
TILE = 16384                                     # k_rsp_write's output bytes a workgroup (gd_frameout.h)


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


@pytest.fixture(scope="module")
def eng(gd):
    e = gd.GrainDispatch(device=0, table_capacity=1 << 12)
    e.encode_configure(SILO_TUPLES)
    e.respond_configure(R.INFOS)
    yield e
    e.close()


def _dev(e, buf, offs, kind, result=None, rej=None, info=None, body=None, body_off=None, order=None, lead=0,
         out_cap=None):
    """gd_respond_frames_device on torch buffers.  Returns (out bytes, out_off, rsp_status)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(offs)
    up = lambda a, dt, t: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt)).view(t)).to(dev)
    d_buf = torch.from_numpy(np.frombuffer(buf or b"\0", dtype=np.uint8).copy()).to(dev)
    d_off = up(offs if n else [0], np.uint64, np.int64)
    d_kind = up(kind if n else [0], np.uint8, np.uint8)
    d_res, d_rej, d_info = up(result, np.uint8, np.uint8), up(rej, np.uint8, np.uint8), up(info, np.uint32, np.int32)
    d_body = None if body is None else torch.from_numpy(np.frombuffer(body or b"\0", dtype=np.uint8).copy()).to(dev)
    d_boff, d_od = up(body_off, np.uint64, np.int64), up(order, np.uint32, np.int32)
    cap = len(buf) + (len(body) if body else 0) + n * 96 if out_cap is None else out_cap
    room = torch.full((lead + cap + 64 + 16,), 0xA5, dtype=torch.uint8, device=dev)
    base = (-room.data_ptr()) % 16 + lead                          # out pointer = 16-B boundary + lead
    d_out_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize()
    e.respond_frames_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n, d_kind.data_ptr(), ptr(d_res), ptr(d_rej),
                            ptr(d_info), ptr(d_body), ptr(d_boff), ptr(d_od), room.data_ptr() + base, cap,
                            d_out_off.data_ptr(), d_st.data_ptr())
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
        err.out_off = out_off
        raise err
    return whole[base:base + total].tobytes(), out_off, d_st.cpu().numpy()[:n]


def _same(got, want):
    out, off, st = got[:3]
    wout, woff, wst = want
    np.testing.assert_array_equal(st, wst, err_msg="rsp_status")
    np.testing.assert_array_equal(off, woff, err_msg="out_off")
    if out != wout:
        a, b = np.frombuffer(out, np.uint8), np.frombuffer(wout, np.uint8)
        k = int(np.flatnonzero(a != b)[0])
        j = int(np.searchsorted(woff, k, side="right")) - 1
        raise AssertionError(f"first differing byte {k} (output frame {j}, byte {k - int(woff[j])} of it): "
                             f"{a[k]:#x} != {b[k]:#x}")


def _check(e, batch, order=None, lead=0):
    want = R.respond_batch(*batch, order, R.INFOS)
    _same(_dev(e, *batch, order=order, lead=lead), want)
    return want


def _frames(frames, pad=b""):
    buf, offs = pad, []
    for f in frames:
        offs.append(len(buf))
        buf += f
    return buf, np.array(offs, dtype=np.uint64)


def _plain(frames, pad=b"", kind=R.RSP_REJECTION, info=2, rej=1, bodies=None):
    """A batch of the given frames, every one answered alike."""
    buf, offs = _frames(frames, pad)
    n = len(offs)
    bodies = bodies or [b""] * n
    boff = np.zeros(n + 1, np.uint64)
    boff[1:] = np.cumsum([len(b) for b in bodies])
    return (buf, offs, np.full(n, kind, np.uint8), np.zeros(n, np.uint8), np.full(n, rej, np.uint8),
            np.full(n, info, np.uint32), b"".join(bodies), boff)


K = (7, 8, 0x0300000000000011)
K2 = (1, 2, 0x0300000000000022)
BASE = {"category": 2, "direction": 0, "correlation_id": 99, "target_grain": (K, None), "target_silo": R.SILO2,
        "target_activation": ((5, 6, 0), None), "sending_grain": (K2, None), "sending_activation": ((9, 9, 0), None),
        "sending_silo": R.SILO, "resend_count": 1}


# ----------------------------------------------------------------------------- batches
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_sizes(eng, n):
    rng = np.random.default_rng(200 + n)
    batch = R.random_batch(n, rng)
    for lead in (0, 1, 7, 15):
        want = _check(eng, batch, lead=lead)
    if n >= 257:
        assert (want[2] == R.ST_OK).sum() > n // 2
    # the optional inputs absent: Success, Transient, no info, empty bodies, batch order
    buf, offs, kind = batch[:3]
    _same(_dev(eng, buf, offs, kind), R.respond_batch(buf, offs, kind, None, None, None, None, None, None, R.INFOS))


def test_mixed_and_order(eng):
    rng = np.random.default_rng(21)
    n = 3000
    batch = R.random_batch(n, rng)
    want = _check(eng, batch)
    assert set(np.unique(want[2]).tolist()) == {0, 1, 2, 3, 4}
    assert set(np.unique(batch[2]).tolist()) >= {0, 1, 2}
    _check(eng, batch, order=rng.permutation(n).astype(np.uint32), lead=5)


def test_large_body_straddles_tiles(eng):
    rng = np.random.default_rng(22)
    frames = [H.encode_frame(dict(BASE, correlation_id=k), b"q" * (k % 7)) for k in range(130)]
    bodies = [bytes(rng.integers(0, 256, size=k % 50, dtype=np.uint8)) for k in range(130)]
    bodies[64] = bytes(rng.integers(0, 256, size=300000, dtype=np.uint8))
    for lead, pad in ((0, b""), (9, b"\x01\x02\x03")):
        want = _check(eng, _plain(frames, pad, bodies=bodies), lead=lead)
        assert (want[2] == R.ST_OK).all() and len(want[0]) > 300000 + TILE    # the body alone spans 18 tiles


def test_tile_edges(eng):
    """An output of exactly one 16-KiB tile and of one tile plus one byte; a frame edge and a body's first byte (a
    run edge inside a frame) on the tile boundary."""
    rng = np.random.default_rng(24)
    frames = [H.encode_frame(dict(BASE, correlation_id=k), b"") for k in range(40)]
    n = len(frames)
    empty = _plain(frames)
    w0 = R.respond_batch(*empty, None, R.INFOS)
    flen = int(w0[1][1])                                              # every answer has the same length
    assert (w0[2] == R.ST_OK).all() and len(w0[0]) == n * flen < TILE
    for total, split in ((TILE, 0), (TILE + 1, 0), (None, 1), (None, 2)):
        lens = [0] * n
        if split == 0:
            lens[5] = total - n * flen                                # one body brings the total to `total`
        elif split == 1:
            lens[5], lens[30] = TILE - 20 * flen, 40                  # frame 20 starts on the tile boundary
        else:
            lens[5], lens[20] = TILE - 21 * flen, 40                  # frame 20's body starts on the tile boundary
        total = n * flen + sum(lens)
        bodies = [bytes(rng.integers(0, 256, size=k, dtype=np.uint8)) for k in lens]
        b = empty[:6] + (b"".join(bodies), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
        for lead in (0, 9):
            want = _check(eng, b, lead=lead)
            assert len(want[0]) == total
            if split == 1:
                assert int(want[1][20]) == TILE
            if split == 2:
                assert int(want[1][21]) - lens[20] == TILE


def test_skipped_run_longer_than_the_lds_offsets(eng):
    frames = [H.encode_frame(dict(BASE, correlation_id=k), b"") for k in range(1502)]
    batch = list(_plain(frames, bodies=[b"b" * (k % 5) for k in range(1502)]))
    batch[2][1:1501] = R.RSP_NONE                                  # 1,500 zero-length frames inside one tile
    want = _check(eng, tuple(batch))
    assert (want[2][1:1501] == R.ST_SKIPPED).all() and want[2][0] == want[2][1501] == R.ST_OK
    batch[2][:] = R.RSP_NONE                                       # all skipped: total 0, nothing written
    want = _check(eng, tuple(batch))
    assert want[0] == b""


def test_run_edges_at_every_offset(eng):
    """DebugContext and KeyExt lengths 0..17 move every later run edge through every offset mod 16."""
    frames = []
    for d in range(18):
        for x in range(18):
            ext = "e" * x
            h = dict(BASE, debug_context="D" * d, target_grain=(K, ext), sending_grain=(K2, ext[::2]),
                     target_activation=((5, 6, 0), ext[:x // 3]), read_only=True, always_interleave=bool(x & 1),
                     time_to_live=1 << 33)
            if d % 3 == 0:
                h["transaction_info"] = b"t" * (d + x)
            frames.append(H.encode_frame(h, b"in"))
    bodies = [b"B" * ((3 * k) % 23) for k in range(len(frames))]
    for lead, pad, kind in ((0, b"", R.RSP_REJECTION), (3, b"\x00", R.RSP_RESPONSE), (14, b"\x00\x00", R.RSP_REJECTION)):
        want = _check(eng, _plain(frames, pad, kind=kind, info=3, bodies=bodies), lead=lead)
        assert (want[2] == R.ST_OK).all()


def test_long_headers_past_the_window(eng):
    frames = [H.encode_frame(dict(BASE, debug_context="d" * 300), b"bb"),
              H.encode_frame(dict(BASE, debug_context="D" * 5000, generic_grain_type="G" * 100), b"c"),
              H.encode_frame(dict(BASE, sending_grain=(K2, "s" * 400), target_activation=((1, 1, 1), "x" * 333))),
              H.encode_frame(dict(BASE, debug_context="e" * 170), b"dddd")]     # the window ends inside the walk
    for pad in (b"", b"\x01", b"\x01\x02\x03"):
        want = _check(eng, _plain(frames * 3, pad, bodies=[b"xyz"] * 12))
        assert (want[2] == R.ST_OK).all()


def test_capacity(eng, gd):
    rng = np.random.default_rng(23)
    batch = R.random_batch(300, rng)
    want = R.respond_batch(*batch, None, R.INFOS)
    total = len(want[0])
    with pytest.raises(gd.GrainDispatchError) as ei:               # at the next synchronisation: out_off complete,
        _dev(eng, *batch, out_cap=total - 1)                       # nothing written (_dev)
    assert ei.value.code == gd.GD_EFULL
    np.testing.assert_array_equal(ei.value.out_off, want[1])
    out = np.full(total - 1, 0xA5, np.uint8)
    with pytest.raises(gd.GrainDispatchError) as ei:
        eng.respond_frames(*batch, out=out)
    assert ei.value.code == gd.GD_EFULL and (out == 0xA5).all()
    _same(_dev(eng, *batch, out_cap=total), want)                  # exactly enough; the handle still works


def test_kinds_every_pair(eng):
    import torch
    turn, recv = [a.ravel().astype(np.uint8) for a in np.meshgrid(np.arange(12), np.arange(9), indexing="ij")]
    for rs in (recv, None):
        wk, wr = R.kinds_from_turns(turn, rs)
        k, r = eng.respond_kinds(turn, rs)
        np.testing.assert_array_equal(k, wk)
        np.testing.assert_array_equal(r, wr)
        d = lambda a: torch.from_numpy(a).cuda()
        dt, dk, dr = d(turn), torch.full((len(turn),), 9, dtype=torch.uint8).cuda(), torch.full((len(turn),), 9, dtype=torch.uint8).cuda()
        drs = None if rs is None else d(rs)
        eng.respond_kinds_device(dt.data_ptr(), None if drs is None else drs.data_ptr(), len(turn), dk.data_ptr(),
                                 dr.data_ptr())
        eng.synchronize()
        np.testing.assert_array_equal(dk.cpu().numpy(), wk)
        np.testing.assert_array_equal(dr.cpu().numpy(), wr)
    assert set(wk.tolist()) == {0, 2}


@pytest.mark.parametrize("n_silos", [1, 5, 300])
def test_silo_index(gd, n_silos):
    import torch
    rng = np.random.default_rng(24 + n_silos)
    tuples = [(f"10.{s >> 8}.{s & 255}.7", 11000 + s % 3, 5 + s // 7) for s in range(n_silos)]
    if n_silos > 4:
        tuples[4] = tuples[1]                                      # a repeated address: the lowest index
    table = [bytes(gd.silo_addr(*t).ip) + struct.pack("<ii", t[1], t[2]) for t in tuples]
    pick = rng.integers(0, n_silos, size=700)
    wire = np.frombuffer(b"".join(table[int(s)] for s in pick), np.uint8).reshape(-1, 24).copy()
    wire[::7, 16] ^= 1                                             # port changed: absent
    wire[3::11, 23] ^= 0x80                                        # generation changed: absent
    wire[5::13] = 0                                                # all zero
    want = R.silo_index(wire, table)
    assert (want == R.NO_SILO).any() and (want != R.NO_SILO).any()
    with gd.GrainDispatch(device=0, table_capacity=1 << 10) as e:
        with pytest.raises(gd.GrainDispatchError) as ei:
            e.silo_index(wire)
        assert ei.value.code == gd.GD_ESTATE
        e.encode_configure(tuples)
        np.testing.assert_array_equal(e.silo_index(wire), want)
        d_w = torch.from_numpy(wire).cuda()
        d_s = torch.full((len(wire),), 77, dtype=torch.int32).cuda()
        e.silo_index_device(d_w.data_ptr(), len(wire), d_s.data_ptr())
        e.synchronize()
        np.testing.assert_array_equal(d_s.cpu().numpy().view(np.uint32), want)


def test_host_forms_agree(eng):
    rng = np.random.default_rng(25)
    batch = R.random_batch(500, rng)
    order = rng.permutation(500).astype(np.uint32)
    want = R.respond_batch(*batch, order, R.INFOS)
    got = _dev(eng, *batch, order=order)
    out = np.full(len(want[0]) + 64, 0xA5, np.uint8)
    o2, off, st, total = eng.respond_frames(*batch, order=order, out=out)
    assert o2 is out and total == len(want[0]) and (out[total:] == 0xA5).all()
    _same((out[:total].tobytes(), off, st), want)
    _same(got, (out[:total].tobytes(), off, st))
    buf, offs, kind = batch[:3]                                    # every optional input absent
    o3, off3, st3, t3 = eng.respond_frames(buf, offs, kind)
    _same((o3[:t3].tobytes(), off3, st3), R.respond_batch(buf, offs, kind, None, None, None, None, None, None, R.INFOS))


def test_chain_to_sender_queues(gd):
    """decode -> silo_index -> send_queues -> respond_frames(order = perm) on one handle, nothing read back in
    between: each queue's byte run is the concatenation of the reference's answers for that queue."""
    import torch
    rng = np.random.default_rng(26)
    n, nq = 2000, 5
    batch = list(R.random_batch(n, rng))
    buf, offs = batch[0], batch[1]
    batch[2] = rng.choice([R.RSP_RESPONSE, R.RSP_REJECTION], size=n).astype(np.uint8)
    # the senders: R.SILO = 10.0.0.1:11111 gen 7, R.SILO2 = 10.0.0.9:22222 gen 3, and three others
    tuples = [("10.0.0.1", 11111, 7), ("10.0.0.2", 1, 1), ("10.0.0.9", 22222, 3), ("10.0.0.3", 1, 1), ("10.0.0.4", 1, 1)]
    sh = SQ.hashes_with_edges(rng, len(tuples))
    dev = torch.device("cuda:0")
    with gd.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=1) as e:
        e.encode_configure(tuples)
        e.respond_configure(R.INFOS)
        e.send_configure(sh, nq)
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(dev)
        d_buf = up(np.frombuffer(buf, np.uint8).copy(), np.uint8)
        d_off = up(offs, np.int64)
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
        flags, tg = i32(n), torch.empty((n, 3), dtype=torch.int64, device=dev)
        ss = torch.empty((n, 24), dtype=torch.uint8, device=dev)
        silo, perm, qoff = i32(n), i32(n), i32(nq + 5)
        sst = torch.empty(n, dtype=torch.uint8, device=dev)
        d_kind, d_res, d_rej = up(batch[2], np.uint8), up(batch[3], np.uint8), up(batch[4], np.uint8)
        d_info, d_boff = up(batch[5], np.int32), up(batch[7], np.int64)
        d_body = up(np.frombuffer(batch[6], np.uint8).copy(), np.uint8)
        cap = len(buf) + len(batch[6]) + 96 * n
        out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=dev)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        e.decode_frames_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n,
                               {"flags": flags.data_ptr(), "target_grain": tg.data_ptr(), "sending_silo": ss.data_ptr()})
        e.silo_index_device(ss.data_ptr(), n, silo.data_ptr())
        e.send_queues_device(silo.data_ptr(), None, None, None, n, sst.data_ptr(), None, perm.data_ptr(),
                             qoff.data_ptr())
        e.respond_frames_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n, d_kind.data_ptr(), d_res.data_ptr(),
                                d_rej.data_ptr(), d_info.data_ptr(), d_body.data_ptr(), d_boff.data_ptr(),
                                perm.data_ptr(), out.data_ptr(), cap, out_off.data_ptr(), st.data_ptr())
        e.synchronize()
        table = [bytes(gd.silo_addr(*t).ip) + struct.pack("<ii", t[1], t[2]) for t in tuples]
    wsilo = R.silo_index(H.decode_frames(buf, offs)["sending_silo"], table)
    np.testing.assert_array_equal(silo.cpu().numpy().view(np.uint32), wsilo)
    assert {0, 2, R.NO_SILO} <= set(wsilo.tolist())
    wperm, wqoff = SQ.send_queues_loop(wsilo, None, None, None, sh, nq, 1)[2:4]
    perm_h, qoff_h = perm.cpu().numpy().view(np.uint32), qoff.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(perm_h, wperm)
    want = R.respond_batch(*batch, wperm, R.INFOS)
    total = int(want[1][n])
    whole = out.cpu().numpy()
    assert (whole[total:] == 0xA5).all()
    got = (whole[:total].tobytes(), out_off.cpu().numpy().view(np.uint64), st.cpu().numpy())
    _same(got, want)
    single = R.respond_batch(*batch, None, R.INFOS)
    fr = lambda i: single[0][int(single[1][i]):int(single[1][i + 1])]
    for b in range(len(qoff_h) - 1):
        members = perm_h[qoff_h[b]:qoff_h[b + 1]]
        run = got[0][int(got[1][qoff_h[b]]):int(got[1][qoff_h[b + 1]])]
        assert run == b"".join(fr(int(i)) for i in members)


def test_state_errors(gd, eng):
    with gd.GrainDispatch(device=0, table_capacity=1 << 10) as e:
        for n in (0, 3):
            with pytest.raises(gd.GrainDispatchError) as ei:
                e.respond_frames(b"\0" * 64, np.zeros(n, np.uint64), np.zeros(n, np.uint8))
            assert ei.value.code == gd.GD_ESTATE
        with pytest.raises(gd.GrainDispatchError) as ei:
            e.respond_frames_device(0, 0, 0, 0, 0, None, None, None, None, None, None, 0, 0, 8, 0)
        assert ei.value.code == gd.GD_ESTATE
        e.respond_configure([])                                    # no strings: every info index names none
        fr = H.encode_frame(BASE, b"")
        out, off, st, total = e.respond_frames(fr, [0], [R.RSP_REJECTION], info=[0])
        assert (st[0], out[:total].tobytes()) == R.respond_splice(fr, 0, R.RSP_REJECTION, 0, 0, 0, b"", [])
    out, off, st, total = eng.respond_frames(b"", [], [], order=np.zeros(0, np.uint32), out_cap=16)
    assert total == 0 and off.tolist() == [0] and len(st) == 0
    with pytest.raises(gd.GrainDispatchError) as ei:               # totals are 32-bit: the bound is refused
        eng.respond_frames_device(8, (1 << 32) - 100, 8, 2, 8, None, None, None, None, None, None, 8, 0, 8, 8)
    assert ei.value.code == gd.GD_EINVAL
