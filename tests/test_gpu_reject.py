"""GPU parity for the forward rejections (gd_forward_reject_frames*): TryForwardRequest's failure arm +
RejectMessage + CreateRejectionResponse + Message.Serialize for a batch, bit for bit against the reference form
(_reject_ref.py): the status of every frame, out_off and every output byte; and no byte outside the output is
written.

Every device run goes into a buffer pre-filled with 0xA5 that has 64 spare bytes: the bytes before the output and
at or past out_off[n] must still be 0xA5 (_dev).  The source buffer holds exactly the frames."""
import struct

import numpy as np
import pytest

import _cih_ref as C
import _forward_ref as F
import _reject_ref as J
import _respond_ref as R
import _sendq_ref as SQ
import headers as H

pytestmark = pytest.mark.gpu

TILE = 16384                                     # k_rej_write's output bytes a workgroup (gd_frameout.h)


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


@pytest.fixture(scope="module")
def cfg():
    return F.make_config(np.random.default_rng(9))


@pytest.fixture(scope="module")
def eng(gd, cfg):
    e = gd.GrainDispatch(device=0, table_capacity=1 << 12)
    e.set_option(gd.OPT_WALK_INVALIDATION, 1)   # for the responder, the sniff stage and the decoder: this stage walks anyway
    e.encode_configure(F.SILO_TUPLES, F.TYPE_NAMES)
    e.activation_ids_set(np.arange(len(cfg.act_ids)), cfg.act_ids)
    e.respond_configure(J.INFOS)
    yield e
    e.close()


def _up(a, dt):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a, dtype=dt))
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _dev(e, buf, offs, kind, old_act=None, info=None, body=None, body_off=None, order=None, lead=0, out_cap=None,
         max_fc=F.MAX_FC, local=F.LOCAL_SILO, keep=None):
    """gd_forward_reject_frames_device on torch buffers.  Returns (out bytes, out_off, rej_status); keep (a dict)
    receives the device tensors of the source and the output."""
    import torch
    n = len(offs)
    d_buf = _up(np.frombuffer(buf or b"\0", dtype=np.uint8), np.uint8)
    d_off, d_kind = _up(offs if n else [0], np.uint64), _up(kind if n else [0], np.uint8)
    d_old, d_info, d_od = _up(old_act, np.uint32), _up(info, np.uint32), _up(order, np.uint32)
    has_body = body is not None and body_off is not None
    d_body = _up(np.frombuffer(body or b"\0", dtype=np.uint8), np.uint8) if has_body else None
    d_boff = _up(body_off, np.uint64) if has_body else None
    nbody = int(body_off[-1]) if has_body and len(body_off) else 0
    cap = 2 * len(buf) + nbody + n * 160 if out_cap is None else out_cap
    room = torch.full((lead + cap + 64 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    base = (-room.data_ptr()) % 16 + lead                          # out pointer = 16-B boundary + lead
    d_out_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    db = {"buf": d_buf.data_ptr(), "buf_len": len(buf), "frame_off": d_off.data_ptr(), "kind": d_kind.data_ptr(),
          "old_act": ptr(d_old), "max_forward_count": max_fc, "local_silo": local}
    torch.cuda.synchronize()
    e.forward_reject_frames_device(db, n, ptr(d_info), ptr(d_body), ptr(d_boff), ptr(d_od), room.data_ptr() + base,
                                   cap, d_out_off.data_ptr(), d_st.data_ptr())
    err = None
    try:
        e.synchronize()
    except Exception as ex:                                        # GD_EFULL surfaces here; the caller checks
        err = ex
    whole = room.cpu().numpy()
    out_off = d_out_off.cpu().numpy().view(np.uint64)
    total = int(out_off[n])
    assert (whole[:base] == 0xA5).all(), "bytes before the output were written"
    written = base + (total if err is None else 0)
    assert (whole[written:] == 0xA5).all(), "bytes at or past out_off[n] were written"
    if err is not None:
        err.out_off = out_off
        raise err
    if keep is not None:
        keep.update(room=room, base=base, d_out_off=d_out_off)
    return whole[base:base + total].tobytes(), out_off, d_st.cpu().numpy()[:n]


def _same(got, want):
    out, off, st = got[:3]
    wout, woff, wst = want[:3]
    np.testing.assert_array_equal(st, wst, err_msg="rej_status")
    np.testing.assert_array_equal(off, woff, err_msg="out_off")
    if out != wout:
        a, b = np.frombuffer(out, np.uint8), np.frombuffer(wout, np.uint8)
        k = int(np.flatnonzero(a != b)[0])
        j = int(np.searchsorted(woff, k, side="right")) - 1
        raise AssertionError(f"first differing byte {k} (output frame {j}, byte {k - int(woff[j])} of it): "
                             f"{a[k]:#x} != {b[k]:#x}")


def _check(e, cfg, batch, order=None, lead=0, max_fc=F.MAX_FC, local=F.LOCAL_SILO):
    """batch = (buf, offs, kind, old_act, info, body, body_off)."""
    want = J.reject_batch(*batch, order, max_fc, local, cfg)
    _same(_dev(e, *batch, order=order, lead=lead, max_fc=max_fc, local=local), want)
    return want


def _good_acts(cfg, n, rng):
    good = np.flatnonzero(cfg.act_ids.any(axis=1))
    return rng.choice(good, size=n).astype(np.uint32)


def _plain(cfg, frames, rng, pad=b"", bodies=None):
    """A batch of the given frames, every one FORWARD with an old address and info 0."""
    buf, offs = F.pack_frames(frames, pad)
    n = len(offs)
    body = body_off = None
    if bodies is not None:
        body_off = np.zeros(n + 1, np.uint64)
        body_off[1:] = np.cumsum([len(b) for b in bodies])
        body = b"".join(bodies)
    return (buf, offs, np.full(n, F.FWD_FORWARD, np.uint8), _good_acts(cfg, n, rng), np.zeros(n, np.uint32), body,
            body_off)


K = (7, 8, 0x0300000000000011)
BASE = {"category": 2, "direction": 0, "correlation_id": 99, "forward_count": 2, "target_grain": (K, None),
        "target_silo": F.SILOS[1], "target_activation": ((5, 6, 0), None),
        "sending_grain": ((1, 2, 0x0300000000000022), None), "sending_silo": F.SILOS[0], "time_to_live": 1 << 33}


# ----------------------------------------------------------------------------- batches
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(eng, cfg, n):
    """Mixed frames: old entry counts 0-3, field absent and with count 0, KeyExt strings in entries and TargetGrain,
    ForwardCount absent, below, at and above max_forward_count 0, 1 and 2; source frames at all four alignments."""
    rng = np.random.default_rng(500 + n)
    for k, (lead, max_fc) in enumerate(((0, 2), (1, 1), (7, 0), (15, 2))):
        batch = J.random_batch(n, rng, cfg, max_fc, pad=bytes(k))
        _check(eng, cfg, batch, lead=lead, max_fc=max_fc)
    # the optional inputs absent: no old address, no info, no bodies, batch order
    buf, offs, kind = batch[:3]
    _check(eng, cfg, (buf, offs, kind, None, None, None, None))
    _check(eng, cfg, batch[:5] + (None, None), order=rng.permutation(n).astype(np.uint32), lead=3)


def _fwd_status(e, buf, offs, kind, old_act, max_fc, local):
    """gd_forward_frames_device's statuses for the same batch."""
    import torch
    n = len(offs)
    t = [_up(np.frombuffer(buf, np.uint8), np.uint8), _up(offs, np.uint64), _up(kind, np.uint8), _up(old_act, np.uint32)]
    cap = 2 * len(buf) + n * 256
    d_out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    db = {"buf": t[0].data_ptr(), "buf_len": len(buf), "frame_off": t[1].data_ptr(), "kind": t[2].data_ptr(),
          "old_act": t[3].data_ptr(), "max_forward_count": max_fc, "local_silo": local}
    e.forward_frames_device(db, n, None, None, None, None, None, None, d_out.data_ptr(), cap, d_off.data_ptr(),
                            d_st.data_ptr(), None)
    e.synchronize()
    return d_st.cpu().numpy()


def test_every_status_and_the_partition(eng, cfg):
    """Every status is reached; DISCARDED + NO_SILO + NO_ID + OK are exactly the forward writer's REJECT frames on
    the same batch, and the SKIPPED, MALFORMED and FALLBACK sets are its own."""
    rng = np.random.default_rng(51)
    n = 900
    batch = J.random_batch(n, rng, cfg)
    buf, offs, kind, old_act = batch[:4]
    seen = set()
    for local, max_fc in ((F.LOCAL_SILO, 2), (9, 2), (F.LOCAL_SILO, 1)):
        st = _check(eng, cfg, batch, max_fc=max_fc, local=local)[2]
        fst = _fwd_status(eng, buf, offs, kind, old_act, max_fc, local)
        np.testing.assert_array_equal(np.isin(st, J.FWD_REJECT_SET), fst == F.ST_REJECT)
        for mine, theirs in ((J.ST_SKIPPED, F.ST_SKIPPED), (J.ST_MALFORMED, F.ST_MALFORMED), (J.ST_FALLBACK, F.ST_FALLBACK)):
            np.testing.assert_array_equal(st == mine, fst == theirs)
        seen |= set(np.unique(st).tolist())
    assert seen == set(range(8))
    want = J.reject_batch(*batch, None, 2, F.LOCAL_SILO, cfg)
    assert len(want[0]) > 2 * TILE and (want[2] == J.ST_OK).sum() > n // 5       # frames straddle the tile edges


def test_without_an_old_address_it_is_the_responder(eng, cfg):
    """old_act NULL and old_act GD_NO_ACTIVATION: the bytes equal gd_respond_frames_device's under
    GD_OPT_WALK_INVALIDATION 1 (kind REJECTION, type 0, same info and body) for every frame both mark OK; the
    default-Category + DebugContext frame is OK here and is checked against the reference form."""
    import torch
    rng = np.random.default_rng(52)
    n = 300
    buf, offs, kind, _, info, body, body_off = J.random_batch(n, rng, cfg, max_fc=0)
    kind[:] = F.FWD_FORWARD
    for old in (None, np.full(n, J.NONE32, np.uint32)):
        got = _dev(eng, buf, offs, kind, old, info, body, body_off, max_fc=0)
        _same(got, J.reject_batch(buf, offs, kind, old, info, body, body_off, None, 0, F.LOCAL_SILO, cfg))
    t = [_up(np.frombuffer(buf, np.uint8), np.uint8), _up(offs, np.uint64), _up(np.full(n, R.RSP_REJECTION), np.uint8),
         _up(info, np.uint32), _up(np.frombuffer(body, np.uint8), np.uint8), _up(body_off, np.uint64)]
    cap = len(buf) + len(body) + n * 96
    d_out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    eng.respond_frames_device(t[0].data_ptr(), len(buf), t[1].data_ptr(), n, t[2].data_ptr(), None, None, t[3].data_ptr(),
                              t[4].data_ptr(), t[5].data_ptr(), None, d_out.data_ptr(), cap, d_off.data_ptr(),
                              d_st.data_ptr())
    eng.synchronize()
    rout, roff, rst = d_out.cpu().numpy().tobytes(), d_off.cpu().numpy().view(np.uint64), d_st.cpu().numpy()
    out, off, st = got
    both = split = 0
    for i in range(n):
        mine = out[int(off[i]):int(off[i + 1])]
        if st[i] == J.ST_OK:
            assert rst[i] in (R.ST_OK, R.ST_FALLBACK)
        if rst[i] == R.ST_OK:
            assert st[i] in (J.ST_OK, J.ST_MAY_FORWARD, J.ST_FALLBACK)
        if rst[i] == R.ST_OK and st[i] == J.ST_OK:
            assert mine == rout[int(roff[i]):int(roff[i + 1])], i
            both += 1
        elif rst[i] == R.ST_FALLBACK and st[i] == J.ST_OK:
            split += 1
    assert both > n // 3 and split >= 1


# ----------------------------------------------------------------------------- window, alignment, tiles
@pytest.mark.parametrize("align", [0, 1, 2, 3])
def test_window_edges(eng, cfg, align):
    """The last old entry's end, TargetGrain's first and TargetGrain's last byte on bytes 191, 192 and 193 of the
    frame (either side of the staged window), at every source alignment and every out_buf lead 0-15."""
    rng = np.random.default_rng(53 + align)
    buf, offs, what = C.edge_frames(rng, align)
    n = len(offs)
    assert {w[:2] for w in what} == {(t, b) for t in ("entry_end", "tg_first", "tg_last") for b in (191, 192, 193)}
    batch = (buf, offs, np.ones(n, np.uint8), _good_acts(cfg, n, rng), rng.integers(0, 4, size=n).astype(np.uint32),
             None, None)
    want = J.reject_batch(*batch, None, 0, F.LOCAL_SILO, cfg)      # the reference once, every lead against it
    assert (want[2] == J.ST_OK).all()
    for lead in range(16):
        _same(_dev(eng, *batch, lead=lead, max_fc=0), want)


def test_run_edges_at_every_offset(eng, cfg):
    """DebugContext, KeyExt and info lengths move every later run edge through every offset mod 16."""
    rng = np.random.default_rng(57)
    frames = []
    for d in range(0, 18):
        for x in range(0, 18, 2):
            h = dict(BASE, debug_context="D" * d, target_grain=((3, 4, 0x0600000000000007), "e" * x), read_only=True)
            if d % 3 == 0:
                h["transaction_info"] = b"t" * (d + x)
            if d % 4 == 0:
                h["cache_invalidation"] = F.w_invalidation(F.rand_entries(rng, 1 + d // 8))
            if d % 5 == 0:
                del h["time_to_live"]
            frames.append(H.encode_frame(h, b"B" * 5))
    n = len(frames)
    bodies = [b"Q" * ((3 * k) % 23) for k in range(n)]
    for lead, pad in ((0, b""), (3, b"\x00"), (14, b"\x00\x00")):
        b = list(_plain(cfg, frames, rng, pad, bodies))
        b[4] = rng.integers(0, 5, size=n).astype(np.uint32)
        assert (_check(eng, cfg, tuple(b), lead=lead)[2] == J.ST_OK).all()


def test_tile_edges(eng, cfg):
    """An output of exactly one 16-KiB tile and of one tile plus one byte; a frame edge and a body's first byte (a
    run edge inside a frame) on the tile boundary."""
    rng = np.random.default_rng(58)
    frames = [H.encode_frame(dict(BASE, correlation_id=k), b"") for k in range(40)]
    n = len(frames)
    empty = _plain(cfg, frames, rng, bodies=[b""] * n)
    w0 = J.reject_batch(*empty, None, F.MAX_FC, F.LOCAL_SILO, cfg)
    flen = int(w0[1][1])                                              # every answer has the same length
    assert len(w0[0]) == n * flen < TILE
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
        b = empty[:5] + (b"".join(bodies), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
        for lead in (0, 9):
            want = _check(eng, cfg, b, lead=lead)
            assert len(want[0]) == total
            if split == 1:
                assert int(want[1][20]) == TILE
            if split == 2:
                assert int(want[1][21]) - lens[20] == TILE


def test_more_frame_starts_in_a_tile_than_the_lds_offsets(eng, cfg):
    rng = np.random.default_rng(59)
    frames = [H.encode_frame(dict(BASE, correlation_id=k), b"") for k in range(1502)]
    batch = list(_plain(cfg, frames, rng))
    batch[2][1:1501] = F.FWD_NONE                                  # 1,500 zero-length frames inside one tile
    want = _check(eng, cfg, tuple(batch))
    assert (want[2][1:1501] == J.ST_SKIPPED).all() and want[2][0] == want[2][1501] == J.ST_OK
    batch[2][:] = F.FWD_NONE                                       # all skipped: total 0, nothing written
    assert _check(eng, cfg, tuple(batch))[0] == b""


# ----------------------------------------------------------------------------- order, capacity, arguments
def test_order_is_a_send_queues_perm(gd, cfg):
    """gd_silo_index on the decoder's sending_silo, gd_send_queues, its perm as `order`: each queue's rejections
    are one contiguous run."""
    rng = np.random.default_rng(60)
    nq = 4
    with gd.GrainDispatch(device=0, table_capacity=1 << 12) as e:
        e.set_option(gd.OPT_WALK_INVALIDATION, 1)
        e.encode_configure(F.SILO_TUPLES, F.TYPE_NAMES)
        e.activation_ids_set(np.arange(len(cfg.act_ids)), cfg.act_ids)
        e.respond_configure(J.INFOS)
        e.send_configure(SQ.hashes_with_edges(rng, len(F.SILO_TUPLES)), nq)
        n = 400
        batch = J.random_batch(n, rng, cfg)
        buf, offs = batch[:2]
        fields, _ = e.decode_frames_turn(buf, offs, fields=("flags", "target_grain", "sending_silo"))
        silo = e.silo_index(fields["sending_silo"])
        _, _, perm, qoff = e.send_queues(silo)
        want = J.reject_batch(*batch, perm, F.MAX_FC, F.LOCAL_SILO, cfg)
        _same(_dev(e, *batch, order=perm, lead=5), want)
        single = J.reject_batch(*batch, None, F.MAX_FC, F.LOCAL_SILO, cfg)
        fr_of = lambda i: single[0][int(single[1][i]):int(single[1][i + 1])]
        busy = 0
        for b in range(len(qoff) - 1):
            run = want[0][int(want[1][qoff[b]]):int(want[1][qoff[b + 1]])]
            assert run == b"".join(fr_of(int(i)) for i in perm[qoff[b]:qoff[b + 1]])
            busy += bool(run)
        assert busy >= 3 and sorted(perm.tolist()) == list(range(n))


def _hb(batch, max_fc=F.MAX_FC, local=F.LOCAL_SILO):
    return {"buf": batch[0], "offsets": batch[1], "kind": batch[2], "old_act": batch[3], "max_forward_count": max_fc,
            "local_silo": local}


def test_capacity(eng, cfg, gd):
    rng = np.random.default_rng(61)
    batch = J.random_batch(300, rng, cfg)
    want = J.reject_batch(*batch, None, F.MAX_FC, F.LOCAL_SILO, cfg)
    total = len(want[0])
    with pytest.raises(gd.GrainDispatchError) as ei:               # at the next synchronisation: out_off complete,
        _dev(eng, *batch, out_cap=total - 1)                       # nothing written (_dev's canary)
    assert ei.value.code == gd.GD_EFULL
    np.testing.assert_array_equal(ei.value.out_off, want[1])
    out = np.full(total - 1, 0xA5, np.uint8)
    with pytest.raises(gd.GrainDispatchError) as ei:
        eng.forward_reject_frames(_hb(batch), *batch[4:7], out=out)
    assert ei.value.code == gd.GD_EFULL and (out == 0xA5).all()
    _same(_dev(eng, *batch, out_cap=total), want)                  # exactly enough; the handle still works


def test_host_form_equals_the_device_form(eng, cfg):
    rng = np.random.default_rng(62)
    n = 500
    batch = J.random_batch(n, rng, cfg)
    order = rng.permutation(n).astype(np.uint32)
    want = J.reject_batch(*batch, order, F.MAX_FC, F.LOCAL_SILO, cfg)
    got = _dev(eng, *batch, order=order)
    out = np.full(len(want[0]) + 64, 0xA5, np.uint8)
    o2, off, st, total = eng.forward_reject_frames(_hb(batch), *batch[4:7], order=order, out=out)
    assert o2 is out and total == len(want[0]) and (out[total:] == 0xA5).all()
    _same((out[:total].tobytes(), off, st), want)
    _same(got, (out[:total].tobytes(), off, st))
    buf, offs, kind = batch[:3]                                    # every optional input absent
    o3, off3, st3, t3 = eng.forward_reject_frames({"buf": buf, "offsets": offs, "kind": kind})
    _same((o3[:t3].tobytes(), off3, st3), J.reject_batch(buf, offs, kind, None, None, None, None, None, 2, 0, cfg))


def test_info_indexes(eng, cfg):
    """Indexes past the table, GD_RSP_NO_INFO and the empty string write no RejectionInfo."""
    rng = np.random.default_rng(63)
    frames = [H.encode_frame(dict(BASE, correlation_id=k), b"") for k in range(8)]
    b = list(_plain(cfg, frames, rng))
    b[4] = np.array([0, 1, 2, 3, 4, 1000, J.NO_INFO, 1], np.uint32)
    want = _check(eng, cfg, tuple(b))
    lens = np.diff(want[1].astype(np.int64))
    assert lens[1] == lens[4] == lens[5] == lens[6] == lens[7] and lens[0] == lens[1] + 4 + len(J.INFOS[0])
    for i in (1, 4, 5, 6):
        fr = want[0][int(want[1][i]):int(want[1][i + 1])]
        assert not struct.unpack_from("<I", fr, 8)[0] & H.REJECTION_INFO


def test_state_and_argument_errors(gd, eng, cfg):
    empty = {"buf": b"\0" * 64, "offsets": np.zeros(3, np.uint64), "kind": np.zeros(3, np.uint8)}
    with gd.GrainDispatch(device=0, table_capacity=1 << 10) as e:
        with pytest.raises(gd.GrainDispatchError) as ei:           # before gd_encode_configure
            e.forward_reject_frames(empty)
        assert ei.value.code == gd.GD_ESTATE
        e.encode_configure(F.SILO_TUPLES)
        with pytest.raises(gd.GrainDispatchError) as ei:           # before gd_respond_configure
            e.forward_reject_frames(empty)
        assert ei.value.code == gd.GD_ESTATE
        with pytest.raises(gd.GrainDispatchError) as ei:
            e.forward_reject_frames_device({"buf": 8, "buf_len": 64, "frame_off": 8, "kind": 8}, 0, None, None, None,
                                           None, 8, 0, 8, 8)
        assert ei.value.code == gd.GD_ESTATE
        e.respond_configure(())
        out, off, st, total = e.forward_reject_frames(empty)       # configured, no strings: all SKIPPED
        assert total == 0 and (st == J.ST_SKIPPED).all()
    out, off, st, total = eng.forward_reject_frames({"buf": b"", "offsets": [], "kind": []},
                                                    order=np.zeros(0, np.uint32), out_cap=16)
    assert total == 0 and off.tolist() == [0] and len(st) == 0     # n == 0
    assert _dev(eng, b"", np.zeros(0, np.uint64), np.zeros(0, np.uint8))[1].tolist() == [0]
    with pytest.raises(gd.GrainDispatchError) as ei:               # totals are 32-bit: the bound is refused
        eng.forward_reject_frames_device({"buf": 8, "buf_len": (1 << 31) - 100, "frame_off": 8, "kind": 8}, 2, None,
                                         None, None, None, 8, 0, 8, 8)
    assert ei.value.code == gd.GD_EINVAL
    longest = max(len(s) for s in J.INFOS)
    n_over = ((1 << 32) - 2 * 4096) // (90 + longest) + 1          # 2 * buf_len + n * (90 + longest info string) >= 2^32
    for n, code in ((n_over, gd.GD_EINVAL),):
        with pytest.raises(gd.GrainDispatchError) as ei:
            eng.forward_reject_frames_device({"buf": 8, "buf_len": 4096, "frame_off": 8, "kind": 8}, n, None, None,
                                             None, None, 8, 0, 8, 8)
        assert ei.value.code == code
    with pytest.raises(gd.GrainDispatchError) as ei:               # a NULL status array
        eng.forward_reject_frames_device({"buf": 8, "buf_len": 64, "frame_off": 8, "kind": 8}, 2, None, None, None, None,
                                         8, 0, 8, None)
    assert ei.value.code == gd.GD_EINVAL


# ----------------------------------------------------------------------------- the round trip
def test_round_trip_on_one_device_buffer(gd, eng, cfg):
    """This stage, then gd_sniff_frames_device and gd_decode_frames_turn_device on its output where it lies: the
    entries are the old ones plus the appended one, in order; Direction Response, Result Rejection,
    GD_FRAME_INVALIDATION, CorrelationId and the exchanged addresses as the reference form gives them."""
    import torch
    rng = np.random.default_rng(64)
    frames = [C.request(rng, count=c, tg_ext=x, forward_count=2, time_to_live=5, target_silo=F.SILOS[3],
                        target_activation=((4 + c if c else 9, 5, 0), None))
              for c in (None, 0, 1, 3) for x in (None, "", "ext-of-target")] * 6
    batch = _plain(cfg, frames, rng, bodies=[b"b" * (k % 7) for k in range(len(frames))])
    n = len(frames)
    keep = {}
    out, off, st = _dev(eng, *batch, lead=0, keep=keep)
    want = J.reject_batch(*batch, None, F.MAX_FC, F.LOCAL_SILO, cfg)
    _same((out, off, st), want)
    assert (st == J.ST_OK).all()
    d_buf = keep["room"][keep["base"]:]
    total = len(out)
    d_foff = keep["d_out_off"]
    # sniff
    cap = total // 80
    z = lambda nbytes: torch.zeros(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    so = {"count": z(4 * n), "ent_off": z(4 * (n + 1)), "status": z(n), "flags": z(n), "ent_frame": z(4 * cap),
          "ent_silo": z(24 * cap), "ent_grain": z(24 * cap), "ent_ext_off": z(8 * cap), "ent_ext_len": z(4 * cap),
          "ent_act_id": z(24 * cap)}
    eng.sniff_frames_device(d_buf.data_ptr(), total, d_foff.data_ptr(), n, {k: v.data_ptr() for k, v in so.items()}, cap)
    eng.synchronize()
    dn = lambda k, dt, cnt: so[k].cpu().numpy()[:cnt * np.dtype(dt).itemsize].view(dt)
    ent_off = dn("ent_off", np.uint32, n + 1)
    m = int(ent_off[n])
    assert (dn("status", np.uint8, n) == gd.GD_SNIFF_OK).all()
    e_silo = dn("ent_silo", np.uint8, 24 * m).reshape(m, 24)
    e_grain, e_act = dn("ent_grain", np.uint64, 3 * m).reshape(m, 3), dn("ent_act_id", np.uint64, 3 * m).reshape(m, 3)
    e_xlen = dn("ent_ext_len", np.int32, m)
    for i in range(n):
        req = F.parse_fields(frames[i], struct.unpack_from("<i", frames[i], 0)[0])[0]
        ents = list(req.get("invalidation", [])) + [(H.w_silo(*F.SILOS[F.LOCAL_SILO]), req["target_grain"],
                                                     (cfg.act_id(int(batch[3][i])), None))]
        assert int(ent_off[i + 1]) - int(ent_off[i]) == len(ents)
        for k, (s, g, a) in enumerate(ents):
            e = int(ent_off[i]) + k
            assert e_silo[e].tobytes() == s and tuple(int(x) for x in e_grain[e]) == tuple(g[0])
            assert tuple(int(x) for x in e_act[e]) == tuple(a[0])
            assert int(e_xlen[e]) == (-1 if g[1] is None else len(g[1].encode()))
    # decode
    sz = lambda dt, sh: n * np.dtype(dt).itemsize * int(np.prod(sh, dtype=np.int64))
    d = {k: z(sz(dt, sh)) for k, (dt, sh) in gd.FRAME_FIELDS.items()}
    dtf = {k: z(sz(dt, ())) for k, dt in gd.FRAME_TURN_FIELDS.items()}
    eng.decode_frames_turn_device(d_buf.data_ptr(), total, d_foff.data_ptr(), n, {k: v.data_ptr() for k, v in d.items()},
                                  {k: v.data_ptr() for k, v in dtf.items()})
    eng.synchronize()
    got = {k: d[k].cpu().numpy()[:sz(dt, sh)].view(dt).reshape((n,) + sh) for k, (dt, sh) in gd.FRAME_FIELDS.items()}
    got.update({k: dtf[k].cpu().numpy()[:sz(dt, ())].view(dt) for k, dt in gd.FRAME_TURN_FIELDS.items()})
    rows = C.decode_batch(want[0], want[1][:-1])                   # the reference decoder on the reference form
    for k in ("flags", "mask", "target_grain", "target_activation", "sending_activation", "sending_grain",
              "target_silo", "sending_silo", "correlation_id", "direction", "result", "rejection_type"):
        np.testing.assert_array_equal(got[k], rows[k], err_msg=k)
    assert (got["direction"] == 1).all() and (got["result"] == 2).all()
    assert (got["flags"] & gd.FRAME_INVALIDATION).all()
    for i in range(n):
        req = F.parse_fields(frames[i], struct.unpack_from("<i", frames[i], 0)[0])[0]
        assert int(got["correlation_id"][i]) == req["correlation_id"]
        assert tuple(int(x) for x in got["target_grain"][i]) == tuple(req["sending_grain"][0])
        assert tuple(int(x) for x in got["sending_grain"][i]) == tuple(req["target_grain"][0])
        assert got["target_silo"][i].tobytes() == H.w_silo(*req["sending_silo"])
        assert got["sending_silo"][i].tobytes() == H.w_silo(*req["target_silo"])
