"""GPU parity for the forward writer (gd_forward_*): TryForwardRequest + AddressMessage +
Message.Serialize for a batch, bit for bit against the byte-run form of the reference (_forward_ref.py): the status
of every frame, out_off, the TargetGrain keys and every output byte; and no byte outside the output is written.

Every device run goes into a buffer pre-filled with 0xA5 that has 64 spare bytes: the bytes before the output and
at or past out_off[n] must still be 0xA5 (_dev).  The source buffer holds exactly the frames: the last frame ends
at buf_len."""
import struct

import numpy as np
import pytest

import _forward_ref as F
import _sendq_ref as SQ
import headers as H

pytestmark = pytest.mark.gpu

TILE = 16384                                     # k_fwd_write's output bytes a workgroup (gd_frameout.h)
OK = (F.ST_OK_ADDRESSED, F.ST_OK_UNADDRESSED)


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
    e.encode_configure(F.SILO_TUPLES, F.TYPE_NAMES)
    e.activation_ids_set(np.arange(len(cfg.act_ids)), cfg.act_ids)
    yield e
    e.close()


def _dev(e, buf, offs, kind, old_act=None, fwd_silo=None, fwd_act=None, routes=None, order=None, lead=0,
         out_cap=None, max_fc=F.MAX_FC, local=F.LOCAL_SILO, want_target=True):
    """gd_forward_frames_device on torch buffers.  Returns (out bytes, out_off, fwd_status, target)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(offs)
    up = lambda a, dt, t: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt)).view(t)).to(dev)
    d_buf = torch.from_numpy(np.frombuffer(buf or b"\0", dtype=np.uint8).copy()).to(dev)
    d_off = up(offs if n else [0], np.uint64, np.int64)
    d_kind = up(kind if n else [0], np.uint8, np.uint8)
    d_old, d_fs, d_fa = up(old_act, np.uint32, np.int32), up(fwd_silo, np.uint32, np.int32), up(fwd_act, np.uint32, np.int32)
    r = (None,) * 5 if routes is None else routes
    d_r = [up(r[0], np.uint32, np.int32), up(r[1], np.uint32, np.int32), up(r[2], np.uint8, np.uint8),
           up(r[3], np.uint8, np.uint8), up(r[4], np.uint32, np.int32)]
    d_od = up(order, np.uint32, np.int32)
    cap = 2 * len(buf) + n * 256 if out_cap is None else out_cap
    room = torch.full((lead + cap + 64 + 16,), 0xA5, dtype=torch.uint8, device=dev)
    base = (-room.data_ptr()) % 16 + lead                          # out pointer = 16-B boundary + lead
    d_out_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device=dev)
    d_tg = torch.full((max(n, 1), 3), -1, dtype=torch.int64, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    db = {"buf": d_buf.data_ptr(), "buf_len": len(buf), "frame_off": d_off.data_ptr(), "kind": d_kind.data_ptr(),
          "old_act": ptr(d_old), "fwd_silo": ptr(d_fs), "fwd_act": ptr(d_fa), "max_forward_count": max_fc,
          "local_silo": local}
    torch.cuda.synchronize()
    e.forward_frames_device(db, n, *[ptr(t) for t in d_r], ptr(d_od), room.data_ptr() + base, cap,
                            d_out_off.data_ptr(), d_st.data_ptr(), d_tg.data_ptr() if want_target else None)
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
    tg = d_tg.cpu().numpy().view(np.uint64)[:n]
    if not want_target:
        assert (tg == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    return whole[base:base + total].tobytes(), out_off, d_st.cpu().numpy()[:n], tg


def _same(got, want, target=True):
    out, off, st = got[:3]
    wout, woff, wst = want[:3]
    np.testing.assert_array_equal(st, wst, err_msg="fwd_status")
    np.testing.assert_array_equal(off, woff, err_msg="out_off")
    if target:
        np.testing.assert_array_equal(got[3], want[3], err_msg="target")
    if out != wout:
        a, b = np.frombuffer(out, np.uint8), np.frombuffer(wout, np.uint8)
        k = int(np.flatnonzero(a != b)[0])
        j = int(np.searchsorted(woff, k, side="right")) - 1
        raise AssertionError(f"first differing byte {k} (output frame {j}, byte {k - int(woff[j])} of it): "
                             f"{a[k]:#x} != {b[k]:#x}")


def _check(e, cfg, batch, order=None, lead=0, **kw):
    """batch = (buf, offs, kind, old_act, fwd_silo, fwd_act, routes)."""
    want = F.forward_batch(*batch, order, kw.get("max_fc", F.MAX_FC), kw.get("local", F.LOCAL_SILO), cfg)
    _same(_dev(e, *batch, order=order, lead=lead, **kw), want)
    return want


K = (7, 8, 0x0300000000000011)
BASE = {"category": 2, "direction": 0, "correlation_id": 99, "target_grain": (K, None), "target_silo": F.SILOS[1],
        "target_activation": ((5, 6, 0), None), "sending_grain": ((1, 2, 0x0300000000000022), None),
        "sending_silo": F.SILOS[0], "time_to_live": 1 << 33}


def _good_acts(cfg, n, rng):
    good = np.flatnonzero(cfg.act_ids.any(axis=1))
    return rng.choice(good, size=n).astype(np.uint32)


def _plain(cfg, frames, rng, pad=b"", fwd=True):
    """A batch of the given frames, every one forwarded with an old address; with or without a forwarding address."""
    buf, offs = F.pack_frames(frames, pad)
    n = len(offs)
    fs = rng.integers(0, 5, size=n).astype(np.uint32) if fwd else None
    return (buf, offs, np.full(n, F.FWD_FORWARD, np.uint8), _good_acts(cfg, n, rng), fs,
            _good_acts(cfg, n, rng) if fwd else None, None)


# ----------------------------------------------------------------------------- batches
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_sizes(eng, cfg, n):
    rng = np.random.default_rng(300 + n)
    for k, lead in enumerate((0, 1, 7, 15)):
        batch = F.random_batch(n, rng, cfg, pad=bytes(k))          # source frames at all four byte alignments
        want = _check(eng, cfg, batch, lead=lead)
    if n >= 257:
        assert np.isin(want[2], OK).sum() > n // 2
    # the optional inputs absent: no old address, no forwarding address, no route, batch order, no target wanted
    buf, offs, kind = batch[:3]
    got = _dev(eng, buf, offs, kind, want_target=False)
    _same(got, F.forward_batch(buf, offs, kind, None, None, None, None, None, F.MAX_FC, F.LOCAL_SILO, cfg), target=False)
    # placed and new_type absent, the route arrays there
    r = batch[6][:3] + (None, None)
    _check(eng, cfg, batch[:6] + (r,))


def test_every_status_and_order(eng, cfg):
    rng = np.random.default_rng(31)
    n = 1200
    batch = F.random_batch(n, rng, cfg)
    want = _check(eng, cfg, batch)
    assert set(np.unique(want[2]).tolist()) == set(range(8))
    assert len(want[0]) > 2 * TILE                                  # frames straddle the tile edges
    _check(eng, cfg, batch, order=rng.permutation(n).astype(np.uint32), lead=5)
    _check(eng, cfg, batch, max_fc=1, local=4)
    assert (_check(eng, cfg, batch, local=7)[2] == F.ST_NO_SILO).sum() > n // 5     # every appended entry


def test_old_entries_past_the_window(eng, cfg):
    """2 and 3 old entries push TargetGrain past the 192-B staged window; a KeyExt TargetGrain goes into the entry."""
    rng = np.random.default_rng(32)
    frames = []
    for n_old in (1, 2, 3, 6):
        for x in (None, "", "e", "ext" * 5, "k" * 200):
            cat = 3 if x is None else 6
            h = dict(BASE, cache_invalidation=F.w_invalidation(F.rand_entries(rng, n_old)),
                     target_grain=((1, 2, (cat << 56) | 5), x), forward_count=1, debug_context="D" * (3 * n_old))
            frames.append(H.encode_frame(h, b"body" * n_old))
    for pad in (b"", b"\x01", b"\x01\x02", b"\x01\x02\x03"):
        for fwd in (True, False):
            want = _check(eng, cfg, _plain(cfg, frames, rng, pad, fwd))
            assert (want[2] == (F.ST_OK_ADDRESSED if fwd else F.ST_OK_UNADDRESSED)).all()


def test_run_edges_at_every_offset(eng, cfg):
    """DebugContext and KeyExt lengths 0..17 move every later run edge through every offset mod 16."""
    rng = np.random.default_rng(33)
    frames = []
    for d in range(1, 18):
        for x in range(18):
            h = dict(BASE, debug_context="D" * d, target_grain=((3, 4, 0x0600000000000007), "e" * x),
                     read_only=True, is_new_placement=bool(x & 1) or None, new_grain_type="T" * (1 + x // 3))
            h = {k: v for k, v in h.items() if v is not None}
            if d % 3 == 0:
                h["transaction_info"] = b"t" * (d + x)
            if d % 4 == 0:
                h["cache_invalidation"] = F.w_invalidation(F.rand_entries(rng, 1))
            frames.append(H.encode_frame(h, b"B" * ((3 * d + x) % 23)))
    n = len(frames)
    for lead, pad, fwd in ((0, b"", True), (3, b"\x00", False), (14, b"\x00\x00", True)):
        b = _plain(cfg, frames, rng, pad, fwd)
        routes = (rng.integers(0, 5, size=n).astype(np.uint32), _good_acts(cfg, n, rng), np.zeros(n, np.uint8),
                  rng.integers(0, 3, size=n).astype(np.uint8), rng.integers(0, 5, size=n).astype(np.uint32))
        want = _check(eng, cfg, b[:6] + (routes,), lead=lead)
        assert (want[2] == F.ST_OK_ADDRESSED).all()


def test_large_body_straddles_tiles(eng, cfg):
    rng = np.random.default_rng(34)
    frames = [H.encode_frame(dict(BASE, correlation_id=k), bytes(rng.integers(0, 256, size=k % 50, dtype=np.uint8)))
              for k in range(130)]
    frames[64] = H.encode_frame(BASE, bytes(rng.integers(0, 256, size=100000, dtype=np.uint8)))
    for lead, pad in ((0, b""), (9, b"\x01\x02\x03")):
        want = _check(eng, cfg, _plain(cfg, frames, rng, pad), lead=lead)
        assert np.isin(want[2], OK).all() and len(want[0]) > 100000 + TILE


def test_tile_edges(eng, cfg):
    """An output of exactly one 16-KiB tile and of one tile plus one byte; a frame edge and a body's first byte (a
    run edge inside a frame: the written TargetSilo ends there) on the tile boundary."""
    rng = np.random.default_rng(37)
    n = 40

    def frames(lens):
        return [H.encode_frame(dict(BASE, correlation_id=k), bytes(rng.integers(0, 256, size=lens[k], dtype=np.uint8)))
                for k in range(n)]

    empty = _plain(cfg, frames([0] * n), rng)
    w0 = F.forward_batch(*empty, None, F.MAX_FC, F.LOCAL_SILO, cfg)
    flen = int(w0[1][1])                                              # every forwarded frame has the same length
    assert (w0[2] == F.ST_OK_ADDRESSED).all() and len(w0[0]) == n * flen < TILE
    for total, split in ((TILE, 0), (TILE + 1, 0), (None, 1), (None, 2)):
        lens = [0] * n
        if split == 0:
            lens[5] = total - n * flen                                # one body brings the total to `total`
        elif split == 1:
            lens[5], lens[30] = TILE - 20 * flen, 40                  # frame 20 starts on the tile boundary
        else:
            lens[5], lens[20] = TILE - 21 * flen, 40                  # frame 20's body starts on the tile boundary
        total = n * flen + sum(lens)
        b = F.pack_frames(frames(lens), b"") + empty[2:]
        for lead in (0, 9):
            want = _check(eng, cfg, b, lead=lead)
            assert len(want[0]) == total
            if split == 1:
                assert int(want[1][20]) == TILE
            if split == 2:
                assert int(want[1][21]) - lens[20] == TILE


def test_more_frame_starts_in_a_tile_than_the_lds_offsets(eng, cfg):
    rng = np.random.default_rng(35)
    frames = [H.encode_frame(dict(BASE, correlation_id=k), b"") for k in range(1502)]
    batch = list(_plain(cfg, frames, rng))
    batch[2][1:1501] = F.FWD_NONE                                  # 1,500 zero-length frames inside one tile
    want = _check(eng, cfg, tuple(batch))
    assert (want[2][1:1501] == F.ST_SKIPPED).all() and want[2][0] == want[2][1501] == F.ST_OK_ADDRESSED
    batch[2][:] = F.FWD_NONE                                       # all skipped: total 0, nothing written
    assert _check(eng, cfg, tuple(batch))[0] == b""


def test_capacity(eng, cfg, gd):
    rng = np.random.default_rng(36)
    batch = F.random_batch(300, rng, cfg)
    want = F.forward_batch(*batch, None, F.MAX_FC, F.LOCAL_SILO, cfg)
    total = len(want[0])
    with pytest.raises(gd.GrainDispatchError) as ei:               # at the next synchronisation: out_off complete,
        _dev(eng, *batch, out_cap=total - 1)                       # nothing written (_dev's canary)
    assert ei.value.code == gd.GD_EFULL
    np.testing.assert_array_equal(ei.value.out_off, want[1])
    out = np.full(total - 1, 0xA5, np.uint8)
    with pytest.raises(gd.GrainDispatchError) as ei:
        eng.forward_frames(_hb(batch), *_hr(batch), out=out)
    assert ei.value.code == gd.GD_EFULL and (out == 0xA5).all()
    _same(_dev(eng, *batch, out_cap=total), want)                  # exactly enough; the handle still works


def _hb(batch, max_fc=F.MAX_FC, local=F.LOCAL_SILO):
    return {"buf": batch[0], "offsets": batch[1], "kind": batch[2], "old_act": batch[3], "fwd_silo": batch[4],
            "fwd_act": batch[5], "max_forward_count": max_fc, "local_silo": local}


def _hr(batch):
    return (None,) * 5 if batch[6] is None else batch[6]


def test_host_forms_agree(eng, cfg):
    rng = np.random.default_rng(37)
    batch = F.random_batch(500, rng, cfg)
    order = rng.permutation(500).astype(np.uint32)
    want = F.forward_batch(*batch, order, F.MAX_FC, F.LOCAL_SILO, cfg)
    got = _dev(eng, *batch, order=order)
    out = np.full(len(want[0]) + 64, 0xA5, np.uint8)
    o2, off, st, tg, total = eng.forward_frames(_hb(batch), *_hr(batch), order=order, out=out)
    assert o2 is out and total == len(want[0]) and (out[total:] == 0xA5).all()
    _same((out[:total].tobytes(), off, st, tg), want)
    _same(got, (out[:total].tobytes(), off, st, tg))
    buf, offs, kind = batch[:3]                                    # every optional input absent
    o3, off3, st3, tg3, t3 = eng.forward_frames({"buf": buf, "offsets": offs, "kind": kind})
    _same((o3[:t3].tobytes(), off3, st3, tg3),
          F.forward_batch(buf, offs, kind, None, None, None, None, None, 2, 0, cfg))


def test_kinds(eng):
    import torch
    turn = np.arange(12, dtype=np.uint8).repeat(7)
    want = F.kinds_from_turns(turn)
    np.testing.assert_array_equal(eng.forward_kinds(turn), want)
    dt, dk = torch.from_numpy(turn).cuda(), torch.full((len(turn),), 9, dtype=torch.uint8).cuda()
    eng.forward_kinds_device(dt.data_ptr(), len(turn), dk.data_ptr())
    eng.synchronize()
    np.testing.assert_array_equal(dk.cpu().numpy(), want)
    assert set(want.tolist()) == {0, 1}


def test_round_trip_twice_then_reject(eng, cfg):
    """ForwardCount 0 -> 1 -> 2 through the device, the output of one pass the input of the next; the third attempt
    is REJECT and the header holds the two entries in order."""
    rng = np.random.default_rng(38)
    frames = [H.encode_frame(dict(BASE, correlation_id=k, target_grain=((k, 2, 0x0300000000000005), None)), b"p" * k)
              for k in range(40)]
    b1 = _plain(cfg, frames, rng, fwd=True)
    o1 = _check(eng, cfg, b1)
    b2 = (o1[0], o1[1][:-1].copy(), b1[2], _good_acts(cfg, 40, rng), None, None, None)
    o2 = _check(eng, cfg, b2, local=4)
    assert (o1[2] == F.ST_OK_ADDRESSED).all() and (o2[2] == F.ST_OK_UNADDRESSED).all()
    b3 = (o2[0], o2[1][:-1].copy(), b1[2], b2[3], None, None, None)
    o3 = _check(eng, cfg, b3)
    assert (o3[2] == F.ST_REJECT).all() and o3[0] == b""
    for k in range(40):
        fr = o2[0][int(o2[1][k]):int(o2[1][k + 1])]
        h = F.parse_fields(fr, struct.unpack_from("<i", fr, 0)[0])[0]
        assert h["forward_count"] == 2 and fr.endswith(b"p" * k)
        assert [(e[0], e[2][0]) for e in h["invalidation"]] == [
            (H.w_silo(*F.SILOS[F.LOCAL_SILO]), cfg.act_id(int(b1[3][k]))), (H.w_silo(*F.SILOS[4]), cfg.act_id(int(b2[3][k])))]


# ----------------------------------------------------------------------------- the chain
def _chain_engine(gd, nq, rng):
    """A handle with a ring of 3 silos, a directory of a few hundred grains and every table of the chain."""
    import oracle as o
    silos = o.bench_silos(3)
    tuples = [(s.ip, s.port, s.gen) for s in silos]
    wire = [H.w_silo(bytes(gd.silo_addr(*t).ip), t[1], t[2]) for t in tuples]
    G = 300
    ids = np.zeros((G, 3), np.uint64)
    ids[:, 0], ids[:, 1], ids[:, 2] = np.arange(G) + 77, 5, 0x0400000000000000
    ids[9::50] = 0                                                  # some activations without an id
    spec = o.ring_spec(silos, "D")
    tc = o.grain_type_code(o.PING_GRAIN_CLASS)
    reg = o.grain_keys(tc, np.arange(G))
    owner = o.ring_owner_np(spec, o.jenkins_u64x3_np(reg[:, 2], reg[:, 0], reg[:, 1])).astype(np.uint32)
    e = gd.GrainDispatch(device=0, table_capacity=4 * G, my_silo=1)
    e.ring_set_silos("D", tuples)
    e.register(reg, np.arange(G), owner)
    e.encode_configure(tuples, F.TYPE_NAMES)
    e.activation_ids_set(np.arange(G), ids)
    sh = SQ.hashes_with_edges(rng, len(tuples))
    e.send_configure(sh, nq)
    from _encode_ref import Config
    return e, Config(wire, F.TYPE_NAMES, ids), sh, o.grain_keys(tc, rng.integers(0, G + 40, size=900))


def test_chain(gd):
    """gd_forward_send = forward_frames(route(keys)) composed on the host; each sender queue's byte range holds
    exactly its frames; the result decodes with the reference's field reader."""
    import torch
    rng = np.random.default_rng(39)
    nq = 4
    e, cfg, sh, targets = _chain_engine(gd, nq, rng)
    n = len(targets)
    with e:
        frames = []
        for k in range(n):
            if rng.random() < 0.08:
                frames.append(F.odd_frame(rng))
                continue
            fr = F.normal_frame(rng)
            if rng.random() < 0.85:                                # most frames: a long-keyed target of the directory
                h = F.parse_fields(fr, struct.unpack_from("<i", fr, 0)[0])[0]
                inv = h.pop("invalidation", None)
                if inv:
                    h["cache_invalidation"] = F.w_invalidation(inv)
                h["target_grain"] = (tuple(int(x) for x in targets[k]), None)
                fr = H.encode_frame(h, b"b" * (k % 9))
            frames.append(fr)
        buf, offs = F.pack_frames(frames)
        kind = rng.choice([F.FWD_FORWARD, F.FWD_NONE], size=n, p=[0.93, 0.07]).astype(np.uint8)
        old_act = rng.integers(0, 300, size=n).astype(np.uint32)
        old_act[rng.random(n) < 0.3] = F.NONE32
        fwd_silo = rng.integers(0, 3, size=n).astype(np.uint32)
        fwd_silo[rng.random(n) < 0.6] = F.NONE32
        fwd_act = rng.integers(0, 300, size=n).astype(np.uint32)
        hb = {"buf": buf, "offsets": offs, "kind": kind, "old_act": old_act, "fwd_silo": fwd_silo, "fwd_act": fwd_act,
              "max_forward_count": 2, "local_silo": 1}
        # the stages composed on the host: plan without a route, route the keys, merge, send queues, write
        _, _, st0, tg0, _ = e.forward_frames(hb)
        rst, silo, act = e.route(tg0)
        fields = lambda i: F.parse_fields(buf[int(offs[i]):], struct.unpack_from("<i", buf, int(offs[i]))[0])[0]
        ext = [st0[i] in OK and fields(i)["target_grain"][1] is not None for i in range(n)]
        for i in range(n):
            if st0[i] == F.ST_OK_ADDRESSED:
                silo[i], act[i], rst[i] = fwd_silo[i], fwd_act[i], 0
            elif st0[i] != F.ST_OK_UNADDRESSED:
                silo[i], act[i], rst[i] = F.NONE32, F.NONE32, 6
            elif ext[i]:
                silo[i], act[i], rst[i] = F.NONE32, F.NONE32, 4
        ttl, cat = np.full(n, np.iinfo(np.int64).max, np.int64), np.zeros(n, np.uint8)
        for i in range(n):
            if st0[i] in OK:
                h = fields(i)
                ttl[i], cat[i] = h.get("time_to_live", ttl[i]), h.get("category", 0)
        sst, q, perm, qoff = e.send_queues(silo, rst, cat, ttl)
        wperm, wqoff = SQ.send_queues_loop(silo, rst, cat, ttl, sh, nq, 1)[2:4]
        np.testing.assert_array_equal(perm, wperm)
        routes = (silo, act, rst, None, None)
        want = F.forward_batch(buf, offs, kind, old_act, fwd_silo, fwd_act, routes, perm, 2, 1, cfg)
        out, off, st, tg, total = e.forward_frames(hb, *routes, order=perm)
        _same((out[:total].tobytes(), off, st, tg), want)
        assert (st == F.ST_OK_ADDRESSED).sum() > n // 3 and (st == F.ST_OK_UNADDRESSED).sum() > n // 20
        assert (rst == 0).sum() > n // 3 and (rst == 1).any() and {6, 0} <= set(rst.tolist())
        # ... the host chain ...
        c = e.forward_send(hb)
        for k, w in (("status", rst), ("silo", silo), ("act", act), ("send_status", sst), ("queue", q), ("perm", perm),
                     ("offsets", qoff), ("out_off", off), ("fwd_status", st), ("target", tg)):
            np.testing.assert_array_equal(c[k], w, err_msg=k)
        assert c["total"] == total and c["out"][:total].tobytes() == out[:total].tobytes()
        # ... and the device chain
        dev = torch.device("cuda:0")
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(dev)
        d_buf, d_foff, d_kind = up(np.frombuffer(buf, np.uint8).copy(), np.uint8), up(offs, np.int64), up(kind, np.uint8)
        d_old, d_fs, d_fa = up(old_act, np.int32), up(fwd_silo, np.int32), up(fwd_act, np.int32)
        i32 = lambda k: torch.full((k,), -1, dtype=torch.int32, device=dev)
        u8 = lambda k: torch.full((k,), 0xEE, dtype=torch.uint8, device=dev)
        d_silo, d_act, d_perm, d_q, d_qoff = i32(n), i32(n), i32(n), i32(n), i32(nq + 5)
        d_rst, d_sst, d_st = u8(n), u8(n), u8(n)
        d_out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=dev)
        d_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
        d_tg = torch.full((n, 3), -1, dtype=torch.int64, device=dev)
        db = {"buf": d_buf.data_ptr(), "buf_len": len(buf), "frame_off": d_foff.data_ptr(), "kind": d_kind.data_ptr(),
              "old_act": d_old.data_ptr(), "fwd_silo": d_fs.data_ptr(), "fwd_act": d_fa.data_ptr(),
              "max_forward_count": 2, "local_silo": 1}
        torch.cuda.synchronize()
        e.forward_send_device(db, n, d_silo.data_ptr(), d_act.data_ptr(), d_rst.data_ptr(), d_sst.data_ptr(),
                              d_q.data_ptr(), d_perm.data_ptr(), d_qoff.data_ptr(), d_out.data_ptr(), total,
                              d_off.data_ptr(), d_st.data_ptr(), d_tg.data_ptr())
        e.synchronize()
        h32 = lambda x: x.cpu().numpy().view(np.uint32)
        for got, w, name in ((h32(d_silo), silo, "silo"), (h32(d_act), act, "act"), (d_rst.cpu().numpy(), rst, "status"),
                             (d_sst.cpu().numpy(), sst, "send_status"), (h32(d_q), q, "queue"), (h32(d_perm), perm, "perm"),
                             (h32(d_qoff), qoff, "offsets"), (d_off.cpu().numpy().view(np.uint64), off, "out_off"),
                             (d_st.cpu().numpy(), st, "fwd_status"), (d_tg.cpu().numpy().view(np.uint64), tg, "target")):
            np.testing.assert_array_equal(got, w, err_msg=name)
        whole = d_out.cpu().numpy()
        assert whole[:total].tobytes() == out[:total].tobytes() and (whole[total:] == 0xA5).all()
    # each sender queue's byte range holds exactly its frames, and they decode with the reference's field reader
    single = F.forward_batch(buf, offs, kind, old_act, fwd_silo, fwd_act, routes, None, 2, 1, cfg)
    fr_of = lambda i: single[0][int(single[1][i]):int(single[1][i + 1])]
    res = out[:total].tobytes()
    for b in range(len(qoff) - 1):
        members = perm[qoff[b]:qoff[b + 1]]
        run = res[int(off[qoff[b]]):int(off[qoff[b + 1]])]
        assert run == b"".join(fr_of(int(i)) for i in members)
    for i in np.flatnonzero(np.isin(st, OK))[:200]:
        fr = fr_of(int(i))
        h = F.parse_fields(fr, struct.unpack_from("<i", fr, 0)[0])[0]
        assert tuple(h["target_grain"][0]) == tuple(int(x) for x in tg[i])
        assert ("target_silo" in h) == (st[i] == F.ST_OK_ADDRESSED)
        if old_act[i] != F.NONE32:
            assert h["invalidation"][-1][0] == cfg.silos[1] and h["invalidation"][-1][2][0] == cfg.act_id(int(old_act[i]))


def test_state_errors(gd, eng, cfg):
    with gd.GrainDispatch(device=0, table_capacity=1 << 10) as e:
        for n in (0, 3):
            with pytest.raises(gd.GrainDispatchError) as ei:       # before gd_encode_configure
                e.forward_frames({"buf": b"\0" * 64, "offsets": np.zeros(n, np.uint64), "kind": np.zeros(n, np.uint8)})
            assert ei.value.code == gd.GD_ESTATE
        with pytest.raises(gd.GrainDispatchError) as ei:
            e.forward_kinds(np.zeros(3, np.uint8))
        assert ei.value.code == gd.GD_ESTATE
        e.encode_configure(F.SILO_TUPLES)
        with pytest.raises(gd.GrainDispatchError) as ei:           # the chain: before gd_send_configure
            e.forward_send({"buf": b"\0" * 64, "offsets": np.zeros(1, np.uint64), "kind": np.zeros(1, np.uint8)})
        assert ei.value.code == gd.GD_ESTATE
    out, off, st, tg, total = eng.forward_frames({"buf": b"", "offsets": [], "kind": []}, order=np.zeros(0, np.uint32),
                                                 out_cap=16)
    assert total == 0 and off.tolist() == [0] and len(st) == 0
    with pytest.raises(gd.GrainDispatchError) as ei:               # totals are 32-bit: the bound is refused
        eng.forward_frames_device({"buf": 8, "buf_len": (1 << 31) - 100, "frame_off": 8, "kind": 8}, 2, None, None, None,
                                  None, None, None, 8, 0, 8, 8, None)
    assert ei.value.code == gd.GD_EINVAL
    with pytest.raises(gd.GrainDispatchError) as ei:               # the route arrays go together
        eng.forward_frames_device({"buf": 8, "buf_len": 64, "frame_off": 8, "kind": 8}, 2, 8, None, None, None, None,
                                  None, 8, 0, 8, 8, None)
    assert ei.value.code == gd.GD_EINVAL
