"""GPU parity for the sniff stage (gd_sniff_frames*, gd_cache_invalidate*, gd_sniff_invalidate*):
SniffIncomingMessage + InvalidateCacheEntry for a received batch against the per-message reference (_sniff_ref.py):
every output array, the cache's statistics, its entries with their generations, and NumAccesses of every entry.

Every device output is pre-filled with 0xA5 and has 64 spare bytes: entries at or past m and the bytes past the
arrays must still be 0xA5.  The source buffer holds exactly the frames: the last frame ends at buf_len."""
import struct

import numpy as np
import pytest

import _forward_ref as F
import _sniff_ref as S
import headers as H

pytestmark = pytest.mark.gpu

SEED = 4100                                       # tests/test_sniff_ref.py asserts the conditions for these batches
PER_FRAME = {"count": (np.uint32, 1), "ent_off": (np.uint32, 1), "status": (np.uint8, 1), "flags": (np.uint8, 1)}
PER_ENTRY = {"ent_frame": (np.uint32, 1), "ent_silo": (np.uint32, 6), "ent_grain": (np.uint64, 3),
             "ent_ext_off": (np.uint64, 1), "ent_ext_len": (np.int32, 1), "ent_act_id": (np.uint64, 3)}
SENT = 0xA5


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    assert g.GD_SNIFF_MALFORMED == S.SNIFF_MALFORMED and g.GD_INV_NO_ID == S.INV_NO_ID
    return g


def _engine(gd, sc, configure=True):
    """A handle whose cache holds the scene's entries, added in the reference's order."""
    e = gd.GrainDispatch(device=0, table_capacity=1 << 10)
    e.activation_ids_set(np.arange(len(sc.act_ids)), sc.act_ids)
    if not configure:
        return e
    e.cache_configure(sc.cache_size, [], 5)
    order = sc.load_order()
    full = [c for c in order if c[2] != S.EMPTY_SILO]
    empty = [c for c in order if c[2] == S.EMPTY_SILO]
    exts = lambda cs: [None if sc.grains[c[0]][1] is None else sc.grains[c[0]][1].encode() for c in cs]
    keys = lambda cs: np.array([sc.grains[c[0]][0] for c in cs], np.uint64).reshape(-1, 3)
    if full:
        e.cache_add(keys(full), [c[1] for c in full], [c[2] for c in full], [c[3] for c in full], exts(full))
    if empty:                                                # an empty address list comes by a refresh response
        st = e.cache_refresh_apply(1000, keys(empty), [gd.GD_LM_UPDATED] * len(empty), [gd.NO_ACTIVATION] * len(empty),
                                   [gd.NO_SILO] * len(empty), [c[3] for c in empty], exts(empty))
        assert (st == gd.GD_CR_UPDATED).all()
    return e


def _same_cache(e, cache):
    kv, nacc, (accesses, hits, next_gen) = cache.state()
    ent = e.cache_entries_ext()
    assert ent == kv
    acc = e.cache_entries_age()[2]
    assert {k: int(a) for k, a in zip(ent, acc)} == nacc
    st = e.cache_stats()
    assert (st["count"], st["accesses"], st["hits"], st["next_generation"]) == (len(kv), accesses, hits, next_gen)


def _dev(e, buf, offs, ent_cap, chain=True, skip=()):
    """gd_sniff_invalidate_device (chain) or gd_sniff_frames_device on torch buffers pre-filled with 0xA5.  Returns
    (arrays by name -- the per-entry ones whole, ent_cap long --, the error of the checked synchronisation or None)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(offs)
    d_buf = torch.from_numpy(np.frombuffer(buf or b"\0", dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(np.asarray(offs if n else [0], np.uint64).view(np.int64).copy()).to(dev)
    sizes = {f: (dt, w, n + (f == "ent_off")) for f, (dt, w) in PER_FRAME.items()}
    sizes.update({f: (dt, w, ent_cap) for f, (dt, w) in PER_ENTRY.items()})
    sizes["inv"] = (np.uint8, 1, ent_cap)
    t = {f: torch.full((cnt * w * np.dtype(dt).itemsize + 64,), SENT, dtype=torch.uint8, device=dev)
         for f, (dt, w, cnt) in sizes.items() if f not in skip}
    d_out = {f: t[f].data_ptr() for f in t if f != "inv"}
    torch.cuda.synchronize()
    if chain:
        e.sniff_invalidate_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n, d_out, ent_cap, t["inv"].data_ptr())
    else:
        e.sniff_frames_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n, d_out, ent_cap)
    err = None
    try:
        e.synchronize()
    except Exception as ex:                                  # GD_EFULL surfaces here
        err = ex
    got = {}
    for f, x in t.items():
        dt, w, cnt = sizes[f]
        raw = x.cpu().numpy()
        used = cnt * w * np.dtype(dt).itemsize
        assert (raw[used:] == SENT).all(), f"bytes past {f} were written"
        a = raw[:used].view(dt)
        got[f] = a.reshape(cnt, w) if w > 1 else a
    return got, err


def _same(got, want, chain=True, skip=()):
    m = want["m"]
    for f in PER_FRAME:
        if f not in skip:
            np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    names = list(PER_ENTRY) + (["inv"] if chain else [])
    for f in names:
        if f in skip:
            continue
        np.testing.assert_array_equal(got[f][:m], want[f], err_msg=f)
        assert (got[f][m:].view(np.uint8) == SENT).all(), f"{f} at or past m was written"


def _run(gd, sc, buf, offs, ent_cap=None, e=None):
    """The chain on a fresh engine against form (a); returns (engine, reference outputs, reference cache)."""
    own = e is None
    e = e or _engine(gd, sc)
    cache = sc.new_cache()
    want = S.sniff_messages(buf, offs, cache)
    got, err = _dev(e, buf, offs, want["m"] + 3 if ent_cap is None else ent_cap)
    assert err is None, err
    _same(got, want)
    _same_cache(e, cache)
    if own:
        e.close()
    return want


# ----------------------------------------------------------------------------- 1. random batches
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_random_batches(gd, n):
    sc = S.Scene(n, SEED + n)
    for pad in (b"", b"\x01", b"\x01\x02", b"\x01\x02\x03"):   # all four alignments of frame_off
        buf, offs = sc.pack(pad)
        want = _run(gd, sc, buf, offs)
        assert {int(o) % 4 for o in offs} == {0, 1, 2, 3} or n < 8
    S.check_conditions(sc, want)
    # 9. the existing stages are untouched: the decoder still answers FALLBACK for the frames with the header
    with _engine(gd, sc, configure=False) as e:
        flags = e.decode_frames(buf, offs, ["flags"])["flags"]
    hdr = want["status"] == S.SNIFF_OK
    assert hdr.any() and (flags[hdr] & gd.FRAME_FALLBACK).all() and not (flags[hdr] & gd.FRAME_HAS_TARGET).any()


# ----------------------------------------------------------------------------- 2. order inside a batch
def _frame(sc, entries):
    return S.with_invalidation(F.normal_frame(sc.rng, n_old=0), entries)


def test_order_inside_a_batch(gd):
    sc = S.Scene(1, 21)
    other, match = sc._entry(0, "other"), sc._entry(0, "match")
    m5 = sc._entry(5, "match")
    frames = [_frame(sc, [other, match, match]),                             # KEPT, REMOVED, MISS
              _frame(sc, [m5, sc._entry(5, "other")]), _frame(sc, [m5]),     # REMOVED, MISS, MISS
              _frame(sc, [sc._entry(8, "other"), sc._entry(10, "other"), sc._entry(8, "other")])]
    buf, offs = F.pack_frames(frames)
    e = _engine(gd, sc)
    before = e.cache_stats()["next_generation"]
    want = _run(gd, sc, buf, offs, e=e)
    assert want["inv"].tolist() == [S.INV_KEPT, S.INV_REMOVED, S.INV_MISS, S.INV_REMOVED, S.INV_MISS, S.INV_MISS,
                                    S.INV_KEPT, S.INV_KEPT, S.INV_KEPT]
    ent = e.cache_entries_ext()
    assert e.cache_stats()["next_generation"] == before + 6                 # the hits: 2 + 1 + 3
    assert ent[sc.key(10)][3] == before + 5 and ent[sc.key(8)][3] == before + 6   # survivors in batch order
    e.close()


def test_same_grain_across_a_wave_boundary(gd):
    sc = S.Scene(1, 22)
    match = sc._entry(0, "match")
    fill = [sc._entry(j, "other") for j in (8, 9, 10, 12, 13, 14, 16)]
    frames = [_frame(sc, [fill[k % 7]]) for k in range(63)] + [_frame(sc, [match]), _frame(sc, [match])]
    buf, offs = F.pack_frames(frames)
    want = _run(gd, sc, buf, offs)
    assert want["inv"][63] == S.INV_REMOVED and want["inv"][64] == S.INV_MISS and want["m"] == 65


# ----------------------------------------------------------------------------- 3. the header past the window
def test_header_past_the_staging_window(gd):
    sc = S.Scene(40, 23)
    kx = [j for j, (g, x) in enumerate(sc.grains) if x is not None]
    frames = []
    for cnt in (3, 6):
        for r in range(4):
            es = [sc._entry(kx[(r + 2 * k) % len(kx)], "match" if k % 2 else "other") for k in range(cnt)]
            frames.append(_frame(sc, es))
    for pad in (b"", b"\x07"):
        buf, offs = F.pack_frames(frames, pad)
        want = _run(gd, sc, buf, offs)
        assert (want["ent_ext_len"] >= 0).all() and (want["ent_ext_len"] >= 40).any()
        assert (want["ent_ext_off"] - np.repeat(offs, want["count"]) > 192).any()     # strings read past the window


# ----------------------------------------------------------------------------- 4. malformed frames
def test_malformed_frames(gd):
    sc = S.Scene(1, 24)
    ok = lambda: _frame(sc, [sc._entry(0, "other"), sc._entry(8, "match")])
    es = [sc._entry(9, "match"), sc._entry(10, "match")]
    neg = S.with_invalidation(F.normal_frame(sc.rng, n_old=0), es, count=-1)
    huge = S.with_invalidation(F.normal_frame(sc.rng, n_old=0), es, count=0x7fffffff)
    bad_len = bytearray(_frame(sc, es))
    struct.pack_into("<i", bad_len, 16 + 24 + 24, -2)                      # the first GrainId's string length
    cut = bytearray(_frame(sc, es))
    body = struct.unpack_from("<i", cut, 4)[0]
    struct.pack_into("<ii", cut, 0, 4 + 4 + 80 + 40, len(cut) - 8 - (4 + 4 + 80 + 40))   # headerLength ends in entry 2
    assert body >= 0
    last = ok()                                                             # cut by buf_len: 5 bytes short
    frames = [ok(), neg, ok(), huge, bytes(bad_len), ok(), bytes(cut), ok(), last]
    buf, offs = F.pack_frames(frames)
    buf = buf[:-5]
    want = _run(gd, sc, buf, offs)
    assert want["status"].tolist() == [1, 2, 1, 2, 2, 1, 2, 1, 2]
    assert want["count"].tolist() == [2, 0, 2, 0, 0, 2, 0, 2, 0]


# ----------------------------------------------------------------------------- 5. capacity
def test_capacity(gd):
    sc = S.Scene(65, SEED + 65)
    buf, offs = sc.pack()
    ref = S.sniff_messages(buf, offs)
    m = ref["m"]
    e = _engine(gd, sc)
    cache = sc.new_cache()
    # the device form: the error at the next checked call, ent_off complete, nothing else written
    got, err = _dev(e, buf, offs, m - 1)
    assert err is not None and err.code == gd.GD_EFULL
    np.testing.assert_array_equal(got["ent_off"], ref["ent_off"])
    np.testing.assert_array_equal(got["count"], ref["count"])
    for f in list(PER_ENTRY) + ["inv"]:
        assert (got[f].view(np.uint8) == SENT).all(), f
    _same_cache(e, cache)
    # the host form
    with pytest.raises(gd.GrainDispatchError) as ei:
        e.sniff_invalidate(buf, offs, ent_cap=m - 1)
    assert ei.value.code == gd.GD_EFULL
    np.testing.assert_array_equal(ei.value.arrays["ent_off"], ref["ent_off"])
    assert not ei.value.arrays["ent_grain"].any() and not ei.value.arrays["inv"].any()
    _same_cache(e, cache)
    with pytest.raises(gd.GrainDispatchError) as ei:
        e.sniff_frames(buf, offs, ent_cap=m - 1)
    assert ei.value.code == gd.GD_EFULL
    e.synchronize()                                          # reported once
    # ent_cap = m exactly
    _run(gd, sc, buf, offs, ent_cap=m, e=e)
    e.close()


# ----------------------------------------------------------------------------- 6. d_m on the device
def test_live_count_on_the_device(gd):
    import torch
    sc = S.Scene(64, SEED + 64)
    buf, offs = sc.pack()
    ref = S.sniff_messages(buf, offs)
    m, live = ref["m"], ref["m"] // 2
    e = _engine(gd, sc)
    cache = sc.new_cache()
    keys = [S.cache_key(ref["ent_grain"][k], ref["ent_ext"][k]) for k in range(m)]
    ids = [None if not ref["ent_act_id"][k].any() else tuple(int(x) for x in ref["ent_act_id"][k]) for k in range(m)]
    want = [S.invalidate_cache_entry(cache, keys[k], ids[k]) for k in range(live)]
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_buf, d_k, d_id = up(np.frombuffer(buf, np.uint8)), up(ref["ent_grain"]), up(ref["ent_act_id"])
    d_xo, d_xl = up(ref["ent_ext_off"]), up(ref["ent_ext_len"])
    d_m = up(np.array([live], np.uint32))
    d_out = torch.full((m + 64,), SENT, dtype=torch.uint8, device=dev)
    ext = {"bytes": d_buf.data_ptr(), "offset": d_xo.data_ptr(), "length": d_xl.data_ptr(), "bytes_len": len(buf)}
    torch.cuda.synchronize()
    e.cache_invalidate_device(d_k.data_ptr(), ext, d_id.data_ptr(), m, d_m.data_ptr(), d_out.data_ptr())
    e.synchronize()
    out = d_out.cpu().numpy()
    assert out[:live].tolist() == want and (out[live:] == SENT).all()
    _same_cache(e, cache)
    # without d_m, and through the host form with copied strings: the rest of the batch
    rest = [S.invalidate_cache_entry(cache, keys[k], ids[k]) for k in range(live, m)]
    got = e.cache_invalidate(ref["ent_grain"][live:], ref["ent_act_id"][live:], ref["ent_ext"][live:])
    assert got.tolist() == rest
    _same_cache(e, cache)
    # keys the device cannot match: a miss without an access in the device form, GD_EINVAL in the host form
    kx = np.array([sc.grains[5][0]], np.uint64)
    d_k1, d_id1 = up(kx), up(np.zeros((1, 3), np.uint64))
    d_xo1, d_xl1 = up(np.array([len(buf) - 1], np.uint64)), up(np.array([2], np.int32))
    ext1 = dict(ext, offset=d_xo1.data_ptr(), length=d_xl1.data_ptr())
    e.cache_invalidate_device(d_k1.data_ptr(), ext1, d_id1.data_ptr(), 1, None, d_out.data_ptr())
    e.synchronize()
    assert d_out.cpu().numpy()[0] == S.INV_MISS
    _same_cache(e, cache)
    with pytest.raises(gd.GrainDispatchError) as ei:
        e.cache_invalidate(kx, np.zeros((1, 3), np.uint64), [gd.GD_KEYEXT_HOST])
    assert ei.value.code == gd.GD_EINVAL
    _same_cache(e, cache)
    e.close()


# ----------------------------------------------------------------------------- 7. nothing to do
def test_empty_batches_and_state(gd):
    sc = S.Scene(1, 25)
    e = _engine(gd, sc)
    cache = sc.new_cache()
    got, err = _dev(e, b"", [], 4)
    assert err is None and got["ent_off"].tolist() == [0]
    assert e.sniff_invalidate(b"", [])["m"] == 0 and len(e.cache_invalidate(np.zeros((0, 3), np.uint64), np.zeros((0, 3), np.uint64))) == 0
    frames = [F.normal_frame(sc.rng, n_old=0) for _ in range(70)]          # no header at all
    buf, offs = F.pack_frames(frames, b"\x00")
    want = _run(gd, sc, buf, offs, ent_cap=0, e=e)
    assert want["m"] == 0 and (want["status"] == S.SNIFF_NONE).all()
    _same_cache(e, cache)                                                    # accesses too
    e.close()
    bare = _engine(gd, sc, configure=False)
    for call in (lambda: bare.sniff_invalidate(buf, offs), lambda: bare.cache_invalidate(np.zeros((1, 3), np.uint64), np.zeros((1, 3), np.uint64))):
        with pytest.raises(gd.GrainDispatchError) as ei:
            call()
        assert ei.value.code == gd.GD_ESTATE
    assert bare.sniff_frames(buf, offs)["m"] == 0                            # the first stage needs no cache
    bare.close()


# ----------------------------------------------------------------------------- 8. against the forward writer
def test_chain_against_the_forward_writer(gd):
    rng = np.random.default_rng(26)
    cfg = F.make_config(rng)
    good = np.flatnonzero(cfg.act_ids.any(axis=1))
    n = 40
    old, new = good[:n].astype(np.uint32), good[n:2 * n].astype(np.uint32)
    keys = np.array([(int(rng.integers(1, 1 << 60)), j, S.PLAIN_TCD) for j in range(n)], np.uint64)
    base = {"category": 2, "direction": 0, "correlation_id": 9, "sending_silo": F.SILOS[0], "time_to_live": 1 << 33}
    frames = [H.encode_frame(dict(base, target_grain=(tuple(int(x) for x in keys[j]), None)), b"b" * j) for j in range(n)]
    buf, offs = F.pack_frames(frames)
    with gd.GrainDispatch(device=0, table_capacity=1 << 10) as a:            # the forwarding silo
        a.encode_configure(F.SILO_TUPLES, F.TYPE_NAMES)
        a.activation_ids_set(np.arange(len(cfg.act_ids)), cfg.act_ids)
        out, out_off, fst, _, total = a.forward_frames(
            {"buf": buf, "offsets": offs, "kind": np.full(n, gd.GD_FWD_FORWARD, np.uint8), "old_act": old,
             "local_silo": F.LOCAL_SILO})
    assert (fst == gd.GD_FWDST_OK_UNADDRESSED).all()
    fwd = out[:total].tobytes()

    def receiver():
        b = gd.GrainDispatch(device=0, table_capacity=1 << 10)
        b.ring_set_silos("D", F.SILO_TUPLES)
        b.activation_ids_set(np.arange(len(cfg.act_ids)), cfg.act_ids)
        b.cache_configure(256, [], 5)
        b.cache_add(keys, np.concatenate([old[:n // 2], new[n // 2:]]), np.full(n, F.LOCAL_SILO), np.arange(n))
        return b

    b = receiver()
    r = b.sniff_invalidate(fwd, out_off[:n])
    assert r["m"] == n and (r["status"] == S.SNIFF_OK).all()
    np.testing.assert_array_equal(r["ent_grain"], keys)
    np.testing.assert_array_equal(r["ent_act_id"], cfg.act_ids[old])
    assert (r["ent_silo"].view(np.uint8).reshape(n, 24) == np.frombuffer(S.silo24(F.LOCAL_SILO), np.uint8)).all()
    assert r["inv"].tolist() == [S.INV_REMOVED] * (n // 2) + [S.INV_KEPT] * (n - n // 2)
    st, silo, act = b.route(keys)
    assert (st[:n // 2] == gd.ROUTE_MISS).all() and (st[n // 2:] == gd.ROUTE_OK).all()
    np.testing.assert_array_equal(act[n // 2:], new[n // 2:])
    b.close()
    c = receiver()                                           # what gd_cache_remove does on the same input
    assert c.cache_remove(r["ent_grain"]).all()
    assert (c.route(keys)[0] == gd.ROUTE_MISS).all()
    c.close()


# ----------------------------------------------------------------------------- the host forms
def test_host_forms_equal_the_device_forms(gd):
    sc = S.Scene(257, SEED + 257)
    buf, offs = sc.pack(b"\x01")
    e = _engine(gd, sc)
    cache = sc.new_cache()
    want = S.sniff_messages(buf, offs, cache)
    got = e.sniff_invalidate(buf, offs, ent_cap=want["m"] + 5)
    assert got["m"] == want["m"]
    for f in list(PER_FRAME) + list(PER_ENTRY) + ["inv"]:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    _same_cache(e, cache)
    # the first stage alone, in both forms, with optional outputs absent
    only = e.sniff_frames(buf, offs)
    for f in list(PER_FRAME) + list(PER_ENTRY):
        np.testing.assert_array_equal(only[f], want[f], err_msg=f)
    skip = ("flags", "ent_frame", "ent_silo", "ent_ext_off", "ent_act_id")
    dev, err = _dev(e, buf, offs, want["m"], chain=False, skip=skip + ("inv",))
    assert err is None
    _same(dev, want, chain=False, skip=skip)
    _same_cache(e, cache)                                    # the first stage touches no cache
    e.close()
