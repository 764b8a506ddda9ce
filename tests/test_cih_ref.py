"""The two forms of the GD_OPT_WALK_INVALIDATION reference (tests/_cih_ref.py) agree: the direct walker (form A)
and the cut-and-reuse form (form B) give the same decoder outputs, encoder frames and answers on the batches the
GPU tests use, and the fixtures hold the cases those tests name."""
import struct

import numpy as np
import pytest

import headers as H
import _cih_ref as X
import _encode_ref as E
import _forward_ref as F
import _respond_ref as R


def _batches():
    rng = np.random.default_rng(1805)
    out = [X.mixed_batch(n, rng) for n in (1, 63, 64, 65, 257)]
    out += [X.edge_frames(rng, a)[:2] for a in range(4)]
    return out


@pytest.fixture(scope="module")
def batches():
    return _batches()


def test_decoder_forms_agree(batches):
    seen = set()
    for buf, offs in batches:
        for o in offs:
            a, b = X.decode_walk(buf, int(o)), X.decode_cut(buf, int(o))
            assert a == b, (int(o), {k: (a[k], b[k]) for k in a if a[k] != b[k]})
            seen.add(a["flags"])
    inv = X.F_INVALIDATION
    assert inv | H.F_HAS_TARGET in seen and inv | H.F_HAS_TARGET | H.F_TARGET_KEYEXT in seen
    assert inv | H.F_FALLBACK in seen and H.F_MALFORMED in seen and H.F_HAS_TARGET in seen
    assert any(f & inv and f & H.F_FALLBACK and f & H.F_HAS_TARGET for f in seen)        # TargetObserver


def test_without_the_field_the_references_are_unchanged(batches):
    buf, offs = batches[4]
    for o in offs:
        o = int(o)
        if X.frame_lengths(buf, o) and not struct.unpack_from("<I", buf, o + 8)[0] & X.CIH:
            a = X.decode_walk(buf, o)
            want = H.decode_frame(buf, o)
            assert all(a[k] == want[k] for k in want)


def test_tg_ext_off_is_absolute(batches):
    n = 0
    for buf, offs in batches:
        for o in offs:
            a = X.decode_walk(buf, int(o))
            if a["tg_ext_off"] is not None:
                ext = a["target_ext"]
                assert bytes(buf[a["tg_ext_off"]:a["tg_ext_off"] + len(ext)]) == ext
                n += a["flags"] & X.F_INVALIDATION != 0
    assert n > 20


def test_encoder_forms_agree(batches):
    rng = np.random.default_rng(7)
    cfg = E.make_config(rng)
    st_seen = set()
    for buf, offs in batches:
        n = len(offs)
        silo = rng.integers(0, len(cfg.silos), size=n)
        act = rng.integers(0, len(cfg.act_ids), size=n)
        placed = rng.integers(0, 3, size=n)
        ntype = rng.integers(0, len(cfg.type_names) + 1, size=n)
        status = rng.choice([E.ROUTE_OK, E.ROUTE_ADDRESSED, E.ROUTE_MISS], size=n, p=[0.85, 0.1, 0.05])
        for i, o in enumerate(offs):
            args = (buf, int(o), int(silo[i]), int(act[i]), int(status[i]), int(placed[i]), int(ntype[i]), cfg)
            a, b = X.encode_walk(*args), X.encode_cut(*args)
            assert a == b, int(o)
            m = struct.unpack_from("<I", buf, int(o) + 8)[0] if X.frame_lengths(buf, int(o)) else 0
            st_seen.add((a[0], bool(m & X.CIH)))
            if a[0] == E.ENC_OK and m & X.CIH:             # the field is carried through in front of Category
                src = X.cut_frame(buf, int(o))[1]
                assert a[1][12:12 + len(src)] == src and struct.unpack_from("<I", a[1], 8)[0] & X.CIH
                assert X.decode_walk(a[1], 0)["flags"] & (H.F_COMPLETE | X.F_INVALIDATION) == H.F_COMPLETE | X.F_INVALIDATION
    assert {(E.ENC_OK, True), (E.ENC_FALLBACK, True), (E.ENC_MALFORMED, True), (E.ENC_COPIED, True)} <= st_seen


def test_responder_forms_agree(batches):
    rng = np.random.default_rng(8)
    seen = set()
    for buf, offs in batches:
        for o in offs:
            o = int(o)
            kind = int(rng.choice([R.RSP_RESPONSE, R.RSP_REJECTION, R.RSP_NONE], p=[0.5, 0.45, 0.05]))
            args = (buf, o, kind, int(rng.integers(0, 2)), int(rng.integers(0, 4)), int(rng.integers(0, 5)),
                    bytes(rng.integers(0, 256, size=int(rng.integers(0, 20)), dtype=np.uint8)), R.INFOS)
            a, b = X.respond_walk(*args), X.respond_cut(*args)
            assert a == b, o
            if X.frame_lengths(buf, o) is None or not struct.unpack_from("<I", buf, o + 8)[0] & X.CIH:
                continue
            try:
                _, field, count = X.cut_frame(buf, o)
            except X.Bad:
                continue
            seen.add((a[0], min(count, 1)))
            if a[0] == R.ST_OK:
                om = struct.unpack_from("<I", a[1], 8)[0]
                if count:                                  # the same entries, byte for byte, behind the mask
                    assert om & X.CIH and a[1][12:12 + len(field)] == field
                else:                                      # no list is built: the bit is dropped
                    assert not om & X.CIH
    assert {(R.ST_OK, 0), (R.ST_OK, 1), (R.ST_FALLBACK, 1), (R.ST_DISCARDED, 1)} <= seen


def test_default_category_case():
    """The one frame the responder leaves to C# although its field can be walked: count > 0, a Category byte of the
    enum's default and a non-empty DebugContext.  Its neighbours are answered."""
    rng = np.random.default_rng(3)
    go = lambda fr: X.respond_walk(fr, 0, R.RSP_RESPONSE, 0, 0, R.NO_INFO, b"", R.INFOS)
    assert go(X.request(rng, count=1, category=0, debug="kept"))[0] == R.ST_FALLBACK
    for kw in (dict(count=1, category=0), dict(count=1, category=0, debug=""), dict(count=0, category=0, debug="kept"),
               dict(count=1, category=None, debug="kept"), dict(count=1, category=2, debug="kept")):
        fr = X.request(rng, **kw)
        st, out = go(fr)
        assert st == R.ST_OK and X.respond_cut(fr, 0, R.RSP_RESPONSE, 0, 0, R.NO_INFO, b"", R.INFOS) == (st, out)
        assert not struct.unpack_from("<I", out, 8)[0] & H.CATEGORY or kw["category"] == 2


def test_malformed_fields():
    rng = np.random.default_rng(4)
    cfg = E.make_config(rng)
    for fr in X.malformed(rng):
        assert X.decode_walk(fr, 0)["flags"] == H.F_MALFORMED == X.decode_cut(fr, 0)["flags"]
        assert X.encode_walk(fr, 0, 0, 1, E.ROUTE_OK, 0, E.NO_TYPE, cfg)[0] == E.ENC_MALFORMED
        assert X.respond_walk(fr, 0, R.RSP_RESPONSE, 0, 0, R.NO_INFO, b"", R.INFOS)[0] == R.ST_MALFORMED
    # the last frame of a buffer whose length is no multiple of 4 decodes; one byte short it does not
    buf, offs = X.unaligned_tail(rng)
    assert len(buf) % 4 and X.decode_walk(buf, int(offs[1]))["flags"] & H.F_HAS_TARGET
    assert X.decode_walk(buf[:-1], int(offs[1]))["flags"] == H.F_MALFORMED


def test_edge_frames_cover_the_window():
    rng = np.random.default_rng(5)
    for a in range(4):
        _, offs, what = X.edge_frames(rng, a)
        assert {(t, b) for t, b, _ in what} == {(t, b) for t in ("entry_end", "tg_first", "tg_last")
                                                for b in (191, 192, 193)}
        assert len(offs) == len(what)
