"""CPU checks of the frame-encoder reference (_encode_ref.py): its two forms agree on canonical frames, one
case per line of the rule (include/graindispatch.h, "frame encoder"), and one frame assembled byte by byte."""
import struct

import numpy as np
import pytest

import _encode_ref as R
import headers as H

K = (7, 8, 0x0300000000000011)
AID = (0x1111, 0x2222, 0x3333)
CFG = R.Config(R.SILOS, R.TYPE_NAMES, [[0, 0, 0], list(AID), [5, 6, 7]])
TA = struct.pack("<QQQi", *AID, -1)
TS = H.w_silo(*R.SILOS[2])
BASE = {"category": 2, "direction": 1, "correlation_id": 99, "target_grain": (K, None),
        "sending_silo": R.SILOS[0], "resend_count": 1}


def both(frame, silo=2, act=1, status=R.ROUTE_OK, placed=None, new_type=None, cfg=CFG, pad=b""):
    buf = pad + frame
    a = R.encode_splice(buf, len(pad), silo, act, status, placed, new_type, cfg)
    b = R.encode_reparse(buf, len(pad), silo, act, status, placed, new_type, cfg)
    assert a == b
    return a


def expect(h, body=b"", **set_fields):
    h = dict(h)
    h.update(set_fields)
    return H.encode_frame(h, body)


ADDR = {"target_activation": (AID, None), "target_silo": R.SILOS[2]}


def test_forms_agree_on_random_frames():
    rng = np.random.default_rng(5)
    cfg = R.make_config(rng)
    buf, offs, silo, act, status, placed, new_type = R.random_batch(3000, rng, cfg)
    a = R.encode_batch(buf, offs, silo, act, status, placed, new_type, None, cfg, R.encode_splice)
    b = R.encode_batch(buf, offs, silo, act, status, placed, new_type, None, cfg, R.encode_reparse)
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])
    assert set(np.unique(a[2]).tolist()) == set(range(7))          # every status occurs
    # the OK outputs decode as complete addresses carrying what was set
    for j in np.flatnonzero(a[2] == R.ENC_OK)[:200]:
        d = H.decode_frame(a[0], int(a[1][j]))
        assert d["flags"] & H.F_COMPLETE and not d["flags"] & H.F_MALFORMED
        assert d["target_activation"] == cfg.act_id(int(act[j]))
        if not d["flags"] & H.F_FALLBACK:
            assert d["target_silo"] == cfg.silos[int(silo[j])]


def test_insert_all_four():
    st, out = both(H.encode_frame(BASE, b"body"), placed=R.PLACED_NEW, new_type=0)
    assert st == R.ENC_OK
    assert out == expect(BASE, b"body", is_new_placement=True, new_grain_type="Grains.Ping", **ADDR)


def test_replace_all_four():
    h = dict(BASE, target_activation=((9, 9, 9), None), target_silo=R.SILOS[4], is_new_placement=True,
             new_grain_type="Old.Type")
    st, out = both(H.encode_frame(h, b"xy"), placed=R.PLACED_NEW, new_type=3)
    assert st == R.ENC_OK
    assert out == expect(BASE, b"xy", is_new_placement=True, new_grain_type="G", **ADDR)


def test_false_token_becomes_true():
    h = dict(BASE, always_interleave=False, is_new_placement=False, read_only=True, is_unordered=False)
    st, out = both(H.encode_frame(h), placed=R.PLACED_NEW)
    assert st == R.ENC_OK and out == expect(h, is_new_placement=True, **ADDR)


def test_not_new_keeps_the_frames_own_token():
    for own in (True, False):
        h = dict(BASE, is_new_placement=own)
        for placed in (None, 0, 2, 3):
            st, out = both(H.encode_frame(h), placed=placed)
            assert st == R.ENC_OK and out == expect(h, **ADDR)
    st, out = both(H.encode_frame(BASE), placed=2)
    assert out == expect(BASE, **ADDR)                             # absent stays absent


def test_type_empty_none_or_out_of_range_keeps_the_frames_own():
    for h in (BASE, dict(BASE, new_grain_type="Own.Type")):
        for nt in (None, R.NO_TYPE, 1, len(R.TYPE_NAMES)):         # index 1 is the empty string
            st, out = both(H.encode_frame(h), new_type=nt)
            assert st == R.ENC_OK and out == expect(h, **ADDR)
    st, out = both(H.encode_frame(dict(BASE, new_grain_type="Own.Type")), new_type=2)
    assert out == expect(BASE, new_grain_type=R.TYPE_NAMES[2], **ADDR)


def test_target_activation_with_keyext_is_replaced_whole():
    h = dict(BASE, target_activation=((1, 2, 3), "ext-of-the-old-id"))
    st, out = both(H.encode_frame(h, b"b"))
    assert st == R.ENC_OK and out == expect(BASE, b"b", **ADDR)


def test_target_observer_alone_puts_the_silo_at_the_header_end():
    h = dict(BASE, target_observer=b"\x07" * 13)
    st, out = both(H.encode_frame(h, b"zz"))
    assert st == R.ENC_OK and out == expect(h, b"zz", **ADDR)
    assert out[:-2].endswith(TS)
    h2 = dict(h, target_silo=R.SILOS[1])                           # and replaces the one standing there
    st, out2 = both(H.encode_frame(h2, b"zz"))
    assert st == R.ENC_OK and out2 == out


def test_transaction_info_stays_behind_the_silo():
    h = dict(BASE, transaction_info=b"\x05" * 9)
    st, out = both(H.encode_frame(h))
    assert st == R.ENC_OK and out == expect(h, **ADDR) and out.endswith(TS + b"\x05" * 9)


@pytest.mark.parametrize("extra", [{"target_observer": b"o" * 5, "transaction_info": b"t" * 5},
                                   {"request_context": struct.pack("<i", 0)},
                                   {"cache_invalidation": struct.pack("<i", 0)}])
def test_fallback(extra):
    assert both(H.encode_frame(dict(BASE, **extra))) == (R.ENC_FALLBACK, b"")


def test_statuses():
    fr = H.encode_frame(BASE, b"1234")
    for rs in (R.ROUTE_MISS, R.ROUTE_SYSTEM_TARGET, R.ROUTE_MEMBERSHIP, R.ROUTE_KEYEXT, R.ROUTE_UNDECODED,
               R.ROUTE_MULTI_ACT):
        assert both(fr, status=rs) == (R.ENC_SKIPPED, b"")
    full = H.encode_frame(dict(BASE, target_activation=((4, 4, 4), "k"), target_silo=R.SILOS[3]), b"1234")
    assert both(full, status=R.ROUTE_ADDRESSED, pad=b"\xee" * 3) == (R.ENC_COPIED, full)
    assert both(fr, silo=len(R.SILOS)) == (R.ENC_NO_SILO, b"")
    assert both(fr, act=0) == (R.ENC_NO_ID, b"")                   # all-zero id
    assert both(fr, act=3) == (R.ENC_NO_ID, b"")                   # past the map
    assert both(fr, silo=99, act=0) == (R.ENC_NO_SILO, b"")        # the order of the rule
    cut = bytearray(fr)
    struct.pack_into("<i", cut, 0, struct.unpack_from("<i", cut, 0)[0] - 20)
    assert both(bytes(cut)) == (R.ENC_MALFORMED, b"")              # the walk runs off the header
    assert both(fr[:-1]) == (R.ENC_MALFORMED, b"")                 # the frame runs off the buffer
    assert both(fr[:-1], status=R.ROUTE_ADDRESSED) == (R.ENC_MALFORMED, b"")
    assert both(fr[:5]) == (R.ENC_MALFORMED, b"")
    assert both(fr[:-1], status=R.ROUTE_MISS) == (R.ENC_SKIPPED, b"")
    neg = bytearray(H.encode_frame(dict(BASE, debug_context="abc")))
    struct.pack_into("<i", neg, 13, -2)                            # a string length below -1
    assert both(bytes(neg)) == (R.ENC_MALFORMED, b"")


def test_hand_assembled_frame():
    """No encoder on either side: mask 0x00100024 = Category | Direction | TargetGrain."""
    tg = struct.pack("<QQQi", 1, 2, 3, -1)
    src = struct.pack("<iiI", 4 + 1 + 1 + 28, 3, 0x00100024) + b"\x02" + b"\x01" + tg + b"abc"
    want_mask = 0x00100024 | (1 << 19) | (1 << 21) | (1 << 18) | (1 << 8)
    ngt = struct.pack("<i", 1) + b"G"
    want = (struct.pack("<iiI", 4 + 1 + 1 + 1 + 5 + 28 + 28 + 24, 3, want_mask) + b"\x02" + b"\x01" + b"\x03" + ngt +
            TA + tg + TS + b"abc")
    assert both(src, placed=R.PLACED_NEW, new_type=3, pad=b"\x00" * 5) == (R.ENC_OK, want)
    assert len(want) - len(src) == 28 + 24 + 1 + 5


def test_batch_layout_and_order():
    rng = np.random.default_rng(9)
    cfg = R.make_config(rng)
    buf, offs, silo, act, status, placed, new_type = R.random_batch(200, rng, cfg)
    out, off, est = R.encode_batch(buf, offs, silo, act, status, placed, new_type, None, cfg)
    order = rng.permutation(200).astype(np.uint32)
    out2, off2, est2 = R.encode_batch(buf, offs, silo, act, status, placed, new_type, order, cfg)
    np.testing.assert_array_equal(est, est2)                       # indexed by input frame
    assert int(off[200]) == len(out) == len(out2) == int(off2[200])
    for j, i in enumerate(order):
        assert out2[int(off2[j]):int(off2[j + 1])] == out[int(off[i]):int(off[i + 1])]
    assert R.encode_batch(b"", [], [], [], [], None, None, None, cfg)[1].tolist() == [0]
