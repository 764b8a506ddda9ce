"""The reference walk of the turn headers (tests/_frame_turns_ref.py) against what oracle/headers.py's encoder was
given, against decode_frame's flags and mask, and the clamp / saturation rules of DESIGN 5.21.  CPU only."""
import itertools
import struct

import numpy as np
import pytest

import headers as H
import oracle as o
import _frame_turns_ref as F
import _turns_ref as T

I64_MAX, I64_MIN, I32_MAX = (1 << 63) - 1, -(1 << 63), (1 << 31) - 1
TG = ((0, 5, 0x0300000000000001), None)
BASE = {"category": 2, "direction": 0, "correlation_id": 9, "target_grain": TG,
        "target_activation": ((3, 4, 0), None), "target_silo": F.SILO}

# name -> (a value to write, the gd_frame_turn_fields member, what the walk gives for it)
FIELDS = {"time_to_live": (123456789012, "ttl", 123456789012), "forward_count": (2, "forward_count", 2),
          "result": (2, "result", 2), "rejection_type": (4, "rejection_type", 4), "resend_count": (7, "resend_count", 7)}


def _walk(h, body=b"xyz"):
    fr = H.encode_frame(h, body)
    r = F.walk_frame(fr, 0)
    d = H.decode_frame(fr, 0)
    assert r["flags"] & ~H.F_TARGET_KEYEXT == d["flags"] & ~H.F_TARGET_KEYEXT and r["mask"] == d["mask"]
    return r


@pytest.mark.parametrize("present", list(itertools.product([False, True], repeat=len(FIELDS))))
def test_every_field_present_or_absent(present):
    h = dict(BASE)
    want = dict(F.ABSENT)
    for (name, (v, member, got)), p in zip(FIELDS.items(), present):
        if p:
            h[name] = v
            want[member] = got
    r = _walk(h)
    assert {k: r[k] for k in want} == want


@pytest.mark.parametrize("ai,ro,np_,un", list(itertools.product([None, False, True], repeat=4)))
def test_both_bool_tokens_in_every_combination(ai, ro, np_, un):
    """None = header absent.  A bit set with a False token reads 0; IsNewPlacement / IsUnordered only shift the
    bytes."""
    h = dict(BASE)
    for name, v in (("always_interleave", ai), ("read_only", ro), ("is_new_placement", np_), ("is_unordered", un)):
        if v is not None:
            h[name] = v
    want = (T.MSG_ALWAYS_INTERLEAVE if ai else 0) | (T.MSG_READ_ONLY if ro else 0)
    assert _walk(h)["msg_flags"] == want


def test_a_bool_byte_that_is_neither_token_reads_false():
    h = dict(BASE, always_interleave=True, read_only=True)
    fr = bytearray(H.encode_frame(h))
    # the two token bytes follow the correlation id: category 1 + direction 1 + correlation id 8 after the mask
    assert fr[12 + 10] == fr[12 + 11] == H.TRUE_TOKEN and F.walk_frame(bytes(fr), 0)["msg_flags"] == 3
    for tok in (0, 1, 2, 4, 5, 255):
        g = bytearray(fr)
        g[12 + 10], g[12 + 11] = tok, H.TRUE_TOKEN
        assert F.walk_frame(bytes(g), 0)["msg_flags"] == T.MSG_READ_ONLY
        g[12 + 10], g[12 + 11] = H.TRUE_TOKEN, tok
        assert F.walk_frame(bytes(g), 0)["msg_flags"] == T.MSG_ALWAYS_INTERLEAVE


@pytest.mark.parametrize("written,want", [(-1, 0), (0, 0), (255, 255), (256, 255), (I32_MAX, 255), (-(1 << 31), 0)])
def test_forward_count_clamps(written, want):
    assert _walk(dict(BASE, forward_count=written))["forward_count"] == want


@pytest.mark.parametrize("ttl", [I64_MAX, 0, -1, I64_MIN, 1])
@pytest.mark.parametrize("age", [0, 1, 10_000_000, I64_MAX])
def test_ttl_as_written_and_aged(ttl, age):
    r = _walk(dict(BASE, time_to_live=ttl))
    assert r["ttl"] == ttl                                   # as written, INT64_MAX colliding with TTL_NONE
    aged = int(F.aged_ttl(np.array([r["ttl"]], np.int64), age)[0])
    if ttl == I64_MAX:
        assert aged == I64_MAX                               # "no value": never ages
    else:
        assert aged == max(ttl - age, I64_MIN)               # saturates, never wraps
    if ttl == I64_MIN and age > 0:
        assert aged == I64_MIN
    # the turn stage's IsExpired on it
    b = T.Batch([0], 1, [0], [0], [0], ttl=[aged])
    assert (T.turns_loop(b)[0][0] == T.TURN_EXPIRED) == (ttl != I64_MAX and ttl - age <= 0)


def test_absent_ttl_stays_none_whatever_the_age():
    assert _walk(BASE)["ttl"] == I64_MAX
    assert int(F.aged_ttl(np.array([I64_MAX], np.int64), 5)[0]) == I64_MAX


def test_fallback_and_malformed_read_absent_observer_reads_decoded():
    full = dict(BASE, time_to_live=5, forward_count=1, read_only=True, always_interleave=True, result=1,
                rejection_type=2, resend_count=3)
    dec = {"ttl": 5, "forward_count": 1, "msg_flags": 3, "result": 1, "rejection_type": 2, "resend_count": 3}
    r = _walk(full)
    assert {k: r[k] for k in dec} == dec
    for extra in ({"request_context": b"\x01\x00\x00\x00" + bytes(8)}, {"cache_invalidation": struct.pack("<i", 0)}):
        r = _walk(dict(full, **extra))
        assert r["flags"] & H.F_FALLBACK and {k: r[k] for k in dec} == F.ABSENT
    r = _walk(dict(full, target_observer=bytes(20)))
    assert r["flags"] & H.F_FALLBACK and {k: r[k] for k in dec} == dec
    fr = bytearray(H.encode_frame(full, b"body"))
    hl = struct.unpack_from("<i", fr, 0)[0]
    for cut in range(4, hl):                                 # every header length short of the real one
        struct.pack_into("<i", fr, 0, cut)
        r = F.walk_frame(bytes(fr), 0)
        assert r["flags"] == H.F_MALFORMED and r["mask"] == 0 and {k: r[k] for k in dec} == F.ABSENT, cut


def test_agrees_with_decode_frame_on_random_frames():
    rng = np.random.default_rng(5)
    n = 3000
    tg = o.grain_keys(o.grain_type_code(o.PING_GRAIN_CLASS), rng.integers(0, 1000, size=n))
    buf, off = H.random_frames(n, tg, rng, p_malformed=0.05)
    f = H.decode_frames(buf, off)
    t = F.walk_frames(buf, off)
    np.testing.assert_array_equal(t["flags"], f["flags"])
    np.testing.assert_array_equal(t["mask"], f["mask"])
    for k, dt in F.TURN_FIELDS.items():
        assert t[k].dtype == dt and t[k].shape == (n,)
    dead = (f["flags"] & H.F_MALFORMED) != 0
    dead |= (f["mask"] & (H.REQUEST_CONTEXT | H.CACHE_INVALIDATION_HEADER)) != 0
    for k, v in F.ABSENT.items():
        assert (t[k][dead] == v).all()
    assert dead.sum() > 50 and (t["ttl"] != F.TTL_NONE).sum() > 100 and t["msg_flags"].any()


def test_chain_ref_composes_the_stage_references():
    """Undecoded frames: RECV_UNDECODED, TURN_NONE, outside every count; msg_flags_or and the age reach the turn
    rule."""
    rng = np.random.default_rng(8)
    n, n_ctx = 600, 5
    aid = np.zeros((n_ctx, 3), np.uint64)
    aid[:, 0] = np.arange(1, n_ctx + 1)
    which = rng.integers(0, n_ctx, n)
    tg = o.grain_keys(o.grain_type_code(o.PING_GRAIN_CLASS), rng.integers(0, 50, size=n))
    ta = aid[which]
    sa = ta.copy()
    sa[::2, 1] = 77
    direction = rng.choice(np.array([0, 1, 2, 0xFF], np.uint8), size=n)
    buf, off = F.chain_frames(rng, tg, ta, sa, direction)
    ctxs, adf = np.arange(n_ctx, dtype=np.uint32), np.ones(n_ctx, np.uint8)
    fl, nr = np.zeros(n_ctx, np.uint8), np.zeros(n_ctx, np.uint32)
    rc = np.full(n_ctx, 1000, np.uint32)
    base = F.chain_ref(buf, off, aid, ctxs, adf, n_ctx, fl, nr, rc)
    f, t, st, ctx, turn = base[0], base[1], base[2], base[3], base[6]
    und = st == F.RECV_UNDECODED
    assert und.sum() > 20 and not turn[und].any() and (ctx[und] == 0xFFFFFFFF).all()
    np.testing.assert_array_equal(ctx[~und], which[~und])
    live = ~und & (direction != 1)
    exp0 = live & (t["ttl"] != F.TTL_NONE) & (t["ttl"] <= 0)
    np.testing.assert_array_equal(turn[live] == T.TURN_EXPIRED, exp0[live])
    aged = F.chain_ref(buf, off, aid, ctxs, adf, n_ctx, fl, nr, rc, ttl_age_ticks=51)[6]
    exp51 = live & (t["ttl"] != F.TTL_NONE) & (t["ttl"] <= 51)
    np.testing.assert_array_equal(aged[live] == T.TURN_EXPIRED, exp51[live])
    assert exp51.sum() > exp0.sum() > 0
    may = np.full(n, T.MSG_MAY_INTERLEAVE, np.uint8)
    ored = F.chain_ref(buf, off, aid, ctxs, adf, n_ctx, fl, nr, rc, msg_flags_or=may)[6]
    assert (ored[live & ~exp0] == T.TURN_START).all() and (turn[live & ~exp0] == T.TURN_WAIT).any()
