"""The request writer's reference (_request_ref.py) against itself, against oracle/headers.py's decoder and against
hand-written answers; the draw of the GPU test's mixed batch; and the declaration of the new entry points.  No GPU."""
import os
import re
import struct

import numpy as np

import _request_ref as R
import headers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = R.tables()
K = (7, 8, 0x0300000000000011)
K2 = (1, 2, 0x0300000000000022)


def _one(target=K, sender=K2, sender_act=3, route=None, **kw):
    """A batch of one message; route = (silo, act, status[, placed[, new_type]])."""
    b = {"target": np.array([target], np.uint64), "sender_grain": np.array([sender], np.uint64),
         "sender_act": np.array([sender_act], np.uint32), "id_base": 99, "ttl_ticks": R.TTL_NONE}
    for k, v in kw.items():
        b[k] = v if k in ("id_base", "ttl_ticks", "body") else ([v] if k.endswith("_ext") else np.array([v]))
    if "body" in b:
        b["body_off"] = np.array([0, len(b["body"])], np.uint64)
    r = None
    if route is not None:
        names = ("silo", "act", "status", "placed", "new_type")
        r = {k: np.array([v]) for k, v in zip(names, route)}
    a, c = R.request_fields(b, r, 0, T), R.request_literal(b, r, 0, T)
    assert a == c
    return a


def test_forms_agree_on_random_batches():
    rng = np.random.default_rng(7)
    for n in (1500, 700):
        b, route = R.random_batch(n, rng, T)
        a = R.request_batch(b, route, None, T, form=R.request_fields)
        c = R.request_batch(b, route, None, T, form=R.request_literal)
        np.testing.assert_array_equal(a[2], c[2])
        np.testing.assert_array_equal(a[1], c[1])
        assert a[0] == c[0]
        assert set(a[2].tolist()) == {0, 1, 2, 3, 4}
    none = R.request_batch(b, None, None, T)                        # no route arrays: nothing is addressed
    assert set(none[2].tolist()) <= {R.ST_UNADDRESSED, R.ST_FALLBACK, R.ST_NO_ID}


def test_decode_returns_the_inputs():
    rng = np.random.default_rng(8)
    b, route = R.random_batch(800, rng, T)
    out, off, st = R.request_batch(b, route, None, T)
    seen = 0
    for i in range(800):
        if st[i] not in (R.ST_OK, R.ST_UNADDRESSED):
            assert off[i + 1] == off[i]
            continue
        seen += 1
        d = H.decode_frame(out, int(off[i]))
        opt = int(b["options"][i])
        assert d["flags"] & H.F_HAS_TARGET and not d["flags"] & (H.F_MALFORMED | H.F_FALLBACK)
        assert bool(d["flags"] & H.F_COMPLETE) == (st[i] == R.ST_OK)
        assert d["target_grain"] == tuple(int(x) for x in b["target"][i])
        assert d["sending_grain"] == tuple(int(x) for x in b["sender_grain"][i])
        assert d["sending_activation"] == T.act_id(int(b["sender_act"][i]))
        assert d["correlation_id"] == R._i64(b["id_base"] + i) and d["category"] == 2
        assert d["direction"] == (2 if opt & R.OPT_ONE_WAY else 0)
        ip, port, gen = T.silos[T.my_silo]
        assert d["sending_silo"] == ip + struct.pack("<ii", port, gen)
        x = b["target_ext"][i]
        assert d["target_ext"] == (None if x is None else x.encode())
        m = d["mask"]
        assert bool(m & H.TIME_TO_LIVE) == (not opt & (R.OPT_ONE_WAY | R.OPT_NO_TTL))
        assert bool(m & H.READ_ONLY) == bool(opt & R.OPT_READ_ONLY)
        assert bool(m & H.ALWAYS_INTERLEAVE) == bool(opt & R.OPT_ALWAYS_INTERLEAVE)
        assert bool(m & H.IS_UNORDERED) == bool(opt & R.OPT_UNORDERED)
        if st[i] == R.ST_OK:
            assert d["target_activation"] == T.act_id(int(route["act"][i]))
            ip, port, gen = T.silos[int(route["silo"][i])]
            assert d["target_silo"] == ip + struct.pack("<ii", port, gen)
            assert bool(m & H.IS_NEW_PLACEMENT) == (int(route["placed"][i]) == R.PLACED_NEW)
        hl, bl = struct.unpack_from("<ii", out, int(off[i]))
        assert out[int(off[i]) + 8 + hl:int(off[i + 1])] == R._body(b, i) and bl == len(R._body(b, i))
    assert seen > 400


BASE_MASK = H.CATEGORY | H.DIRECTION | H.CORRELATION_ID | H.SENDING_ACTIVATION | H.SENDING_GRAIN | H.SENDING_SILO | \
    H.TARGET_GRAIN
ADDR = H.TARGET_ACTIVATION | H.TARGET_SILO


def _mask(fr):
    return struct.unpack_from("<I", fr, 8)[0]


def test_mask_table():
    ok = (2, 7, R.ROUTE_OK)
    cases = [
        (dict(), BASE_MASK, R.ST_UNADDRESSED),
        (dict(route=ok), BASE_MASK | ADDR, R.ST_OK),
        (dict(route=(2, 7, R.ROUTE_MISS, R.PLACED_NEW, 0)), BASE_MASK, R.ST_UNADDRESSED),
        (dict(route=ok + (R.PLACED_NEW, 0)), BASE_MASK | ADDR | H.IS_NEW_PLACEMENT | H.NEW_GRAIN_TYPE, R.ST_OK),
        (dict(route=ok + (2, 1)), BASE_MASK | ADDR, R.ST_OK),       # joined; an empty type string
        (dict(ttl_ticks=5), BASE_MASK | H.TIME_TO_LIVE, R.ST_UNADDRESSED),
        (dict(ttl_ticks=5, options=R.OPT_ONE_WAY), BASE_MASK, R.ST_UNADDRESSED),
        (dict(ttl_ticks=5, options=R.OPT_NO_TTL), BASE_MASK, R.ST_UNADDRESSED),
        (dict(options=R.OPT_ALWAYS_INTERLEAVE | R.OPT_READ_ONLY | R.OPT_UNORDERED),
         BASE_MASK | H.ALWAYS_INTERLEAVE | H.READ_ONLY | H.IS_UNORDERED, R.ST_UNADDRESSED),
        (dict(options=R.OPT_IFACE_VERSION | R.OPT_TXN_REQUIRED), BASE_MASK | (1 << 26) | (1 << 28), R.ST_UNADDRESSED),
        (dict(debug=0, generic=2), BASE_MASK | H.DEBUG_CONTEXT | H.GENERIC_GRAIN_TYPE, R.ST_UNADDRESSED),
        (dict(debug=1, generic=99), BASE_MASK, R.ST_UNADDRESSED),   # an empty string; an index past the table
    ]
    for kw, mask, st in cases:
        got = _one(**kw)
        assert got[0] == st and _mask(got[1]) == mask, kw


def test_status_order():
    sys_target = (1, 2, 0x0100000000000005)
    assert _one(target_ext=R.KEYEXT_HOST, target=sys_target, sender_act=5)[0] == R.ST_FALLBACK
    assert _one(sender_ext=R.KEYEXT_HOST)[0] == R.ST_FALLBACK
    assert _one(target=sys_target, sender_act=5) == (R.ST_FALLBACK, b"")
    assert _one(sender_act=5, route=(9, 7, 0)) == (R.ST_NO_ID, b"")          # act 5 has no ActivationId
    assert _one(sender_act=R.N_ACT, route=(2, 7, 0))[0] == R.ST_NO_ID
    assert _one(route=(5, 5, 0))[0] == R.ST_NO_SILO                           # the silo before the target's id
    assert _one(route=(4, 5, 0))[0] == R.ST_NO_ID
    assert _one(route=(5, 5, 1))[0] == R.ST_UNADDRESSED                       # a miss reads neither


def test_one_frame_by_hand():
    """Addressed, one-way off, ttl 0x0102030405060708, ReadOnly, new placement of "Grains.Ping", DebugContext "ctx",
    a KeyExt "ab" on the target, body "xyz"; sender activation 3, target activation 7 on silo 2, my silo 1."""
    got = _one(route=(2, 7, 0, R.PLACED_NEW, 0), ttl_ticks=0x0102030405060708, options=R.OPT_READ_ONLY, debug=0,
               target_ext="ab", body=b"xyz")
    sa = struct.pack("<QQQ", 0x1111000000000000 + 3 * 977, 0xABCD00000000 + 3, 0x0400000000000000)
    ta = struct.pack("<QQQ", 0x1111000000000000 + 7 * 977, 0xABCD00000000 + 7, 0x0400000000000000)
    # mask bits: 2 Category, 3 CorrelationId, 4 DebugContext, 5 Direction, 6 TimeToLive, 8 NewGrainType,
    # 13 ReadOnly, 15-17 Sending*, 18 IsNewPlacement, 19-21 Target*
    assert 0x003FA17C == sum(1 << k for k in (2, 3, 4, 5, 6, 8, 13, 15, 16, 17, 18, 19, 20, 21))
    hdr = (bytes([0x7C, 0xA1, 0x3F, 0x00])
           + b"\x02" + b"\x03\x00\x00\x00ctx" + b"\x00" + bytes([8, 7, 6, 5, 4, 3, 2, 1])
           + bytes([99, 0, 0, 0, 0, 0, 0, 0]) + b"\x03\x03"
           + b"\x0b\x00\x00\x00Grains.Ping"
           + sa + b"\xff\xff\xff\xff"
           + struct.pack("<QQQ", *K2) + b"\xff\xff\xff\xff"
           + bytes(12) + bytes([10, 0, 0, 2]) + struct.pack("<ii", 11001, 107)
           + ta + b"\xff\xff\xff\xff"
           + struct.pack("<QQQ", *K) + b"\x02\x00\x00\x00ab"
           + bytes(12) + bytes([10, 0, 0, 3]) + struct.pack("<ii", 11002, 114))
    want = struct.pack("<ii", len(hdr), 3) + hdr + b"xyz"
    assert got == (R.ST_OK, want)
    assert len(hdr) == 4 + 1 + 7 + 1 + 8 + 8 + 2 + 15 + 28 + 28 + 24 + 28 + 30 + 24


def test_batch_order_and_offsets():
    rng = np.random.default_rng(9)
    b, route = R.random_batch(200, rng, T)
    order = rng.permutation(200).astype(np.uint32)
    plain = R.request_batch(b, route, None, T)
    out, off, st = R.request_batch(b, route, order, T)
    np.testing.assert_array_equal(st, plain[2])
    for j, i in enumerate(order):
        assert out[int(off[j]):int(off[j + 1])] == plain[0][int(plain[1][i]):int(plain[1][i + 1])]
    ttl = R.send_ttl(b)
    opt = b["options"]
    assert ((ttl == R.TTL_NONE) == ((opt & 3) != 0)).all() and R.send_ttl(dict(b, ttl_ticks=R.TTL_NONE)) is None


def test_gpu_mixed_batch_draw():
    """The mixed batch of test_gpu_request.py (seed 31, n = 3,000): the shares the draw aims at, every status, and
    fewer than half the messages non-OK, so the byte comparison there cannot be empty."""
    b, route = R.random_batch(3000, np.random.default_rng(31), T)
    st = R.request_batch(b, route, None, T)[2]
    n = 3000
    assert (st != R.ST_OK).sum() < n // 2
    assert set(st.tolist()) == {0, 1, 2, 3, 4}
    share = lambda m: m.sum() / n
    assert 0.07 < share(route["status"] != R.ROUTE_OK) < 0.13
    assert 0.015 < share((b["target"][:, 2] >> np.uint64(56)) == 1) < 0.045
    assert 0.008 < share(np.array([T.act_id(int(a)) is None for a in b["sender_act"]])) < 0.035
    assert 0.008 < share(route["silo"] >= len(T.silos)) < 0.035
    for exts in (b["target_ext"], b["sender_ext"]):
        lens = [len(x) for x in exts if isinstance(x, str)]
        assert 0.07 < len(lens) / n < 0.13 and set(lens) == {0, 1, 63, 300}
        assert 1 <= sum(1 for x in exts if isinstance(x, int)) < 60


def test_entry_points_declared_and_bound():
    from orleans_amd import graindispatch as g
    header = open(os.path.join(ROOT, "include", "graindispatch.h")).read()
    names = ["gd_request_configure", "gd_request_frames_device", "gd_request_frames", "gd_request_send_device",
             "gd_request_send"]
    for name in names:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in g.EXPORTED_SYMBOLS and getattr(g.lib, name).argtypes is not None, name
    consts = [("GD_REQ_ONE_WAY", R.OPT_ONE_WAY), ("GD_REQ_NO_TTL", R.OPT_NO_TTL),
              ("GD_REQ_ALWAYS_INTERLEAVE", R.OPT_ALWAYS_INTERLEAVE), ("GD_REQ_READ_ONLY", R.OPT_READ_ONLY),
              ("GD_REQ_UNORDERED", R.OPT_UNORDERED), ("GD_REQ_IFACE_VERSION", R.OPT_IFACE_VERSION),
              ("GD_REQ_TXN_REQUIRED", R.OPT_TXN_REQUIRED), ("GD_REQ_OK", R.ST_OK),
              ("GD_REQ_UNADDRESSED", R.ST_UNADDRESSED), ("GD_REQ_FALLBACK", R.ST_FALLBACK),
              ("GD_REQ_NO_ID", R.ST_NO_ID), ("GD_REQ_NO_SILO", R.ST_NO_SILO)]
    for c, v in consts:
        m = re.search(r"#define " + c + r"\s+(\d+)u?\b", header)
        assert m and int(m.group(1)) == v, c
        assert getattr(g, c[3:]) == v, c
    assert C_sizeof_batch(g) == 96


def C_sizeof_batch(g):
    import ctypes
    return ctypes.sizeof(g.gd_request_batch)
