"""CPU tests of the forward writer's reference (tests/_forward_ref.py): the field form and the byte-run
form agree on randomized frames in serializer-normal form, the status order case by case, a frame computed by hand,
the frozen vectors of tests/golden/forward.json, the round trip 0 -> 1 -> 2 -> REJECT, and the C ABI's argument and
state checks that need no GPU."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import _forward_ref as F
import headers as H
from _encode_ref import Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "forward.json")
OK = (F.ST_OK_ADDRESSED, F.ST_OK_UNADDRESSED)

K = (7, 8, 0x0300000000000011)
IDS = np.array([[0, 0, 0], [11, 12, 13], [21, 22, 23], [31, 32, 33]], np.uint64)
CFG = Config(F.SILOS, F.TYPE_NAMES, IDS)
BASE = {"category": 2, "direction": 0, "correlation_id": 99, "target_grain": (K, None), "target_silo": F.SILOS[1],
        "target_activation": ((5, 6, 0), None), "sending_grain": ((1, 2, 0x0300000000000022), None)}


def _one(h, body=b"", kind=F.FWD_FORWARD, old_act=1, fwd=None, route=None, max_fc=2, local=F.LOCAL_SILO, cfg=CFG,
         form=F.forward_splice, frame=None):
    fr = H.encode_frame(h, body) if frame is None else frame
    fs, fa = (None, None) if fwd is None else fwd
    return form(fr, 0, kind, old_act, fs, fa, route, max_fc, local, cfg)


def _both(*a, **kw):
    s = _one(*a, form=F.forward_splice, **kw)
    f = _one(*a, form=F.forward_fields, **kw)
    assert s == f
    return s


@pytest.mark.parametrize("seed", range(4))
def test_forms_agree_on_random_batches(seed):
    rng = np.random.default_rng(700 + seed)
    cfg = F.make_config(rng)
    n = 600
    batch = F.random_batch(n, rng, cfg)
    routes = batch[6] if seed % 2 == 0 else None                     # with and without route results
    args = batch[:6] + (routes, None, F.MAX_FC, F.LOCAL_SILO, cfg)
    want = F.forward_batch(*args, form=F.forward_fields)
    assert np.isin(want[2], OK).sum() >= n // 2, "the batch has to exercise the writer"
    got = F.forward_batch(*args, form=F.forward_splice)
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[3], want[3])
    assert got[0] == want[0]
    assert set(want[2].tolist()) == set(range(8))
    # what the batch covers: 0..3 old entries, ForwardCount absent / 0 / 1 / 2 / -1, KeyExt and long-keyed targets,
    # with and without a forwarding address
    buf, offs = batch[0], batch[1]
    counts, fcs, exts = set(), set(), set()
    for i in range(n):
        if want[2][i] not in OK:
            continue
        o = int(offs[i])
        hl = struct.unpack_from("<i", buf, o)[0]
        h = F.parse_fields(buf[o:], hl)[0]
        counts.add(len(h.get("invalidation", [])))
        fcs.add(h.get("forward_count"))
        exts.add(h["target_grain"][1] is None)
    assert counts >= {0, 1, 2, 3} and fcs >= {None, 0, 1, -1} and exts == {True, False}
    assert (batch[4] == F.NONE32).any() and (batch[4] != F.NONE32).any()


def test_every_optional_field_present_and_absent():
    rng = np.random.default_rng(5)
    for p in (0.0, 1.0):
        for n_old in (0, 2):
            fr = F.normal_frame(rng, n_old=n_old, fc=1, p=p)
            for fwd in (None, (3, 2)):
                for route in (None, (0, 3, 0, 1, 2)):
                    a = _both(None, frame=fr, fwd=fwd, route=route)
                    assert a[0] == (F.ST_OK_UNADDRESSED if fwd is None and route is None else F.ST_OK_ADDRESSED)


def test_hand_computed_frame():
    """One long-keyed request, ForwardCount absent, no old entries, a forwarding address: every byte by hand."""
    st, out, tg = _both(BASE, b"BODY", old_act=1, fwd=(3, 2))
    assert st == F.ST_OK_ADDRESSED and tg == K
    mask = (H.CACHE_INVALIDATION_HEADER | H.CATEGORY | H.DIRECTION | H.FORWARD_COUNT | H.CORRELATION_ID |
            H.SENDING_GRAIN | H.TARGET_ACTIVATION | H.TARGET_GRAIN | H.TARGET_SILO)
    key = struct.pack("<QQQi", *K, -1)
    entry = H.w_silo(*F.SILOS[F.LOCAL_SILO]) + key + struct.pack("<QQQi", 11, 12, 13, -1)
    assert len(entry) == 80                                          # 24 + 28 + 28 for a long-keyed grain
    hdr = (struct.pack("<Ii", mask, 1) + entry + bytes([2, 0]) + struct.pack("<i", 1) + struct.pack("<q", 99) +
           struct.pack("<QQQi", 1, 2, 0x0300000000000022, -1) + struct.pack("<QQQi", 21, 22, 23, -1) + key +
           H.w_silo(*F.SILOS[3]))
    assert out == struct.pack("<ii", len(hdr), 4) + hdr + b"BODY"


def test_status_order():
    rc = dict(BASE, request_context=struct.pack("<i", 1) + b"\x08" * 11)
    assert _both(BASE, kind=F.FWD_NONE)[0] == F.ST_SKIPPED
    assert _both(BASE, kind=9)[0] == F.ST_SKIPPED
    # MALFORMED: lengths, a negative count, a walk off the header -- ahead of FALLBACK and of REJECT
    fr = bytearray(H.encode_frame(BASE, b""))
    struct.pack_into("<i", fr, 0, 3)
    assert _both(None, frame=bytes(fr))[0] == F.ST_MALFORMED
    assert _both(None, frame=b"\x10\x00\x00")[0] == F.ST_MALFORMED
    neg = dict(BASE, cache_invalidation=struct.pack("<i", -1), forward_count=9)
    assert _both(neg)[0] == F.ST_MALFORMED
    off = bytearray(H.encode_frame(dict(BASE, cache_invalidation=F.w_invalidation(F.rand_entries(
        np.random.default_rng(1), 2)), forward_count=9), b""))
    struct.pack_into("<i", off, 0, 100)                              # the header ends inside the second entry
    assert _both(None, frame=bytes(off) + b"\0" * 8)[0] == F.ST_MALFORMED
    cut = bytearray(H.encode_frame(dict(rc, debug_context="d" * 30), b""))
    struct.pack_into("<i", cut, 0, 12)                               # ... in front of RequestContext: splice only
    assert _one(None, frame=bytes(cut) + b"\0" * 64)[0] == F.ST_MALFORMED
    # FALLBACK ahead of REJECT and the address checks
    for h in (rc, dict(BASE, target_observer=b"\x01", transaction_info=b"\x02"),
              {k: v for k, v in BASE.items() if k != "target_grain"},
              dict(BASE, target_grain=((1, 2, 0x0100000000000005), None))):
        s = _both(dict(h, forward_count=9), old_act=99, fwd=(77, 99))
        assert s == (F.ST_FALLBACK, b"", F.NO_KEY)
    # REJECT ahead of NO_SILO / NO_ID; the key comes back
    assert _both(dict(BASE, forward_count=2), old_act=99, fwd=(77, 99)) == (F.ST_REJECT, b"", K)
    assert _both(dict(BASE, forward_count=1), max_fc=1)[0] == F.ST_REJECT
    assert _both(BASE, max_fc=0)[0] == F.ST_REJECT                   # absent counts as 0
    assert _both(dict(BASE, forward_count=-1), max_fc=0)[0] in OK    # a signed comparison
    # the appended entry's silo, then its id, then the written address' silo, then its id
    assert _both(BASE, old_act=0, local=9, fwd=(77, 99))[0] == F.ST_NO_SILO
    assert _both(BASE, old_act=0, fwd=(77, 99))[0] == F.ST_NO_ID     # all-zero row
    assert _both(BASE, old_act=4, fwd=(77, 99))[0] == F.ST_NO_ID     # past the map
    assert _both(BASE, old_act=1, fwd=(5, 99))[0] == F.ST_NO_SILO
    assert _both(BASE, old_act=1, fwd=(4, 0))[0] == F.ST_NO_ID
    assert _both(BASE, old_act=F.NONE32, local=9, fwd=(4, 1))[0] == F.ST_OK_ADDRESSED   # no append: local unused
    assert _both(BASE, route=(5, 9, 0, 0, None))[0] == F.ST_NO_SILO
    assert _both(BASE, route=(4, 0, 0, 0, None))[0] == F.ST_NO_ID
    assert _both(BASE, route=(9, 9, 1, 0, None))[0] == F.ST_OK_UNADDRESSED              # a miss: nothing is looked at
    assert _both(BASE, fwd=(4, 1), route=(9, 9, 0, 0, None))[0] == F.ST_OK_ADDRESSED    # the address wins


def test_fields_written():
    H_ = H
    m = lambda fr: struct.unpack_from("<I", fr, 8)[0]
    # ForwardCount -1 -> 0: field and bit dropped; IsNewPlacement removed with a forwarding address
    st, out, _ = _both(dict(BASE, forward_count=-1, is_new_placement=True), old_act=None, fwd=(0, 1))
    assert st == F.ST_OK_ADDRESSED and not m(out) & (H_.FORWARD_COUNT | H_.IS_NEW_PLACEMENT | H_.CACHE_INVALIDATION_HEADER)
    # unaddressed: TargetActivation and TargetSilo leave, IsNewPlacement stays
    st, out, _ = _both(dict(BASE, is_new_placement=True), old_act=None)
    assert st == F.ST_OK_UNADDRESSED and not m(out) & (H_.TARGET_ACTIVATION | H_.TARGET_SILO)
    assert m(out) & H_.IS_NEW_PLACEMENT and m(out) & H_.FORWARD_COUNT
    # SetTargetPlacement replaces the frame's NewGrainType and sets IsNewPlacement
    st, out, _ = _both(dict(BASE, new_grain_type="Old"), route=(0, 1, 0, 1, 2))
    h = F.parse_fields(out, struct.unpack_from("<i", out, 0)[0])[0]
    assert h["new_grain_type"] == F.TYPE_NAMES[2] and h["is_new_placement"] and h["forward_count"] == 1
    assert h["target_activation"] == ((11, 12, 13), None) and len(h["invalidation"]) == 1
    # a KeyExt TargetGrain is copied into the entry as it stands
    st, out, _ = _both(dict(BASE, target_grain=((1, 2, 0x0600000000000005), "ext-key")), route=None)
    h = F.parse_fields(out, struct.unpack_from("<i", out, 0)[0])[0]
    assert h["invalidation"][0][1] == ((1, 2, 0x0600000000000005), "ext-key")


def test_round_trip_twice_then_reject():
    fr = H.encode_frame(BASE, b"payload")
    st, f1, _ = _both(None, frame=fr, old_act=1, fwd=(3, 2))
    st2, f2, _ = _both(None, frame=f1, old_act=2, local=4)
    assert (st, st2) == (F.ST_OK_ADDRESSED, F.ST_OK_UNADDRESSED)
    h = F.parse_fields(f2, struct.unpack_from("<i", f2, 0)[0])[0]
    assert h["forward_count"] == 2 and f2.endswith(b"payload")
    assert [(e[0], e[2][0]) for e in h["invalidation"]] == [(H.w_silo(*F.SILOS[2]), (11, 12, 13)),
                                                              (H.w_silo(*F.SILOS[4]), (21, 22, 23))]
    assert all(e[1] == (K, None) for e in h["invalidation"])
    assert _both(None, frame=f2, old_act=3) == (F.ST_REJECT, b"", K)


def test_golden_vectors():
    """A few dozen frames frozen from the field form: both forms still give them."""
    g = json.load(open(GOLDEN))
    cfg = Config([bytes.fromhex(s) for s in g["silos"]], g["type_names"], np.array(g["act_ids"], np.uint64))
    assert len(g["vectors"]) >= 36
    for v in g["vectors"]:
        a = (bytes.fromhex(v["frame"]), 0, v["kind"], v["old_act"], v["fwd_silo"], v["fwd_act"],
             None if v["route"] is None else tuple(v["route"]), g["max_forward_count"], g["local_silo"], cfg)
        for form in (F.forward_fields, F.forward_splice):
            st, out, tg = form(*a)
            assert (st, out.hex(), list(tg)) == (v["status"], v["out"], v["target"])
    assert {v["status"] for v in g["vectors"]} == set(range(8))


def test_kinds():
    turn = np.arange(12, dtype=np.uint8)
    assert F.kinds_from_turns(turn).tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0]


def test_abi_without_a_gpu():
    from orleans_amd import graindispatch as g
    for s in ("gd_forward_kinds", "gd_forward_kinds_device", "gd_forward_frames", "gd_forward_frames_device",
              "gd_forward_send", "gd_forward_send_device"):
        assert s in g.EXPORTED_SYMBOLS and hasattr(g.lib, s)
    assert C.sizeof(g.gd_forward_batch) == 64
    fb = g.gd_forward_batch()
    off = C.c_uint64(0)
    # no handle: no gd_encode_configure
    assert g.lib.gd_forward_kinds(None, None, 0, None) == g.GD_ESTATE
    assert g.lib.gd_forward_frames(None, C.byref(fb), 0, None, None, None, None, None, None, None, 0, C.byref(off),
                                   None, None, None) == g.GD_ESTATE
    assert g.lib.gd_forward_send(None, C.byref(fb), 0, None, None, None, None, None, None, None, None, 0,
                                 C.byref(off), None, None, None) == g.GD_ESTATE
