"""The response writer's reference (_respond_ref.py) against itself and against hand-written answers, and the
declaration of the new entry points.  No GPU."""
import os
import re
import struct

import numpy as np

import _respond_ref as R
import headers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (7, 8, 0x0300000000000011)
K2 = (1, 2, 0x0300000000000022)
TA, SA = (5, 6, 0), (9, 9, 0)
BASE = {"category": 2, "direction": 0, "correlation_id": 99, "target_grain": (K, None), "target_silo": R.SILO2,
        "target_activation": (TA, None), "sending_grain": (K2, None), "sending_activation": (SA, None),
        "sending_silo": R.SILO, "resend_count": 1, "forward_count": 2, "is_new_placement": True,
        "new_grain_type": "Grains.Ping", "generic_grain_type": "[[T]]", "is_unordered": True}


def _both(fr, kind, result=0, rej=0, info=R.NO_INFO, body=b"", off=0):
    a = R.respond_splice(fr, off, kind, result, rej, info, body, R.INFOS)
    b = R.respond_reparse(fr, off, kind, result, rej, info, body, R.INFOS)
    assert a == b
    return a


def _answer(h, body=b""):
    return R.ST_OK, H.encode_frame(h, body)


def test_forms_agree_on_random_frames():
    rng = np.random.default_rng(5)
    batch = R.random_batch(2000, rng)
    a = R.respond_batch(*batch, None, R.INFOS)
    b = R.respond_batch(*batch, None, R.INFOS, form=R.respond_reparse)
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[0] == b[0]
    assert set(a[2].tolist()) == {0, 1, 2, 3, 4}
    frames = R.field_frames(1500, rng)
    for i, fr in enumerate(frames):
        _both(fr, 1 + i % 2, i % 3, i % 4, i % 6, b"b" * (i % 5))


def test_plain_request():
    want = {"category": 2, "direction": 1, "correlation_id": 99, "sending_grain": (K, None), "sending_silo": R.SILO2,
            "sending_activation": (TA, None), "target_grain": (K2, None), "target_activation": (SA, None),
            "target_silo": R.SILO}
    assert _both(H.encode_frame(BASE, b"request body"), R.RSP_RESPONSE, body=b"resp") == _answer(want, b"resp")
    assert _both(H.encode_frame(BASE), R.RSP_RESPONSE, result=1) == _answer(dict(want, result=1))
    assert _both(H.encode_frame(BASE), R.RSP_RESPONSE, result=2) == _answer(want)
    # the bytes themselves, once
    st, out = _both(H.encode_frame({"direction": 0, "correlation_id": 5}), R.RSP_RESPONSE, result=1, body=b"\xAA")
    mask = H.CORRELATION_ID | H.DIRECTION | H.RESULT
    assert out == struct.pack("<iiI", 4 + 1 + 8 + 1, 1, mask) + b"\x01" + struct.pack("<q", 5) + b"\x01" + b"\xAA"


def test_rejections():
    want = {"category": 2, "direction": 1, "correlation_id": 99, "sending_grain": (K, None), "sending_silo": R.SILO2,
            "sending_activation": (TA, None), "target_grain": (K2, None), "target_activation": (SA, None),
            "target_silo": R.SILO, "result": 2}
    fr = H.encode_frame(BASE)
    st, out = _both(fr, R.RSP_REJECTION, rej=R.REJ_TRANSIENT)             # the enum default: no RejectionType byte
    assert (st, out) == _answer(want)
    assert not struct.unpack_from("<I", out, 8)[0] & (H.REJECTION_TYPE | H.REJECTION_INFO)
    assert _both(fr, R.RSP_REJECTION, rej=R.REJ_OVERLOADED, info=0) == \
        _answer(dict(want, rejection_type=1, rejection_info="Overload2"))
    assert _both(fr, R.RSP_REJECTION, rej=3, info=1) == _answer(dict(want, rejection_type=3))      # the empty string
    assert _both(fr, R.RSP_REJECTION, rej=3, info=len(R.INFOS)) == _answer(dict(want, rejection_type=3))
    assert _both(fr, R.RSP_REJECTION, result=1, rej=0, info=2) == _answer(dict(want, rejection_info="x" * 40))
    # the request's own rejection fields do not survive
    old = H.encode_frame(dict(BASE, rejection_info="old", rejection_type=2, result=1))
    assert _both(old, R.RSP_RESPONSE) == _answer({k: v for k, v in want.items() if k != "result"})


def test_addresses():
    h = {k: v for k, v in BASE.items() if k != "sending_grain"}            # no SendingGrain: no TargetActivation
    st, out = _both(H.encode_frame(h), R.RSP_RESPONSE)
    m = struct.unpack_from("<I", out, 8)[0]
    assert st == R.ST_OK and not m & (H.TARGET_ACTIVATION | H.TARGET_GRAIN) and m & H.TARGET_SILO
    h = {k: v for k, v in BASE.items() if k != "target_grain"}             # no TargetGrain: no SendingActivation
    st, out = _both(H.encode_frame(h), R.RSP_RESPONSE)
    m = struct.unpack_from("<I", out, 8)[0]
    assert st == R.ST_OK and not m & (H.SENDING_ACTIVATION | H.SENDING_GRAIN) and m & H.SENDING_SILO
    # KeyExt strings on both grains travel with them
    h = dict(BASE, target_grain=(K, "target-ext"), sending_grain=(K2, ""), sending_activation=(SA, "a"))
    st, out = _both(H.encode_frame(h), R.RSP_RESPONSE)
    want = {"category": 2, "direction": 1, "correlation_id": 99, "sending_grain": (K, "target-ext"),
            "sending_silo": R.SILO2, "sending_activation": (TA, None), "target_grain": (K2, ""),
            "target_activation": (SA, "a"), "target_silo": R.SILO}
    assert (st, out) == _answer(want)
    # TargetObserver is dropped; the TargetSilo behind it is found at the header's end
    st, out = _both(H.encode_frame(dict(BASE, target_observer=b"\x07" * 13)), R.RSP_RESPONSE)
    assert (st, out) == _answer({k: v for k, v in want.items()} | {"sending_grain": (K, None),
                                                                    "target_grain": (K2, None),
                                                                    "target_activation": (SA, None)})


def test_tokens_context_and_tail():
    keep = {"direction": 1, "correlation_id": 99}
    req = {"direction": 0, "correlation_id": 99}
    assert _both(H.encode_frame(dict(req, read_only=False, always_interleave=True)), R.RSP_RESPONSE) == \
        _answer(dict(keep, always_interleave=True))                        # a False token: the bit is dropped
    assert _both(H.encode_frame(dict(req, read_only=True, always_interleave=False)), R.RSP_RESPONSE) == \
        _answer(dict(keep, read_only=True))
    assert _both(H.encode_frame(dict(req, category=0, debug_context="")), R.RSP_RESPONSE) == _answer(keep)
    assert _both(H.encode_frame(dict(req, debug_context=None)), R.RSP_RESPONSE) == _answer(keep)
    assert _both(H.encode_frame(dict(req, category=1, debug_context="ctx", time_to_live=-3)), R.RSP_RESPONSE) == \
        _answer(dict(keep, category=1, debug_context="ctx", time_to_live=-3))
    ti = b"\x05\x06\x07" * 3
    fr = H.encode_frame(dict(req, transaction_info=ti, is_using_interface_version=True, target_silo=R.SILO))
    assert _both(fr, R.RSP_REJECTION, rej=1) == \
        _answer(dict(keep, transaction_info=ti, sending_silo=R.SILO, result=2, rejection_type=1))
    assert _both(H.encode_frame({"correlation_id": 1}), R.RSP_RESPONSE)[0] == R.ST_OK       # no Direction: a request


def test_every_other_status():
    ok = H.encode_frame(BASE)
    assert _both(ok, R.RSP_NONE) == (R.ST_SKIPPED, b"")
    assert _both(ok, 9) == (R.ST_SKIPPED, b"")
    for d in (1, 2):                                                       # Response, OneWay
        assert _both(H.encode_frame(dict(BASE, direction=d)), R.RSP_REJECTION) == (R.ST_DISCARDED, b"")
    for extra in ({"cache_invalidation": struct.pack("<i", 1) + b"\x07" * 9},
                  {"request_context": struct.pack("<i", 1) + b"\x08" * 11},
                  {"target_observer": b"o" * 5, "transaction_info": b"t" * 5}):
        assert _both(H.encode_frame(dict(BASE, **extra)), R.RSP_RESPONSE) == (R.ST_FALLBACK, b"")
    st_key = (0, 9, (R.CAT_SYSTEM_TARGET << 56) | 12)
    h = {k: v for k, v in BASE.items() if k != "target_activation"}
    assert _both(H.encode_frame(dict(h, target_grain=(st_key, None))), R.RSP_RESPONSE) == (R.ST_FALLBACK, b"")
    assert _both(H.encode_frame(dict(BASE, target_grain=(st_key, None))), R.RSP_RESPONSE)[0] == R.ST_OK
    # DISCARDED is decided before FALLBACK where Direction can be read
    assert _both(H.encode_frame(dict(BASE, direction=1, request_context=b"\0" * 8)), R.RSP_RESPONSE)[0] == R.ST_DISCARDED
    # the decoder's length conditions
    assert _both(ok[:7], R.RSP_RESPONSE) == (R.ST_MALFORMED, b"")
    assert _both(ok[:-1], R.RSP_RESPONSE) == (R.ST_MALFORMED, b"")
    assert _both(ok, R.RSP_RESPONSE, off=len(ok) + 1) == (R.ST_MALFORMED, b"")
    bad = bytearray(ok)
    struct.pack_into("<i", bad, 4, -1)
    assert _both(bytes(bad), R.RSP_RESPONSE) == (R.ST_MALFORMED, b"")
    # a walk that leaves the header: before Direction, before TargetGrain's end, behind it
    hl = struct.unpack_from("<i", ok, 0)[0]
    for cut in (hl - 4, hl - 30, 4):
        short = bytearray(ok + b"\0" * 64)
        struct.pack_into("<i", short, 0, cut)
        assert _both(bytes(short), R.RSP_RESPONSE) == (R.ST_MALFORMED, b"")
    neg = bytearray(H.encode_frame(dict(BASE, debug_context="abc")))
    struct.pack_into("<i", neg, 13, -2)
    assert _both(bytes(neg), R.RSP_RESPONSE) == (R.ST_MALFORMED, b"")


def test_batch_order_offsets_and_helpers():
    rng = np.random.default_rng(6)
    batch = R.random_batch(200, rng)
    order = rng.permutation(200).astype(np.uint32)
    a = R.respond_batch(*batch, None, R.INFOS)
    b = R.respond_batch(*batch, order, R.INFOS)
    fr = lambda w, j: w[0][int(w[1][j]):int(w[1][j + 1])]
    for j in range(200):
        assert fr(b, j) == fr(a, int(order[j]))
    assert int(b[1][200]) == len(b[0]) == len(a[0])
    kind, rej = R.kinds_from_turns([R.TURN_REJECT_OVERLOADED, R.TURN_REJECT_TRANSIENT, R.TURN_START, R.TURN_NONE,
                                    R.TURN_NONE, R.TURN_REJECT_TRANSIENT],
                                   [0, 0, 0, R.RECV_REJECT_UNKNOWN, R.RECV_REJECT_OVERLOADED, R.RECV_REJECT_UNKNOWN])
    assert kind.tolist() == [2, 2, 0, 2, 2, 2] and rej.tolist() == [1, 0, 0, 3, 1, 0]
    assert R.kinds_from_turns([R.TURN_NONE, R.TURN_REJECT_OVERLOADED])[0].tolist() == [0, 2]
    table = [H.w_silo(*R.SILO), H.w_silo(*R.SILO2), H.w_silo(*R.SILO)]
    wire = np.frombuffer(table[1] + table[0] + bytes(24), np.uint8).reshape(3, 24)
    assert R.silo_index(wire, table).tolist() == [1, 0, R.NO_SILO]


def test_gpu_batches_are_mostly_written():
    """Every random batch the GPU tests use (test_gpu_respond.py: the seeds and sizes there): at least three
    quarters of the answered frames come out OK, so a writer that falls back everywhere cannot pass."""
    cases = [(200 + n, n) for n in (63, 64, 65, 257)] + [(21, 3000), (23, 300), (25, 500), (26, 2000)]
    for seed, n in cases:
        batch = R.random_batch(n, np.random.default_rng(seed))
        st = R.respond_batch(*batch, None, R.INFOS)[2]
        answered = (batch[2] == R.RSP_RESPONSE) | (batch[2] == R.RSP_REJECTION)
        assert (st[answered] == R.ST_OK).mean() >= 0.75, (seed, n)


def test_entry_points_declared_and_bound():
    from orleans_amd import graindispatch as g
    header = open(os.path.join(ROOT, "include", "graindispatch.h")).read()
    names = ["gd_respond_configure", "gd_respond_kinds_device", "gd_respond_kinds", "gd_silo_index_device",
             "gd_silo_index", "gd_respond_frames_device", "gd_respond_frames"]
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in g.EXPORTED_SYMBOLS and getattr(g.lib, name).argtypes is not None, name
    for c, v in (("GD_RSP_NONE", 0), ("GD_RSP_RESPONSE", 1), ("GD_RSP_REJECTION", 2), ("GD_RSPST_OK", 0),
                 ("GD_RSPST_SKIPPED", 1), ("GD_RSPST_MALFORMED", 2), ("GD_RSPST_DISCARDED", 3),
                 ("GD_RSPST_FALLBACK", 4)):
        assert re.search(r"#define\s+" + c + r"\s+" + str(v) + r"\b", header), c
        assert getattr(g, c[3:]) == v
    assert re.search(r"#define\s+GD_RSP_NO_INFO\s+0xFFFFFFFFu", header) and g.RSP_NO_INFO == R.NO_INFO
    for m in ("respond_configure", "respond_kinds", "respond_kinds_device", "silo_index", "silo_index_device",
              "respond_frames", "respond_frames_device"):
        assert callable(getattr(g.GrainDispatch, m)), m
