"""The turn headers of a frame, restated per frame from HeadersContainer.Deserializer (src/Orleans.Core/Messaging/
Message.cs:1247-1356), and the frame-fed chain composed from the stage references: decode -> oracle/receive.py's
IncomingMessageAgent.ReceiveMessage -> _turns_ref.turns_loop (Dispatcher.ReceiveRequest).  Checker for
gd_decode_frames_turn* and gd_receive_turns_frames* (DESIGN 5.21); constants mirror include/graindispatch.h.

Field rules (gd_frame_turn_fields):
  * a bool is true iff its byte is SerializationTokenType.True (ReadBool, Message.cs:1358-1361);
  * a MALFORMED frame, and a FALLBACK one with CacheInvalidationHeader / RequestContext, reads absent in every
    field; a frame that is FALLBACK only for its TargetObserver has them decoded (they precede it on the wire);
  * ForwardCount is clamped to [0, 255]; an absent TimeToLive is TTL_NONE (= TimeSpan.MaxValue, "never expires").
"""
import struct

import numpy as np

import headers as H
import receive as RV
import _turns_ref as T

TTL_NONE = T.TTL_NONE
I64_MIN = int(np.iinfo(np.int64).min)
RECV_UNDECODED = 6
MSG_READ_ONLY, MSG_ALWAYS_INTERLEAVE, MSG_MAY_INTERLEAVE = T.MSG_READ_ONLY, T.MSG_ALWAYS_INTERLEAVE, T.MSG_MAY_INTERLEAVE

TURN_FIELDS = {"ttl": np.int64, "forward_count": np.uint8, "msg_flags": np.uint8, "result": np.uint8,
               "rejection_type": np.uint8, "resend_count": np.int32}
ABSENT = {"ttl": int(TTL_NONE), "forward_count": 0, "msg_flags": 0, "result": 0, "rejection_type": 0, "resend_count": 0}


class _Bad(Exception):
    pass


def walk_frame(buf: bytes, off: int) -> dict:
    """One frame: {"flags", "mask"} as oracle/headers.py decode_frame gives them, plus the six turn fields."""
    absent = dict(ABSENT, flags=0, mask=0)
    n = len(buf)
    if off + 8 > n:
        return dict(absent, flags=H.F_MALFORMED)
    hl, bl = struct.unpack_from("<ii", buf, off)
    if hl < 4 or bl < 0 or off + 8 + hl + bl > n:
        return dict(absent, flags=H.F_MALFORMED)
    p, end = off + 12, off + 8 + hl
    m = struct.unpack_from("<I", buf, off + 8)[0]
    flags = H.F_COMPLETE if (m & H.TARGET_ACTIVATION and m & H.TARGET_SILO and m & H.TARGET_GRAIN) else 0
    if m & (H.CACHE_INVALIDATION_HEADER | H.REQUEST_CONTEXT):      # an object-serialized field comes first
        return dict(absent, flags=flags | H.F_FALLBACK, mask=m)

    def take(k):
        nonlocal p
        if p + k > end:
            raise _Bad()
        b = buf[p:p + k]
        p += k
        return b

    def string():                                                   # BinaryTokenStreamReader.ReadString
        ln = struct.unpack("<i", take(4))[0]
        if ln < -1:
            raise _Bad()
        if ln > 0:
            take(ln)
        return ln

    def read_bool():                                                # ReadToken() == SerializationTokenType.True
        return take(1)[0] == H.TRUE_TOKEN

    def key():                                                      # ReadUniqueKey: N0, N1, TypeCodeData, KeyExt
        take(24)
        return string()

    r = dict(ABSENT)
    try:
        if m & H.CATEGORY:
            take(1)
        if m & H.DEBUG_CONTEXT:
            string()
        if m & H.DIRECTION:
            take(1)
        if m & H.TIME_TO_LIVE:
            r["ttl"] = struct.unpack("<q", take(8))[0]              # ReadTimeSpan: ticks
        if m & H.FORWARD_COUNT:
            r["forward_count"] = min(max(struct.unpack("<i", take(4))[0], 0), 255)
        if m & H.GENERIC_GRAIN_TYPE:
            string()
        if m & H.CORRELATION_ID:
            take(8)
        if m & H.ALWAYS_INTERLEAVE:
            r["msg_flags"] |= MSG_ALWAYS_INTERLEAVE if read_bool() else 0
        if m & H.IS_NEW_PLACEMENT:
            read_bool()
        if m & H.READ_ONLY:
            r["msg_flags"] |= MSG_READ_ONLY if read_bool() else 0
        if m & H.IS_UNORDERED:
            read_bool()
        if m & H.NEW_GRAIN_TYPE:
            string()
        if m & H.REJECTION_INFO:
            string()
        if m & H.REJECTION_TYPE:
            r["rejection_type"] = take(1)[0]
        if m & H.RESEND_COUNT:
            r["resend_count"] = struct.unpack("<i", take(4))[0]
        if m & H.RESULT:
            r["result"] = take(1)[0]
        if m & H.SENDING_ACTIVATION:
            key()
        if m & H.SENDING_GRAIN:
            key()
        if m & H.SENDING_SILO:
            take(24)
        if m & H.TARGET_ACTIVATION:
            key()
        if m & H.TARGET_GRAIN:
            ext = key()
            flags |= H.F_HAS_TARGET | (H.F_TARGET_KEYEXT if ext >= 0 else 0)
        if m & H.TARGET_SILO:
            if m & H.TARGET_OBSERVER:
                flags |= H.F_FALLBACK
            else:
                take(24)
    except _Bad:
        return dict(absent, flags=H.F_MALFORMED)
    return dict(r, flags=flags, mask=m)


def walk_frames(buf: bytes, offsets) -> dict:
    """SoA form: flags / mask u32 and the six gd_frame_turn_fields arrays."""
    rows = [walk_frame(buf, int(o)) for o in offsets]
    out = {"flags": np.array([x["flags"] for x in rows], np.uint32), "mask": np.array([x["mask"] for x in rows], np.uint32)}
    for k, dt in TURN_FIELDS.items():
        out[k] = np.array([x[k] for x in rows], dtype=dt).reshape(len(rows))
    return out


def aged_ttl(ttl, age: int) -> np.ndarray:
    """Message.TimeToLive's getter (Message.cs:992-1002): wire ttl - age for a ttl with a value, saturating at
    INT64_MIN; TTL_NONE stays."""
    assert age >= 0
    return np.array([t if t == int(TTL_NONE) else max(t - age, I64_MIN) for t in np.asarray(ttl, np.int64).tolist()],
                    dtype=np.int64).reshape(len(ttl))


def receive_frames_ref(f, keys, ctxs, adflags, n_ctx, request_count=None, hard_limit=0, hard_limit_sw=0):
    """gd_receive_frames on decoded fields f: frames without a completely decoded address are RECV_UNDECODED (not
    enqueued, seen by nothing); the others go through ReceiveMessage in arrival order.
    (status, ctx, perm, offsets[n_ctx + 3])."""
    n = len(f["flags"])
    ok = ((f["flags"] & H.F_HAS_TARGET) != 0) & ((f["flags"] & H.F_COMPLETE) != 0) & \
         ((f["flags"] & (H.F_FALLBACK | H.F_MALFORMED)) == 0)
    ad = RV.ActivationDirectory()
    for k, c, fl in zip(keys, ctxs, adflags):
        ad.add(tuple(int(x) for x in k), int(c), int(fl))
    st = np.full(n, RECV_UNDECODED, np.uint8)
    ctx = np.full(n, RV.M32, np.uint32)
    w = RV.receive_batch(f["target_grain"][ok], f["target_activation"][ok], f["direction"][ok], ad, n_ctx,
                         request_count, hard_limit, hard_limit_sw)
    st[ok], ctx[ok] = w[0], w[1]
    key = np.where(ctx != RV.M32, ctx.astype(np.int64), n_ctx + 1)
    perm = np.argsort(key, kind="stable").astype(np.uint32)
    offsets = np.zeros(n_ctx + 3, np.uint32)
    offsets[1:] = np.cumsum(np.bincount(key, minlength=n_ctx + 2))
    return st, ctx, perm, offsets


def chain_ref(buf, offsets, keys, ctxs, adflags, n_ctx, ctx_flags, num_running, request_count, recv_request_count=None,
              recv_hard_limit=0, recv_hard_limit_sw=0, ttl_age_ticks=0, msg_flags_or=None, hard_limit=0, hard_limit_sw=0,
              max_forward_count=2, chain=False, decoded=None):
    """gd_receive_turns_frames: (decoded fields, turn headers as the wire has them, status, ctx, perm, offsets,
    then turns_loop's six outputs).  decoded: (decode_frames, walk_frames) of the same buffer, computed before."""
    f, t = decoded if decoded is not None else (H.decode_frames(buf, offsets), walk_frames(buf, offsets))
    np.testing.assert_array_equal(t["flags"] & ~np.uint32(H.F_TARGET_KEYEXT), f["flags"] & ~np.uint32(H.F_TARGET_KEYEXT))
    st, ctx, perm, offs = receive_frames_ref(f, keys, ctxs, adflags, n_ctx, recv_request_count, recv_hard_limit,
                                             recv_hard_limit_sw)
    mf = t["msg_flags"] if msg_flags_or is None else (t["msg_flags"] | np.asarray(msg_flags_or, np.uint8))
    b = T.Batch(ctx, n_ctx, ctx_flags, num_running, request_count, st, f["direction"], aged_ttl(t["ttl"], ttl_age_ticks),
                t["forward_count"], mf, f["target_activation"], f["sending_activation"], hard_limit, hard_limit_sw,
                max_forward_count, chain)
    return (f, t, st, ctx, perm, offs) + tuple(T.turns_loop(b))


# ---- generators ---------------------------------------------------------------------------------

SILO = (b"\x00" * 12 + bytes([10, 0, 0, 2]), 11111, 3)


def join_frames(frames, lead: int = 0):
    """(buffer, offsets u64): the frames back to back after `lead` filler bytes."""
    offs, pos = [], lead
    for fr in frames:
        offs.append(pos)
        pos += len(fr)
    return bytes(lead) + b"".join(frames), np.array(offs, np.uint64)


def turn_frame(rng, tg, ta, sa=None, direction=None, complete=True, p=0.5, debug=None):
    """One addressed frame around (TargetGrain tg, TargetActivation ta) with every turn header drawn at random
    (present with probability p, both bool tokens)."""
    h = {"category": 2, "correlation_id": int(rng.integers(1, 1 << 62)), "target_grain": (tuple(int(x) for x in tg), None)}
    if direction is not None and direction != 0xFF:
        h["direction"] = int(direction)
    if debug is not None:
        h["debug_context"] = debug
    elif rng.random() < 0.2:
        h["debug_context"] = "d" * int(rng.integers(0, 200))        # long ones push the turn headers past the window
    if rng.random() < p:
        h["time_to_live"] = int(rng.choice([-5, 0, 1, 7, 50, 1 << 40, int(TTL_NONE), I64_MIN]))
    if rng.random() < p:
        h["forward_count"] = int(rng.choice([0, 1, 2, 3, 255, 256, -1]))
    for name in ("always_interleave", "is_new_placement", "read_only", "is_unordered"):
        if rng.random() < p:
            h[name] = bool(rng.random() < 0.5)
    if rng.random() < 0.1:
        h["generic_grain_type"] = None if rng.random() < 0.5 else "[[System.Int32]]"
    if rng.random() < 0.1:
        h["new_grain_type"] = "Grains.Ping"
    if rng.random() < 0.1:
        h["rejection_info"] = "why"
    if rng.random() < p:
        h["rejection_type"] = int(rng.integers(0, 6))
    if rng.random() < p:
        h["resend_count"] = int(rng.choice([0, 1, 3, -1, (1 << 31) - 1]))
    if rng.random() < p:
        h["result"] = int(rng.integers(0, 3))
    if sa is not None:
        h["sending_activation"] = (tuple(int(x) for x in sa), None)
    if complete:
        h["target_activation"] = (tuple(int(x) for x in ta), None)
        h["target_silo"] = SILO
    return h


def chain_frames(rng, tg, ta, sa, direction, p_incomplete=0.04, p_fallback=0.03, p_observer=0.03, p_malformed=0.02):
    """The frames of a mixed received batch: addressed ones, and interleaved with them frames the receive stage
    leaves UNDECODED (no TargetActivation, RequestContext first, TargetObserver, a cut header length)."""
    frames = []
    for i in range(len(tg)):
        h = turn_frame(rng, tg[i], ta[i], sa[i], direction[i], complete=rng.random() >= p_incomplete)
        if rng.random() < p_fallback:
            h["request_context"] = b"\x01\x00\x00\x00" + bytes(12)
        if rng.random() < p_observer:
            h["target_observer"] = bytes(rng.integers(0, 256, size=20, dtype=np.uint8))
        fr = bytearray(H.encode_frame(h, bytes(int(rng.integers(0, 40)))))
        if rng.random() < p_malformed:
            hl = struct.unpack_from("<i", fr, 0)[0]
            struct.pack_into("<i", fr, 0, max(4, hl - 20))
        frames.append(bytes(fr))
    return join_frames(frames, lead=int(rng.integers(0, 4)))
