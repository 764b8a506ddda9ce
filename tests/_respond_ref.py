"""Reference for the response writer (gd_respond_*) -- TEST INFRASTRUCTURE ONLY.

MessageFactory.CreateResponseMessage / CreateRejectionResponse (MessageFactory.cs:49-111) followed by
Message.Serialize (Message.cs:481-516, HeadersContainer.Serializer :1126-1244, mask: GetHeadersMask :1075-1117),
per request frame, in two independent forms:

  * respond_splice: the literal form.  Walks the request's header in Serializer order, notes where the copied
    fields stand and splices their bytes, in the answer's order, around the written ones.
  * respond_reparse: parses the whole header into the dict oracle/headers.py's encode_headers takes, builds the
    response dict field by field as MessageFactory does, and re-encodes with encode_frame.

The rule (include/graindispatch.h): Category is kept unless it is the enum default 0; DebugContext unless
IsNullOrEmpty; Direction = Response (1); TimeToLive and CorrelationId are kept; AlwaysInterleave / ReadOnly are
kept only when the request's token is True (3); RejectionInfo (a non-empty configured string), RejectionType
(unless Transient = 0) and Result (2 rejection, 1 error, absent for success) are written; the request's Target*
become the answer's Sending* (SendingActivation only with TargetGrain) and its Sending* the answer's Target*
(TargetActivation only with SendingGrain); TransactionInfo is kept; everything else is dropped.  The body is the
caller's.  Status, in this order: kind NONE -> SKIPPED; the decoder's length conditions -> MALFORMED;
CacheInvalidationHeader -> FALLBACK; the walk to Direction leaves the header -> MALFORMED; Direction present and
not Request -> DISCARDED; RequestContext, or TargetObserver with TransactionInfo -> FALLBACK; the walk through
TargetGrain leaves the header -> MALFORMED; a system-target TargetGrain without TargetActivation -> FALLBACK;
the rest of the walk leaves the header -> MALFORMED; else OK.

Both forms return (status, frame bytes).  kinds_from_turns, silo_index and respond_batch (order, out_off) are
here too, and the batches the GPU tests use.
"""
import struct

import numpy as np

import headers as H
from _encode_ref import Bad, frame_lengths, parse_headers

RSP_NONE, RSP_RESPONSE, RSP_REJECTION = range(3)
ST_OK, ST_SKIPPED, ST_MALFORMED, ST_DISCARDED, ST_FALLBACK = range(5)
NO_INFO = 0xFFFFFFFF
NO_SILO = 0xFFFFFFFF
REJ_TRANSIENT, REJ_OVERLOADED, REJ_DUPLICATE, REJ_UNRECOVERABLE = 0, 1, 2, 3
CAT_SYSTEM_TARGET = 1
(TURN_NONE, TURN_START, TURN_WAIT, TURN_REJECT_OVERLOADED, TURN_STUCK, TURN_FORWARD, TURN_REJECT_TRANSIENT,
 TURN_EXPIRED, TURN_RESPONSE, TURN_RESPONSE_DROPPED) = range(10)
RECV_REJECT_UNKNOWN, RECV_REJECT_OVERLOADED = 3, 4

INFOS = ["Overload2", "", "x" * 40, "Target silo is not active: a rather longer explanation, 61 bytes."]


def info_bytes(infos, idx):
    """The RejectionInfo string index idx names, or None (no index, past the table, empty)."""
    if idx is None or idx == NO_INFO or idx >= len(infos) or not infos[idx]:
        return None
    s = infos[idx]
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


def written_fields(kind, result, rejection_type, info, infos):
    """(RejectionInfo bytes or None, RejectionType or None, Result or None) as GetHeadersMask keeps them."""
    if kind == RSP_REJECTION:
        return info_bytes(infos, info), (rejection_type or None), 2
    return None, None, (1 if result == 1 else None)


# ------------------------------------------------------------------ form 1: literal splice
def respond_splice(buf, off, kind, result, rejection_type, info, body, infos):
    """(status, answer frame bytes) for the request frame at buf[off:]."""
    if kind not in (RSP_RESPONSE, RSP_REJECTION):
        return ST_SKIPPED, b""
    ln = frame_lengths(buf, off)
    if ln is None:
        return ST_MALFORMED, b""
    hl, _ = ln
    fr = bytes(buf[off:off + 8 + hl])
    m = struct.unpack_from("<I", fr, 8)[0]
    if m & H.CACHE_INVALIDATION_HEADER:
        return ST_FALLBACK, b""
    p, end = 12, 8 + hl

    def take(k):
        nonlocal p
        if p + k > end:
            raise Bad()
        p += k
        return fr[p - k:p]

    def string():
        s = p
        n = struct.unpack("<i", take(4))[0]
        if n < -1:
            raise Bad()
        if n > 0:
            take(n)
        return fr[s:p], n

    def key():
        s = p
        take(24)
        string()
        return fr[s:p]

    def opt(bit, rd):
        return rd() if m & bit else None

    try:
        cat = opt(H.CATEGORY, lambda: take(1))
        dbg = opt(H.DEBUG_CONTEXT, string)
        direction = opt(H.DIRECTION, lambda: take(1))
    except Bad:
        return ST_MALFORMED, b""
    if direction is not None and direction[0] != 0:
        return ST_DISCARDED, b""
    if m & H.REQUEST_CONTEXT or (m & H.TARGET_OBSERVER and m & H.TRANSACTION_INFO):
        return ST_FALLBACK, b""
    try:
        ttl = opt(H.TIME_TO_LIVE, lambda: take(8))
        opt(H.FORWARD_COUNT, lambda: take(4))
        opt(H.GENERIC_GRAIN_TYPE, string)
        corr = opt(H.CORRELATION_ID, lambda: take(8))
        ai = opt(H.ALWAYS_INTERLEAVE, lambda: take(1))
        opt(H.IS_NEW_PLACEMENT, lambda: take(1))
        ro = opt(H.READ_ONLY, lambda: take(1))
        opt(H.IS_UNORDERED, lambda: take(1))
        opt(H.NEW_GRAIN_TYPE, string)
        opt(H.REJECTION_INFO, string)
        opt(H.REJECTION_TYPE, lambda: take(1))
        opt(H.RESEND_COUNT, lambda: take(4))
        opt(H.RESULT, lambda: take(1))
        sa = opt(H.SENDING_ACTIVATION, key)
        sg = opt(H.SENDING_GRAIN, key)
        ss = opt(H.SENDING_SILO, lambda: take(24))
        ta = opt(H.TARGET_ACTIVATION, key)
        tg = opt(H.TARGET_GRAIN, key)
    except Bad:
        return ST_MALFORMED, b""
    if tg is not None and ta is None and struct.unpack_from("<Q", tg, 16)[0] >> 56 == CAT_SYSTEM_TARGET:
        return ST_FALLBACK, b""
    try:
        if m & H.TARGET_OBSERVER:                 # opaque, runs to TargetSilo: the silo is the header's last field
            r = 24 if m & H.TARGET_SILO else 0
            if end - p < r:
                raise Bad()
            ts = fr[end - r:end] if r else None
            p = end
        else:
            ts = opt(H.TARGET_SILO, lambda: take(24))
        ti = fr[p:end] if m & H.TRANSACTION_INFO else None
    except Bad:
        return ST_MALFORMED, b""
    rinfo, rtype, res = written_fields(kind, result, rejection_type, info, infos)
    om, parts = H.DIRECTION, []

    def put(bit, b):
        nonlocal om
        if b is not None:
            om |= bit
            parts.append(b)

    put(H.CATEGORY, cat if cat is not None and cat[0] != 0 else None)
    put(H.DEBUG_CONTEXT, dbg[0] if dbg is not None and dbg[1] > 0 else None)
    parts.append(b"\x01")
    put(H.TIME_TO_LIVE, ttl)
    put(H.CORRELATION_ID, corr)
    put(H.ALWAYS_INTERLEAVE, ai if ai is not None and ai[0] == H.TRUE_TOKEN else None)
    put(H.READ_ONLY, ro if ro is not None and ro[0] == H.TRUE_TOKEN else None)
    put(H.REJECTION_INFO, None if rinfo is None else struct.pack("<i", len(rinfo)) + rinfo)
    put(H.REJECTION_TYPE, None if rtype is None else bytes([rtype]))
    put(H.RESULT, None if res is None else bytes([res]))
    put(H.SENDING_ACTIVATION, ta if tg is not None else None)
    put(H.SENDING_GRAIN, tg)
    put(H.SENDING_SILO, ts)
    put(H.TARGET_ACTIVATION, sa if sg is not None else None)
    put(H.TARGET_GRAIN, sg)
    put(H.TARGET_SILO, ss)
    put(H.TRANSACTION_INFO, ti)
    hdr = b"".join(parts)
    return ST_OK, struct.pack("<iiI", 4 + len(hdr), len(body), om) + hdr + bytes(body)


# ------------------------------------------------------------------ form 2: parse, build the response, re-encode
def _direction_of(fr, hl, m):
    """The Direction byte (None when absent); Bad when the walk to it leaves the header."""
    p, end = 12, 8 + hl
    if m & H.CATEGORY:
        p += 1
    if m & H.DEBUG_CONTEXT:
        if p + 4 > end:
            raise Bad()
        n = struct.unpack_from("<i", fr, p)[0]
        if n < -1:
            raise Bad()
        p += 4 + max(n, 0)
    if not m & H.DIRECTION:
        if p > end:
            raise Bad()
        return None
    if p + 1 > end:
        raise Bad()
    return fr[p]


def respond_reparse(buf, off, kind, result, rejection_type, info, body, infos):
    if kind not in (RSP_RESPONSE, RSP_REJECTION):
        return ST_SKIPPED, b""
    ln = frame_lengths(buf, off)
    if ln is None:
        return ST_MALFORMED, b""
    hl, bl = ln
    frame = bytes(buf[off:off + 8 + hl + bl])
    m = struct.unpack_from("<I", frame, 8)[0]
    if m & H.CACHE_INVALIDATION_HEADER:
        return ST_FALLBACK, b""
    try:
        d = _direction_of(frame, hl, m)
    except Bad:
        return ST_MALFORMED, b""
    if d is not None and d != 0:
        return ST_DISCARDED, b""
    if m & H.REQUEST_CONTEXT or (m & H.TARGET_OBSERVER and m & H.TRANSACTION_INFO):
        return ST_FALLBACK, b""
    # the prefix of the header through TargetGrain decides MALFORMED before the system-target rule
    bad_all = False
    try:
        req, _, _ = parse_headers(frame, hl)
    except Bad:
        bad_all = True
        cut = m & ~(H.TARGET_OBSERVER | H.TARGET_SILO | H.TRANSACTION_INFO)
        f2 = bytearray(frame[:8 + hl])
        struct.pack_into("<I", f2, 8, cut)
        try:
            req, _, _ = parse_headers(bytes(f2), hl)       # what stood behind it is `trailing` now
        except Bad:
            return ST_MALFORMED, b""
    tg, ta = req.get("target_grain"), req.get("target_activation")
    if tg is not None and ta is None and tg[0][2] >> 56 == CAT_SYSTEM_TARGET:
        return ST_FALLBACK, b""
    if bad_all:
        return ST_MALFORMED, b""
    # MessageFactory.CreateResponseMessage (:49-100); a value GetHeadersMask drops is not set
    rsp = {"direction": 1}
    if req.get("category"):
        rsp["category"] = req["category"]
    if "correlation_id" in req:
        rsp["correlation_id"] = req["correlation_id"]
    if req.get("read_only"):
        rsp["read_only"] = True
    if req.get("always_interleave"):
        rsp["always_interleave"] = True
    if "sending_silo" in req:
        rsp["target_silo"] = req["sending_silo"]
    if "transaction_info" in req:
        rsp["transaction_info"] = req["transaction_info"]
    if "sending_grain" in req:
        rsp["target_grain"] = req["sending_grain"]
        if "sending_activation" in req:
            rsp["target_activation"] = req["sending_activation"]
    if "target_silo" in req:
        rsp["sending_silo"] = req["target_silo"]
    if tg is not None:
        rsp["sending_grain"] = tg
        if ta is not None:
            rsp["sending_activation"] = ta
    if req.get("debug_context"):
        rsp["debug_context"] = req["debug_context"]
    if "time_to_live" in req:
        rsp["time_to_live"] = req["time_to_live"]
    # CreateRejectionResponse (:102-111) / the caller's result
    rinfo, rtype, res = written_fields(kind, result, rejection_type, info, infos)
    if res is not None:
        rsp["result"] = res
    if rtype is not None:
        rsp["rejection_type"] = rtype
    if rinfo is not None:
        rsp["rejection_info"] = rinfo.decode("utf-8")
    return ST_OK, H.encode_frame(rsp, bytes(body))


# ------------------------------------------------------------------ the batch
def kinds_from_turns(turn, recv_status=None):
    n = len(turn)
    kind, rej = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        t = int(turn[i])
        r = None if recv_status is None else int(recv_status[i])
        if t == TURN_REJECT_OVERLOADED:
            kind[i], rej[i] = RSP_REJECTION, REJ_OVERLOADED
        elif t == TURN_REJECT_TRANSIENT:
            kind[i], rej[i] = RSP_REJECTION, REJ_TRANSIENT
        elif r == RECV_REJECT_UNKNOWN:
            kind[i], rej[i] = RSP_REJECTION, REJ_UNRECOVERABLE
        elif r == RECV_REJECT_OVERLOADED:
            kind[i], rej[i] = RSP_REJECTION, REJ_OVERLOADED
    return kind, rej


def silo_index(wire24, silos):
    """silos[s] = 24 wire bytes; the lowest index of each address, NO_SILO when it is not in the table."""
    first = {}
    for s, w in enumerate(silos):
        first.setdefault(bytes(w), s)
    w = np.asarray(wire24, np.uint8).reshape(-1, 24)
    return np.array([first.get(bytes(r), NO_SILO) for r in w], np.uint32)


def respond_batch(buf, offs, kind, result, rejection_type, info, body, body_off, order, infos, form=respond_splice):
    """(out bytes, out_off u64[n + 1], rsp_status u8[n]): output frame j answers input frame order[j]."""
    n = len(offs)
    frames, st = [], np.zeros(n, np.uint8)
    g = lambda a, i: None if a is None else int(a[i])
    for i in range(n):
        b = b"" if body is None or body_off is None else body[int(body_off[i]):int(body_off[i + 1])]
        s, fr = form(buf, int(offs[i]), int(kind[i]), g(result, i), g(rejection_type, i), g(info, i), b, infos)
        st[i] = s
        frames.append(fr)
    idx = range(n) if order is None else [int(x) for x in order]
    out_off = np.zeros(n + 1, np.uint64)
    parts, pos = [], 0
    for j, i in enumerate(idx):
        out_off[j] = pos
        parts.append(frames[i])
        pos += len(frames[i])
    out_off[n] = pos
    return b"".join(parts), out_off, st


# ------------------------------------------------------------------ test batches
SILO = (b"\x00" * 12 + bytes([10, 0, 0, 1]), 11111, 7)
SILO2 = (b"\x00" * 12 + bytes([10, 0, 0, 9]), 22222, 3)
P_FALLBACK = 0.03       # with 10 % non-requests and ~1 % malformed: ~85 % of the answered frames come out OK


def field_frames(n, rng):
    """Request frames in which every field the rule copies or drops is drawn independently."""
    frames = []
    tok = lambda: bool(rng.random() < 0.6)
    ext = lambda: None if rng.random() < 0.6 else "k" * int(rng.integers(0, 18))
    key = lambda cat=3: ((int(rng.integers(0, 1 << 60)), int(rng.integers(0, 1 << 60)),
                          (cat << 56) | int(rng.integers(0, 1 << 30))), ext())
    for _ in range(n):
        h = {}
        draw = lambda p: rng.random() < p
        if draw(0.8):
            h["category"] = int(rng.integers(0, 4))
        if draw(0.4):
            h["debug_context"] = None if draw(0.2) else "d" * int(rng.integers(0, 18))
        if draw(0.9):
            h["direction"] = 0 if draw(0.93) else int(rng.integers(1, 3))
        if draw(0.3):
            h["time_to_live"] = int(rng.integers(-5, 1 << 40))
        if draw(0.2):
            h["forward_count"] = 1
        if draw(0.2):
            h["generic_grain_type"] = "[[T]]"
        if draw(0.9):
            h["correlation_id"] = int(rng.integers(1, 1 << 62))
        for f in ("always_interleave", "is_new_placement", "read_only", "is_unordered"):
            if draw(0.3):
                h[f] = tok()
        if draw(0.1):
            h["new_grain_type"] = "Grains.Ping"
        if draw(0.05):
            h["rejection_info"] = "old"
        if draw(0.05):
            h["rejection_type"] = 1
        if draw(0.1):
            h["resend_count"] = 2
        if draw(0.05):
            h["result"] = 1
        if draw(0.6):
            h["sending_activation"] = key()
        if draw(0.8):
            h["sending_grain"] = key()
        if draw(0.8):
            h["sending_silo"] = SILO if draw(0.5) else SILO2
        if draw(0.7):
            h["target_activation"] = key()
        if draw(0.9):
            h["target_grain"] = key(CAT_SYSTEM_TARGET if draw(0.08) else 3)
        if draw(0.05):
            h["target_observer"] = bytes(rng.integers(0, 256, size=int(rng.integers(1, 20)), dtype=np.uint8))
        if draw(0.8):
            h["target_silo"] = SILO2
        if draw(0.1):
            h["transaction_info"] = bytes(rng.integers(0, 256, size=int(rng.integers(0, 30)), dtype=np.uint8))
        if draw(0.1):
            h["is_using_interface_version"] = True
        if draw(0.01):
            h["cache_invalidation"] = struct.pack("<i", 1) + b"\x07" * 9
        if draw(0.01):
            h["request_context"] = struct.pack("<i", 1) + b"\x08" * 11
        fr = bytearray(H.encode_frame(h, bytes(rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8))))
        if draw(0.01):
            struct.pack_into("<i", fr, 0, max(4, struct.unpack_from("<i", fr, 0)[0] - 9))
        frames.append(bytes(fr))
    return frames


def _set_request(buf, offs, rng, p_keep=0.1):
    """oracle/headers.py's random frames draw Direction from all three values: make most of them requests."""
    b = bytearray(buf)
    for o in offs:
        o = int(o)
        ln = frame_lengths(b, o)
        if ln is None or rng.random() < p_keep:
            continue
        m = struct.unpack_from("<I", b, o + 8)[0]
        if m & H.CACHE_INVALIDATION_HEADER:
            continue
        try:
            if _direction_of(bytes(b[o:o + 8 + ln[0]]), ln[0], m) is None:
                continue
        except Bad:
            continue
        p = 12 + (1 if m & H.CATEGORY else 0)
        if m & H.DEBUG_CONTEXT:
            p += 4 + max(struct.unpack_from("<i", b, o + p)[0], 0)
        b[o + p] = 0
    return bytes(b)


def random_batch(n, rng, p_fallback=P_FALLBACK, infos=INFOS):
    """n request frames -- half oracle/headers.py's random_frames (made requests), half field_frames, shuffled --
    with every kind, result, rejection type and info index and random bodies.
    Returns (buf, offs, kind, result, rejection_type, info, body, body_off)."""
    import oracle as o
    n1 = n // 2
    keys = o.grain_keys(77, rng.integers(0, 1 << 20, size=max(n1, 1)))[:n1]
    buf1, offs1 = H.random_frames(n1, keys, rng, p_fallback=p_fallback, p_complete=0.5, p_malformed=0.01)
    buf1 = _set_request(buf1, offs1, rng)
    ends = list(offs1[1:]) + [len(buf1)]
    frames = [buf1[int(a):int(b)] for a, b in zip(offs1, ends)] + field_frames(n - n1, rng)
    frames = [frames[i] for i in rng.permutation(n)]
    pad = bytes(rng.integers(0, 4))
    offs, pos = [], len(pad)
    for f in frames:
        offs.append(pos)
        pos += len(f)
    buf = pad + b"".join(frames)
    kind = rng.choice([RSP_NONE, RSP_RESPONSE, RSP_REJECTION, 7], size=n, p=[0.1, 0.5, 0.38, 0.02]).astype(np.uint8)
    result = rng.integers(0, 3, size=n).astype(np.uint8)
    rej = rng.choice([0, 1, 2, 3], size=n).astype(np.uint8)
    info = rng.integers(0, len(infos) + 2, size=n).astype(np.uint32)
    info[rng.random(n) < 0.2] = NO_INFO
    blen = rng.integers(0, 64, size=n)
    blen[rng.random(n) < 0.2] = 0
    body_off = np.zeros(n + 1, np.uint64)
    body_off[1:] = np.cumsum(blen)
    body = bytes(rng.integers(0, 256, size=int(body_off[n]), dtype=np.uint8))
    return buf, np.array(offs, dtype=np.uint64), kind, result, rej, info, body, body_off
