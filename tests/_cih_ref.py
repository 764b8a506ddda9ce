"""Reference for GD_OPT_WALK_INVALIDATION -- TEST INFRASTRUCTURE ONLY.

With the option on, the decoder, the encoder's planner and the responder's planner step over a frame's
CacheInvalidationHeader (int32 count, then per entry a 24-B SiloAddress and two UniqueKeys with their KeyExt
strings) instead of sending the frame back to C#.  Two independent forms of what they must give:

  * form A (decode_walk, encode_walk, respond_walk): a direct walker over the frame as it stands, the field
    stepped over where the serializer writes it.
  * form B (decode_cut, encode_cut, respond_cut): the field is cut out of the frame -- mask bit 1 cleared, its
    bytes removed, headerLength shortened -- and the result goes, unchanged, to the references the stages already
    have (oracle/headers.py decode_frame, tests/_frame_turns_ref.py walk_frame, tests/_encode_ref.py encode_splice,
    tests/_respond_ref.py respond_splice).  TargetGrain's KeyExt offset is moved back by the removed length; the
    encoder's output gets the field spliced back behind the mask, the responder's only when count > 0.

tests/test_cih_ref.py proves the two equal on the batches the GPU tests use.
"""
import struct

import numpy as np

import headers as H
import _encode_ref as E
import _forward_ref as F
import _frame_turns_ref as FT
import _respond_ref as R
from _encode_ref import Bad, frame_lengths

F_INVALIDATION = 32                      # GD_FRAME_INVALIDATION
CIH = H.CACHE_INVALIDATION_HEADER
DECODE_KEYS = ("flags", "mask", "target_grain", "target_activation", "sending_activation", "sending_grain",
               "target_silo", "sending_silo", "correlation_id", "category", "direction")


# ------------------------------------------------------------------ form A: the direct walker
class _Walk:
    """A cursor over the header of the frame at buf[off:]; positions are bytes from the frame start."""

    def __init__(self, buf, off, hl):
        self.b, self.o, self.p, self.end = buf, off, 12, 8 + hl

    def take(self, k):
        if self.p + k > self.end:
            raise Bad()
        self.p += k
        return bytes(self.b[self.o + self.p - k:self.o + self.p])

    def string(self):
        n = struct.unpack("<i", self.take(4))[0]
        if n < -1:
            raise Bad()
        if n > 0:
            self.take(n)
        return n

    def key(self):
        w = struct.unpack("<QQQ", self.take(24))
        return w, self.string()

    def invalidation(self):
        """Steps over the field; returns its count."""
        cnt = struct.unpack("<i", self.take(4))[0]
        if cnt < 0:
            raise Bad()
        for _ in range(cnt):
            self.take(24)
            self.key()
            self.key()
        return cnt


def _malformed():
    return dict(H.FIELDS_DEFAULT, **FT.ABSENT, flags=H.F_MALFORMED, tg_ext_off=None)


def decode_walk(buf, off):
    """The decoder's outputs for the frame at buf[off:] with the option on: oracle/headers.py decode_frame's dict,
    the six turn fields and tg_ext_off (where TargetGrain's KeyExt string lies in buf; None without one)."""
    ln = frame_lengths(buf, off)
    if ln is None:
        return _malformed()
    w = _Walk(buf, off, ln[0])
    m = struct.unpack_from("<I", buf, off + 8)[0]
    flags = H.F_COMPLETE if (m & H.TARGET_ACTIVATION and m & H.TARGET_SILO and m & H.TARGET_GRAIN) else 0
    if m & CIH:
        flags |= F_INVALIDATION
    r = dict(H.FIELDS_DEFAULT, **FT.ABSENT, mask=m & ~CIH, tg_ext_off=None)
    if m & H.REQUEST_CONTEXT:
        return dict(r, flags=flags | H.F_FALLBACK)
    tok = lambda: w.take(1)[0] == H.TRUE_TOKEN
    try:
        if m & CIH:
            w.invalidation()
        if m & H.CATEGORY:
            r["category"] = w.take(1)[0]
        if m & H.DEBUG_CONTEXT:
            w.string()
        if m & H.DIRECTION:
            r["direction"] = w.take(1)[0]
        if m & H.TIME_TO_LIVE:
            r["ttl"] = struct.unpack("<q", w.take(8))[0]
        if m & H.FORWARD_COUNT:
            r["forward_count"] = min(max(struct.unpack("<i", w.take(4))[0], 0), 255)
        if m & H.GENERIC_GRAIN_TYPE:
            w.string()
        if m & H.CORRELATION_ID:
            r["correlation_id"] = struct.unpack("<q", w.take(8))[0]
        if m & H.ALWAYS_INTERLEAVE and tok():
            r["msg_flags"] |= FT.MSG_ALWAYS_INTERLEAVE
        if m & H.IS_NEW_PLACEMENT:
            w.take(1)
        if m & H.READ_ONLY and tok():
            r["msg_flags"] |= FT.MSG_READ_ONLY
        if m & H.IS_UNORDERED:
            w.take(1)
        if m & H.NEW_GRAIN_TYPE:
            w.string()
        if m & H.REJECTION_INFO:
            w.string()
        if m & H.REJECTION_TYPE:
            r["rejection_type"] = w.take(1)[0]
        if m & H.RESEND_COUNT:
            r["resend_count"] = struct.unpack("<i", w.take(4))[0]
        if m & H.RESULT:
            r["result"] = w.take(1)[0]
        if m & H.SENDING_ACTIVATION:
            r["sending_activation"] = w.key()[0]
        if m & H.SENDING_GRAIN:
            r["sending_grain"] = w.key()[0]
        if m & H.SENDING_SILO:
            r["sending_silo"] = w.take(24)
        if m & H.TARGET_ACTIVATION:
            r["target_activation"] = w.key()[0]
        if m & H.TARGET_GRAIN:
            r["target_grain"], n = w.key()
            flags |= H.F_HAS_TARGET | (H.F_TARGET_KEYEXT if n >= 0 else 0)
            if n >= 0:
                r["tg_ext_off"] = off + w.p - n
                r["target_ext"] = bytes(buf[off + w.p - n:off + w.p])
        if m & H.TARGET_SILO:
            if m & H.TARGET_OBSERVER:
                flags |= H.F_FALLBACK
            else:
                r["target_silo"] = w.take(24)
    except Bad:
        return _malformed()
    return dict(r, flags=flags)


def encode_walk(buf, off, silo, act, route_status, placed, new_type, cfg):
    """(enc status, output frame) of gd_encode_frames* with the option on: _encode_ref.encode_splice's rule, the
    field stepped over."""
    if route_status not in (E.ROUTE_OK, E.ROUTE_ADDRESSED):
        return E.ENC_SKIPPED, b""
    ln = frame_lengths(buf, off)
    if ln is None:
        return E.ENC_MALFORMED, b""
    hl, bl = ln
    frame = bytes(buf[off:off + 8 + hl + bl])
    if route_status == E.ROUTE_ADDRESSED:
        return E.ENC_COPIED, frame
    m = struct.unpack_from("<I", frame, 8)[0]
    if m & H.REQUEST_CONTEXT or (m & H.TARGET_OBSERVER and m & H.TRANSACTION_INFO):
        return E.ENC_FALLBACK, b""
    w = _Walk(frame, 0, hl)
    opt = lambda bit, rd: rd() if m & bit else None
    try:
        opt(CIH, w.invalidation)
        opt(H.CATEGORY, lambda: w.take(1))
        opt(H.DEBUG_CONTEXT, w.string)
        opt(H.DIRECTION, lambda: w.take(1))
        opt(H.TIME_TO_LIVE, lambda: w.take(8))
        opt(H.FORWARD_COUNT, lambda: w.take(4))
        opt(H.GENERIC_GRAIN_TYPE, w.string)
        opt(H.CORRELATION_ID, lambda: w.take(8))
        opt(H.ALWAYS_INTERLEAVE, lambda: w.take(1))
        p_inp = w.p
        r_inp = 1 if m & H.IS_NEW_PLACEMENT else 0
        w.take(r_inp)
        opt(H.READ_ONLY, lambda: w.take(1))
        opt(H.IS_UNORDERED, lambda: w.take(1))
        p_ngt = w.p
        opt(H.NEW_GRAIN_TYPE, w.string)
        r_ngt = w.p - p_ngt
        opt(H.REJECTION_INFO, w.string)
        opt(H.REJECTION_TYPE, lambda: w.take(1))
        opt(H.RESEND_COUNT, lambda: w.take(4))
        opt(H.RESULT, lambda: w.take(1))
        opt(H.SENDING_ACTIVATION, w.key)
        opt(H.SENDING_GRAIN, w.key)
        opt(H.SENDING_SILO, lambda: w.take(24))
        p_ta = w.p
        opt(H.TARGET_ACTIVATION, w.key)
        r_ta = w.p - p_ta
        opt(H.TARGET_GRAIN, w.key)
        r_ts = 24 if m & H.TARGET_SILO else 0
        if m & H.TARGET_OBSERVER:
            if w.end - w.p < r_ts:
                raise Bad()
            p_ts = w.end - r_ts
        else:
            p_ts = w.p
            w.take(r_ts)
    except Bad:
        return E.ENC_MALFORMED, b""
    if silo >= len(cfg.silos):
        return E.ENC_NO_SILO, b""
    aid = cfg.act_id(act)
    if aid is None:
        return E.ENC_NO_ID, b""
    m |= H.TARGET_ACTIVATION | H.TARGET_SILO
    inp = b""
    if placed == E.PLACED_NEW:
        m |= H.IS_NEW_PLACEMENT
        inp = bytes([H.TRUE_TOKEN])
    else:
        r_inp = 0
    name = cfg.type_name(new_type)
    ngt = b""
    if name is not None:
        m |= H.NEW_GRAIN_TYPE
        ngt = H.w_string(name)
    else:
        r_ngt = 0
    hdr = (frame[12:p_inp] + inp + frame[p_inp + r_inp:p_ngt] + ngt + frame[p_ngt + r_ngt:p_ta] +
           struct.pack("<QQQi", *aid, -1) + frame[p_ta + r_ta:p_ts] + cfg.silos[silo] + frame[p_ts + r_ts:8 + hl])
    return E.ENC_OK, struct.pack("<iiI", 4 + len(hdr), bl, m) + hdr + frame[8 + hl:]


def respond_walk(buf, off, kind, result, rejection_type, info, body, infos):
    """(status, answer frame) of gd_respond_frames* with the option on: _respond_ref.respond_splice's rule, the
    field stepped over; carried into the answer when it has entries, its bit dropped when it has none."""
    if kind not in (R.RSP_RESPONSE, R.RSP_REJECTION):
        return R.ST_SKIPPED, b""
    ln = frame_lengths(buf, off)
    if ln is None:
        return R.ST_MALFORMED, b""
    hl, _ = ln
    fr = bytes(buf[off:off + 8 + hl])
    m = struct.unpack_from("<I", fr, 8)[0]
    w = _Walk(fr, 0, hl)

    def span(rd):
        s = w.p
        v = rd()
        return fr[s:w.p], v

    opt = lambda bit, rd: span(rd) if m & bit else None
    byte = lambda: w.take(1)
    try:
        cih = opt(CIH, w.invalidation)
        cat = opt(H.CATEGORY, byte)
        dbg = opt(H.DEBUG_CONTEXT, w.string)
        direction = opt(H.DIRECTION, byte)
    except Bad:
        return R.ST_MALFORMED, b""
    if direction is not None and direction[0][0] != 0:
        return R.ST_DISCARDED, b""
    if m & H.REQUEST_CONTEXT or (m & H.TARGET_OBSERVER and m & H.TRANSACTION_INFO):
        return R.ST_FALLBACK, b""
    try:
        ttl = opt(H.TIME_TO_LIVE, lambda: w.take(8))
        opt(H.FORWARD_COUNT, lambda: w.take(4))
        opt(H.GENERIC_GRAIN_TYPE, w.string)
        corr = opt(H.CORRELATION_ID, lambda: w.take(8))
        ai = opt(H.ALWAYS_INTERLEAVE, byte)
        opt(H.IS_NEW_PLACEMENT, byte)
        ro = opt(H.READ_ONLY, byte)
        opt(H.IS_UNORDERED, byte)
        opt(H.NEW_GRAIN_TYPE, w.string)
        opt(H.REJECTION_INFO, w.string)
        opt(H.REJECTION_TYPE, byte)
        opt(H.RESEND_COUNT, lambda: w.take(4))
        opt(H.RESULT, byte)
        sa = opt(H.SENDING_ACTIVATION, w.key)
        sg = opt(H.SENDING_GRAIN, w.key)
        ss = opt(H.SENDING_SILO, lambda: w.take(24))
        ta = opt(H.TARGET_ACTIVATION, w.key)
        tg = opt(H.TARGET_GRAIN, w.key)
    except Bad:
        return R.ST_MALFORMED, b""
    if tg is not None and ta is None and tg[1][0][2] >> 56 == R.CAT_SYSTEM_TARGET:
        return R.ST_FALLBACK, b""
    try:
        if m & H.TARGET_OBSERVER:
            r = 24 if m & H.TARGET_SILO else 0
            if w.end - w.p < r:
                raise Bad()
            ts = (fr[w.end - r:w.end], None) if r else None
            w.p = w.end
        else:
            ts = opt(H.TARGET_SILO, lambda: w.take(24))
        ti = (fr[w.p:w.end], None) if m & H.TRANSACTION_INFO else None
    except Bad:
        return R.ST_MALFORMED, b""
    keep_cih = cih is not None and cih[1] > 0
    keep_cat = cat is not None and cat[0][0] != 0
    keep_dbg = dbg is not None and dbg[1] > 0
    if keep_cih and cat is not None and not keep_cat and keep_dbg:
        return R.ST_FALLBACK, b""                 # the entries and DebugContext are no longer one run of the request
    rinfo, rtype, res = R.written_fields(kind, result, rejection_type, info, infos)
    om, parts = H.DIRECTION, []

    def put(bit, b):
        nonlocal om
        if b is not None:
            om |= bit
            parts.append(b)

    b0 = lambda f: None if f is None else f[0]
    put(CIH, cih[0] if keep_cih else None)
    put(H.CATEGORY, cat[0] if keep_cat else None)
    put(H.DEBUG_CONTEXT, dbg[0] if keep_dbg else None)
    parts.append(b"\x01")
    put(H.TIME_TO_LIVE, b0(ttl))
    put(H.CORRELATION_ID, b0(corr))
    put(H.ALWAYS_INTERLEAVE, ai[0] if ai is not None and ai[0][0] == H.TRUE_TOKEN else None)
    put(H.READ_ONLY, ro[0] if ro is not None and ro[0][0] == H.TRUE_TOKEN else None)
    put(H.REJECTION_INFO, None if rinfo is None else struct.pack("<i", len(rinfo)) + rinfo)
    put(H.REJECTION_TYPE, None if rtype is None else bytes([rtype]))
    put(H.RESULT, None if res is None else bytes([res]))
    put(H.SENDING_ACTIVATION, b0(ta) if tg is not None else None)
    put(H.SENDING_GRAIN, b0(tg))
    put(H.SENDING_SILO, b0(ts))
    put(H.TARGET_ACTIVATION, b0(sa) if sg is not None else None)
    put(H.TARGET_GRAIN, b0(sg))
    put(H.TARGET_SILO, b0(ss))
    put(H.TRANSACTION_INFO, b0(ti))
    hdr = b"".join(parts)
    return R.ST_OK, struct.pack("<iiI", 4 + len(hdr), len(body), om) + hdr + bytes(body)


# ------------------------------------------------------------------ form B: cut the field out
def cut_frame(buf, off):
    """(the frame at buf[off:] without the field -- a buffer of its own --, the field's bytes, its count); the field
    is None when the mask has no bit.  Bad when the field leaves the header.  The lengths must be good."""
    hl, bl = frame_lengths(buf, off)
    frame = bytes(buf[off:off + 8 + hl + bl])
    m = struct.unpack_from("<I", frame, 8)[0]
    if not m & CIH:
        return frame, None, 0
    try:
        entries, p = F.read_invalidation(frame, 12, 8 + hl)
    except UnicodeDecodeError:                    # the walker decodes the strings it steps over
        raise Bad()
    return struct.pack("<iiI", hl - (p - 12), bl, m & ~CIH) + frame[p:], frame[12:p], len(entries)


def splice_back(frame, field):
    hl, bl, m = struct.unpack_from("<iiI", frame, 0)
    return struct.pack("<iiI", hl + len(field), bl, m | CIH) + field + frame[12:]


def decode_cut(buf, off):
    if frame_lengths(buf, off) is None:
        return _malformed()
    m = struct.unpack_from("<I", buf, off + 8)[0]
    inv = F_INVALIDATION if m & CIH else 0
    if m & H.REQUEST_CONTEXT:                      # nothing behind the mask is read
        cut, removed = struct.pack("<iiI", 4, 0, m & ~CIH), 0
    else:
        try:
            cut, field, _ = cut_frame(buf, off)
        except Bad:
            return _malformed()
        removed = 0 if field is None else len(field)
    d = H.decode_frame(cut, 0)
    t = FT.walk_frame(cut, 0)
    assert d["flags"] & ~H.F_TARGET_KEYEXT == t["flags"] & ~H.F_TARGET_KEYEXT and d["mask"] == t["mask"]
    r = dict(d, **{k: t[k] for k in FT.ABSENT}, tg_ext_off=None)
    if d["flags"] & H.F_MALFORMED:
        return _malformed()
    if d["flags"] & H.F_TARGET_KEYEXT:
        hl = struct.unpack_from("<i", cut, 0)[0]
        _, _, _, _, _, p_ta, r_ta = _positions(cut, hl)
        r["tg_ext_off"] = off + p_ta + r_ta + 28 + removed
    r["flags"] = d["flags"] | inv
    return r


def _positions(cut, hl):
    """_encode_ref's walk up to TargetActivation on a frame whose tail may be opaque."""
    m = struct.unpack_from("<I", cut, 8)[0]
    keep = m & ~(H.TARGET_OBSERVER | H.TARGET_SILO | H.TRANSACTION_INFO)
    probe = bytearray(cut)
    struct.pack_into("<I", probe, 8, keep)
    return E._walk_positions(bytes(probe), 0, hl)[:7]


def encode_cut(buf, off, silo, act, route_status, placed, new_type, cfg):
    if route_status not in (E.ROUTE_OK, E.ROUTE_ADDRESSED):
        return E.ENC_SKIPPED, b""
    ln = frame_lengths(buf, off)
    if ln is None:
        return E.ENC_MALFORMED, b""
    if route_status == E.ROUTE_ADDRESSED:
        return E.ENC_COPIED, bytes(buf[off:off + 8 + ln[0] + ln[1]])
    m = struct.unpack_from("<I", buf, off + 8)[0]
    if E._is_fallback(m & ~CIH):
        return E.ENC_FALLBACK, b""
    try:
        cut, field, _ = cut_frame(buf, off)
    except Bad:
        return E.ENC_MALFORMED, b""
    st, out = E.encode_splice(cut, 0, silo, act, route_status, placed, new_type, cfg)
    if st == E.ENC_OK and field is not None:
        out = splice_back(out, field)
    return st, out


def respond_cut(buf, off, kind, result, rejection_type, info, body, infos):
    if kind not in (R.RSP_RESPONSE, R.RSP_REJECTION):
        return R.ST_SKIPPED, b""
    if frame_lengths(buf, off) is None:
        return R.ST_MALFORMED, b""
    try:
        cut, field, count = cut_frame(buf, off)
    except Bad:
        return R.ST_MALFORMED, b""
    st, out = R.respond_splice(cut, 0, kind, result, rejection_type, info, body, infos)
    if st != R.ST_OK or count == 0:
        return st, out
    m = struct.unpack_from("<I", cut, 8)[0]
    if m & H.CATEGORY and cut[12] == 0 and m & H.DEBUG_CONTEXT and struct.unpack_from("<i", cut, 13)[0] > 0:
        return R.ST_FALLBACK, b""                 # the default-valued Category byte the answer drops splits run 0
    return st, splice_back(out, field)


# ------------------------------------------------------------------ batches
def soa(rows):
    """Rows of decode_walk / decode_cut as the arrays of gd_frame_fields and gd_frame_turn_fields."""
    n = len(rows)
    keys = lambda k: np.array([x[k] for x in rows], dtype=np.uint64).reshape(n, 3)
    silos = lambda k: np.frombuffer(b"".join(x[k] for x in rows), dtype=np.uint8).reshape(n, 24)
    out = {"flags": np.array([x["flags"] for x in rows], np.uint32), "mask": np.array([x["mask"] for x in rows], np.uint32),
           "target_grain": keys("target_grain"), "target_activation": keys("target_activation"),
           "sending_activation": keys("sending_activation"), "sending_grain": keys("sending_grain"),
           "target_silo": silos("target_silo"), "sending_silo": silos("sending_silo"),
           "correlation_id": np.array([x["correlation_id"] for x in rows], np.int64),
           "category": np.array([x["category"] for x in rows], np.uint8),
           "direction": np.array([x["direction"] for x in rows], np.uint8)}
    for k, dt in FT.TURN_FIELDS.items():
        out[k] = np.array([x[k] for x in rows], dtype=dt).reshape(n)
    return out


def decode_batch(buf, offs, form=decode_walk):
    return soa([form(buf, int(o)) for o in offs])


def cut_batch(buf, offs):
    """The batch with every field cut out that can be: (buf, offs); a frame whose lengths or field are bad stays."""
    frames = []
    for o in offs:
        o = int(o)
        ln = frame_lengths(buf, o)
        if ln is None:
            frames.append(bytes(buf[o:o + 12]))
            continue
        try:
            frames.append(cut_frame(buf, o)[0])
        except Bad:
            frames.append(bytes(buf[o:o + 8 + ln[0] + ln[1]]))
    return F.pack_frames(frames)


# ---- frames
def entry(rng, grain_ext=None, act_ext=None):
    g = ((int(rng.integers(1, 1 << 60)), int(rng.integers(0, 1 << 60)), ((6 if grain_ext is not None else 3) << 56) | 7),
         grain_ext)
    a = ((int(rng.integers(1, 1 << 60)), int(rng.integers(0, 1 << 60)), 0), act_ext)
    return H.w_silo(*F.SILOS[int(rng.integers(0, 5))]), g, a


def request(rng, count=None, field=None, tg_ext=None, debug=None, category=2, body=b"", **more):
    """A request in serializer-normal form around the given invalidation field (count entries, or raw bytes)."""
    h = {}
    if field is not None:
        h["cache_invalidation"] = field
    elif count is not None:
        h["cache_invalidation"] = F.w_invalidation([entry(rng) for _ in range(count)])
    if category is not None:
        h["category"] = category
    if debug is not None:
        h["debug_context"] = debug
    h["direction"] = 0
    h["correlation_id"] = int(rng.integers(1, 1 << 62))
    h["sending_activation"] = ((int(rng.integers(1, 1 << 60)), 3, 0), None)
    h["sending_grain"] = ((int(rng.integers(1, 1 << 60)), 4, (3 << 56) | 9), None)
    h["sending_silo"] = F.SILOS[1]
    h["target_grain"] = ((int(rng.integers(1, 1 << 60)), int(rng.integers(0, 1 << 60)),
                          ((6 if tg_ext is not None else 3) << 56) | 5), tg_ext)
    h.update(more)
    return H.encode_frame(h, body)


def family(rng):
    """One frame of every kind the stages tell apart."""
    fr = [request(rng, count=c) for c in (0, 1, 2, 3)]
    fr.append(request(rng, field=F.w_invalidation([entry(rng, grain_ext="grain/ü/17"), entry(rng, act_ext="a")])))
    fr.append(request(rng, count=1, tg_ext="target-string"))
    fr.append(request(rng, count=2, tg_ext="", debug="dbg", time_to_live=123456, forward_count=1,
                      always_interleave=True, is_new_placement=True, read_only=True, resend_count=2,
                      target_activation=((77, 5, 0), None), target_silo=F.SILOS[3]))
    fr.append(request(rng))                                                       # no field at all
    fr.append(request(rng, count=1, request_context=struct.pack("<i", 1) + b"\x08" * 11))
    fr.append(request(rng, request_context=struct.pack("<i", 1) + b"\x08" * 11))
    fr.append(request(rng, count=1, target_observer=b"\x01\x02\x03", target_silo=F.SILOS[2]))
    fr.append(request(rng, count=1, target_observer=b"\x01", transaction_info=b"\x02\x03"))
    fr.append(request(rng, count=2, transaction_info=b"\x05" * 7, target_silo=F.SILOS[0]))
    fr.append(request(rng, count=1, category=0, debug="kept"))                    # the responder's split run 0
    fr.append(request(rng, count=1, category=0))
    fr.append(request(rng, count=1, category=0, debug=""))
    fr.append(request(rng, count=0, category=0, debug="kept"))
    fr.append(request(rng, count=1, category=None, debug="kept"))
    fr.append(request(rng, count=1, debug=None, category=1))
    fr.append(request(rng, count=1, direction=1))                                 # a response: DISCARDED
    fr.append(request(rng, count=1, target_grain=((5, 6, 1 << 56), None)))        # a system target
    fr += malformed(rng)
    return fr


def malformed(rng):
    fr = [request(rng, field=struct.pack("<i", -1))]
    fr.append(request(rng, field=struct.pack("<i", 5) + F.w_invalidation([entry(rng)])[4:]))   # entries past the header
    e = F.w_entry(*entry(rng, act_ext="0123456789"))
    cut = bytearray(request(rng, field=struct.pack("<i", 1) + e, category=None, body=b""))
    # the header ends inside the second key's string length: the mask, the count, and all of the entry but 12 bytes
    struct.pack_into("<i", cut, 0, 4 + 4 + len(e) - 12)
    fr.append(bytes(cut[:8 + 4 + 4 + len(e) - 12]))
    short = bytearray(request(rng, count=2))
    struct.pack_into("<i", short, 0, struct.unpack_from("<i", short, 0)[0] - 9)
    fr.append(bytes(short))
    fr.append(request(rng, field=struct.pack("<i", 0x7FFFFFFF)))
    return fr


def mixed_batch(n, rng, pad=None):
    """n frames: the family in turn, padded out with _forward_ref's normal and odd frames (fields of 0-3 entries
    with KeyExt strings, RequestContext, malformed)."""
    fam = family(rng)
    frames = []
    for i in range(n):
        if i < len(fam):
            frames.append(fam[i])
        elif rng.random() < 0.12:
            frames.append(F.odd_frame(rng))
        else:
            frames.append(F.normal_frame(rng, n_old=int(rng.integers(0, 4)) if rng.random() < 0.7 else 0))
    if n >= len(fam):
        order = rng.permutation(n)
        frames = [frames[i] for i in order]
    return F.pack_frames(frames, bytes(int(rng.integers(0, 4))) if pad is None else pad)


def edge_frames(rng, align):
    """Frames in which, in turn, the last entry's end, TargetGrain's first byte and TargetGrain's last byte fall on
    bytes 191, 192 and 193 of the frame -- either side of the 192 bytes a stage keeps of a frame in LDS -- every
    frame starting `align` bytes past a dword.  DebugContext is the padding in front of TargetGrain; an entry ends
    in front of DebugContext, so its end is moved by its own ActivationId string.  Returns (buf, offs, [(what, byte,
    entries)]); the positions are asserted against the walker."""
    frames, what = [], []
    tg = lambda: ((int(rng.integers(1, 1 << 60)), 9, (6 << 56) | 5), "xy")
    for byte in (191, 192, 193):
        es = [entry(rng), entry(rng, act_ext="e" * (byte - 175))]           # 12 + 4 + 2 * 80 - 1 = 175 without it
        fr = request(rng, field=F.w_invalidation(es), tg_ext="xy")
        assert 12 + len(cut_frame(fr, 0)[1]) - 1 == byte
        frames.append(fr)
        what.append(("entry_end", byte, 2))
        for target, count, base in (("tg_first", 1, 102), ("tg_first", 2, 182), ("tg_last", 1, 131)):
            h = {"cache_invalidation": F.w_invalidation([entry(rng) for _ in range(count)]), "category": 2,
                 "debug_context": "p" * (byte - base), "direction": 0, "target_grain": tg()}
            fr = H.encode_frame(h, b"body")
            ext = decode_walk(fr, 0)["tg_ext_off"]
            assert {"tg_first": ext - 28, "tg_last": ext + 1}[target] == byte
            frames.append(fr)
            what.append((target, byte, count))
    frames = [f if len(f) % 4 == 0 else _pad_body(f, 4 - len(f) % 4) for f in frames]
    buf, offs = F.pack_frames(frames, bytes(align))
    assert all(int(o) % 4 == align for o in offs)
    return buf, offs, what


def unaligned_tail(rng):
    """(buf, offs): the last frame ends at the last byte of a buffer whose length is no multiple of 4."""
    frames = [request(rng, count=2), request(rng, count=1, tg_ext="tail")]
    buf, offs = F.pack_frames(frames, b"\0")
    if len(buf) % 4 == 0:
        frames[1] = _pad_body(frames[1], 1)
        buf, offs = F.pack_frames(frames, b"\0")
    return buf, offs


def _pad_body(frame, k):
    hl, bl = struct.unpack_from("<ii", frame, 0)
    return struct.pack("<ii", hl, bl + k) + frame[8:] + b"\xEE" * k
