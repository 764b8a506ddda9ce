"""Reference for the forward writer (gd_forward_*) -- TEST INFRASTRUCTURE ONLY.

Dispatcher.TryForwardRequest (Dispatcher.cs:526-570) -> TryForwardMessage (:591-599) -> ResendMessageImpl (:601-623)
-> AddressMessage / Message.SetTargetPlacement (Message.cs:629-639) -> Message.Serialize (Message.cs:481-516,
HeadersContainer.Serializer :1126-1244, mask: GetHeadersMask :1075-1117), per source frame, in two independent forms:

  * forward_fields: the field form.  Parses the frame into the message's fields -- the CacheInvalidationHeader as a
    list of (SiloAddress, GrainId, ActivationId) entries (parse_fields: _encode_ref.parse_headers extended by the
    invalidation header) -- applies the reference's steps in the reference's order on those fields and re-serializes
    in Serializer order with the GetHeadersMask rules.
  * forward_splice: the byte-run rule the kernels follow.  Walks the header in Serializer order, through the
    invalidation entries, notes where the fields stand and splices bytes.

The invalidation header on the wire (Message.cs:1132-1140, BuiltInTypes.cs:2059-2063, BinaryTokenStreamWriter.cs:
27-35): int32 count, then per entry SiloAddress (24 B), GrainId UniqueKey (24 B + KeyExt string), ActivationId
UniqueKey (24 B + KeyExt string), no type token.

Status, in this order (include/graindispatch.h): kind not FORWARD -> SKIPPED; the decoder's length conditions, a
negative invalidation count, a walk that leaves the header -> MALFORMED; RequestContext, TargetObserver with
TransactionInfo, no TargetGrain, a system-target TargetGrain -> FALLBACK; ForwardCount >= max -> REJECT; the appended
entry's silo / id, then the written address' silo / id -> NO_SILO / NO_ID; else OK_ADDRESSED / OK_UNADDRESSED.
The two forms agree on frames in serializer-normal form; forward_fields looks at the FALLBACK masks before it
parses (it cannot size RequestContext), so only forward_splice is the rule for malformed frames that carry them.

Both forms return (status, frame bytes, target key).  forward_batch (order, out_off) and the batches the tests use
are here too.
"""
import struct

import numpy as np

import headers as H
from _encode_ref import Bad, Config, PLACED_NEW, ROUTE_OK, frame_lengths, parse_headers

FWD_NONE, FWD_FORWARD = 0, 1
(ST_OK_ADDRESSED, ST_OK_UNADDRESSED, ST_SKIPPED, ST_MALFORMED, ST_FALLBACK, ST_REJECT, ST_NO_SILO,
 ST_NO_ID) = range(8)
NONE32 = 0xFFFFFFFF
CAT_SYSTEM_TARGET = 1
TURN_STUCK, TURN_FORWARD = 4, 5
NO_KEY = (0, 0, 0)


def kinds_from_turns(turn):
    t = np.asarray(turn, np.uint8)
    return np.where((t == TURN_FORWARD) | (t == TURN_STUCK), FWD_FORWARD, FWD_NONE).astype(np.uint8)


# ------------------------------------------------------------------ the invalidation header
def w_entry(silo24, grain, activation):
    """One ActivationAddress: silo24 = 24 wire bytes, grain / activation = ((n0, n1, tcd), KeyExt or None)."""
    return bytes(silo24) + H.w_key(*grain) + H.w_key(*activation)


def w_invalidation(entries):
    """The field's bytes for encode_headers' "cache_invalidation": int32 count + the entries."""
    return struct.pack("<i", len(entries)) + b"".join(w_entry(*e) for e in entries)


def read_invalidation(frame, p, end):
    """(entries, position behind the field) for the field at frame[p:]; Bad when it leaves the header."""
    def take(k):
        nonlocal p
        if p + k > end:
            raise Bad()
        p += k
        return frame[p - k:p]

    def key():
        k = struct.unpack("<QQQ", take(24))
        ln = struct.unpack("<i", take(4))[0]
        if ln < -1:
            raise Bad()
        return k, (None if ln == -1 else take(ln).decode("utf-8"))

    cnt = struct.unpack("<i", take(4))[0]
    if cnt < 0:
        raise Bad()
    entries = []
    for _ in range(cnt):
        s = take(24)
        g = key()
        entries.append((s, g, key()))
    return entries, p


def parse_fields(frame, hl):
    """_encode_ref.parse_headers extended by the invalidation header: (fields, extra mask bits, trailing bytes);
    fields["invalidation"] = the list of entries when the bit is set."""
    m = struct.unpack_from("<I", frame, 8)[0]
    if not m & H.CACHE_INVALIDATION_HEADER:
        return parse_headers(frame, hl)
    entries, p = read_invalidation(frame, 12, 8 + hl)
    cut = bytearray(frame[:12] + frame[p:])                 # the same frame without the field
    struct.pack_into("<i", cut, 0, hl - (p - 12))
    struct.pack_into("<I", cut, 8, m & ~H.CACHE_INVALIDATION_HEADER)
    h, extra, trailing = parse_headers(bytes(cut), hl - (p - 12))
    h["invalidation"] = entries
    return h, extra, trailing


def _is_fallback_mask(m):
    return bool(m & H.REQUEST_CONTEXT) or bool(m & H.TARGET_OBSERVER and m & H.TRANSACTION_INFO) or \
        not m & H.TARGET_GRAIN


def _address_status(cfg, append, old_act, local_silo, fwd):
    """NO_SILO / NO_ID for the appended entry and the forwarding address, or None."""
    if append:
        if local_silo >= len(cfg.silos):
            return ST_NO_SILO
        if cfg.act_id(old_act) is None:
            return ST_NO_ID
    if fwd is not None:
        if fwd[0] >= len(cfg.silos):
            return ST_NO_SILO
        if cfg.act_id(fwd[1]) is None:
            return ST_NO_ID
    return None


def _fwd_of(fwd_silo, fwd_act):
    return None if fwd_silo is None or fwd_silo == NONE32 else (fwd_silo, fwd_act)


# ------------------------------------------------------------------ form 1: the fields
def forward_fields(buf, off, kind, old_act, fwd_silo, fwd_act, route, max_fc, local_silo, cfg):
    """route = (silo, act, status, placed, new_type) or None."""
    if kind != FWD_FORWARD:
        return ST_SKIPPED, b"", NO_KEY
    ln = frame_lengths(buf, off)
    if ln is None:
        return ST_MALFORMED, b"", NO_KEY
    hl, bl = ln
    frame = bytes(buf[off:off + 8 + hl + bl])
    m = struct.unpack_from("<I", frame, 8)[0]
    if _is_fallback_mask(m):
        return ST_FALLBACK, b"", NO_KEY
    try:
        h, extra, trailing = parse_fields(frame, hl)
    except Bad:
        return ST_MALFORMED, b"", NO_KEY
    tg = h["target_grain"]
    if tg[0][2] >> 56 == CAT_SYSTEM_TARGET:
        return ST_FALLBACK, b"", NO_KEY
    append = old_act is not None and old_act != NONE32
    fwd = _fwd_of(fwd_silo, fwd_act)
    # TryForwardRequest :549-552: message.AddToCacheInvalidationHeader(oldAddress) -- ahead of MayForward
    inval = list(h.get("invalidation", []))
    # TryForwardMessage :593: MayForward
    fc = h.get("forward_count", 0)
    if fc >= max_fc:
        return ST_REJECT, b"", tg[0]
    bad = _address_status(cfg, append, old_act, local_silo, fwd)
    if bad is not None:
        return bad, b"", tg[0]
    if append:
        inval.append((cfg.silos[local_silo], tg, (cfg.act_id(old_act), None)))
    h["forward_count"] = (fc + 1 + (1 << 31)) % (1 << 32) - (1 << 31)
    st = ST_OK_UNADDRESSED
    if fwd is not None:                                      # ResendMessageImpl :610-615
        w = cfg.silos[fwd[0]]
        h["target_activation"] = (cfg.act_id(fwd[1]), None)
        h["target_silo"] = (w[:16], *struct.unpack("<ii", w[16:]))
        h.pop("is_new_placement", None)
        st = ST_OK_ADDRESSED
    else:                                                    # :616-622, then AddressMessage
        h.pop("target_activation", None)
        h.pop("target_silo", None)
        if route is not None and route[2] == ROUTE_OK:
            silo, act, _, placed, new_type = route
            if silo >= len(cfg.silos):
                return ST_NO_SILO, b"", tg[0]
            if cfg.act_id(act) is None:
                return ST_NO_ID, b"", tg[0]
            w = cfg.silos[silo]
            h["target_activation"] = (cfg.act_id(act), None)
            h["target_silo"] = (w[:16], *struct.unpack("<ii", w[16:]))
            if placed == PLACED_NEW:
                h["is_new_placement"] = True
            name = cfg.type_name(new_type)
            if name is not None:
                h["new_grain_type"] = name
            st = ST_OK_ADDRESSED
    # GetHeadersMask: ForwardCount and the invalidation header only when not default / not empty
    if h["forward_count"] == 0:
        del h["forward_count"]
    h.pop("invalidation", None)
    if inval or m & H.CACHE_INVALIDATION_HEADER:
        h["cache_invalidation"] = w_invalidation(inval)
    hdr = bytearray(H.encode_headers(h) + trailing)
    struct.pack_into("<I", hdr, 0, struct.unpack_from("<I", hdr, 0)[0] | extra)
    return st, struct.pack("<ii", len(hdr), bl) + bytes(hdr) + frame[8 + hl:], tg[0]


# ------------------------------------------------------------------ form 2: the byte runs
def forward_splice(buf, off, kind, old_act, fwd_silo, fwd_act, route, max_fc, local_silo, cfg):
    if kind != FWD_FORWARD:
        return ST_SKIPPED, b"", NO_KEY
    ln = frame_lengths(buf, off)
    if ln is None:
        return ST_MALFORMED, b"", NO_KEY
    hl, bl = ln
    fr = bytes(buf[off:off + 8 + hl + bl])
    m = struct.unpack_from("<I", fr, 8)[0]
    p, end = 12, 8 + hl

    def take(k):
        nonlocal p
        if p + k > end:
            raise Bad()
        p += k

    def string():
        take(4)
        n = struct.unpack_from("<i", fr, p - 4)[0]
        if n < -1:
            raise Bad()
        if n > 0:
            take(n)
        return n

    def key():
        take(24)
        return string()

    opaque_tail = bool(m & H.TARGET_OBSERVER and m & H.TRANSACTION_INFO)
    cnt, fc, tok, ext = 0, 0, 0, -1
    p_ta = r_ta = p_tg = e_tg = p_ts = r_ts = 0
    try:
        if m & H.CACHE_INVALIDATION_HEADER:
            take(4)
            cnt = struct.unpack_from("<i", fr, 12)[0]
            if cnt < 0:
                raise Bad()
            for _ in range(cnt):
                take(24)
                key()
                key()
        e_cih = p
        if m & H.CATEGORY:
            take(1)
        if m & H.DEBUG_CONTEXT:
            string()
        if m & H.DIRECTION:
            take(1)
        if m & H.TIME_TO_LIVE:
            take(8)
        p_fc, r_fc = p, 0
        if m & H.FORWARD_COUNT:
            take(4)
            fc, r_fc = struct.unpack_from("<i", fr, p - 4)[0], 4
        if m & H.GENERIC_GRAIN_TYPE:
            string()
        if m & H.CORRELATION_ID:
            take(8)
        if m & H.ALWAYS_INTERLEAVE:
            take(1)
        p_inp, r_inp = p, 0
        if m & H.IS_NEW_PLACEMENT:
            take(1)
            tok, r_inp = fr[p - 1], 1
        if m & H.READ_ONLY:
            take(1)
        if m & H.IS_UNORDERED:
            take(1)
        p_ngt = p
        if m & H.NEW_GRAIN_TYPE:
            string()
        r_ngt = p - p_ngt
        if m & H.REJECTION_INFO:
            string()
        if m & H.REJECTION_TYPE:
            take(1)
        if not m & H.REQUEST_CONTEXT:                        # object-serialized: the walk ends in front of it
            if m & H.RESEND_COUNT:
                take(4)
            if m & H.RESULT:
                take(1)
            if m & H.SENDING_ACTIVATION:
                key()
            if m & H.SENDING_GRAIN:
                key()
            if m & H.SENDING_SILO:
                take(24)
            p_ta = p
            if m & H.TARGET_ACTIVATION:
                key()
            r_ta = p - p_ta
            p_tg = p
            if m & H.TARGET_GRAIN:
                ext = key()
            e_tg = p
            if not opaque_tail:
                r_ts = 24 if m & H.TARGET_SILO else 0
                if m & H.TARGET_OBSERVER:                    # opaque, runs to TargetSilo: the header's last field
                    if end - p < r_ts:
                        raise Bad()
                    p_ts = end - r_ts
                else:
                    p_ts = p
                    take(r_ts)
    except Bad:
        return ST_MALFORMED, b"", NO_KEY
    if _is_fallback_mask(m):
        return ST_FALLBACK, b"", NO_KEY
    tg = struct.unpack_from("<QQQ", fr, p_tg)
    if tg[2] >> 56 == CAT_SYSTEM_TARGET:
        return ST_FALLBACK, b"", NO_KEY
    if fc >= max_fc:
        return ST_REJECT, b"", tg
    append = old_act is not None and old_act != NONE32
    fwd = _fwd_of(fwd_silo, fwd_act)
    bad = _address_status(cfg, append, old_act, local_silo, fwd)
    if bad is not None:
        return bad, b"", tg
    null_ext = struct.pack("<i", -1)
    om = m & ~(H.TARGET_ACTIVATION | H.TARGET_SILO | H.FORWARD_COUNT)
    inval = b""
    if m & H.CACHE_INVALIDATION_HEADER or append:
        inval = struct.pack("<i", cnt + (1 if append else 0)) + fr[16:e_cih if m & H.CACHE_INVALIDATION_HEADER else 16]
    if append:
        om |= H.CACHE_INVALIDATION_HEADER
        inval += cfg.silos[local_silo] + fr[p_tg:e_tg] + struct.pack("<QQQ", *cfg.act_id(old_act)) + null_ext
    fc_new = (fc + 1) & 0xFFFFFFFF
    fcb = b""
    if fc_new:
        om |= H.FORWARD_COUNT
        fcb = struct.pack("<I", fc_new)
    inp = fr[p_inp:p_inp + r_inp]
    ngt = fr[p_ngt:p_ngt + r_ngt]
    ta = ts = b""
    st = ST_OK_UNADDRESSED
    if fwd is not None:
        om = (om | H.TARGET_ACTIVATION | H.TARGET_SILO) & ~H.IS_NEW_PLACEMENT
        inp = b""
        ta = struct.pack("<QQQ", *cfg.act_id(fwd[1])) + null_ext
        ts = cfg.silos[fwd[0]]
        st = ST_OK_ADDRESSED
    elif route is not None and route[2] == ROUTE_OK:
        silo, act, _, placed, new_type = route
        if silo >= len(cfg.silos):
            return ST_NO_SILO, b"", tg
        if cfg.act_id(act) is None:
            return ST_NO_ID, b"", tg
        om |= H.TARGET_ACTIVATION | H.TARGET_SILO
        ta = struct.pack("<QQQ", *cfg.act_id(act)) + null_ext
        ts = cfg.silos[silo]
        if placed == PLACED_NEW:
            om |= H.IS_NEW_PLACEMENT
            inp = bytes([H.TRUE_TOKEN])
        name = cfg.type_name(new_type)
        if name is not None:
            om |= H.NEW_GRAIN_TYPE
            ngt = H.w_string(name)
        st = ST_OK_ADDRESSED
    hdr = (inval + fr[e_cih:p_fc] + fcb + fr[p_fc + r_fc:p_inp] + inp + fr[p_inp + r_inp:p_ngt] + ngt +
           fr[p_ngt + r_ngt:p_ta] + ta + fr[p_ta + r_ta:p_ts] + ts + fr[p_ts + r_ts:8 + hl])
    return st, struct.pack("<iiI", 4 + len(hdr), bl, om) + hdr + fr[8 + hl:], tg


# ------------------------------------------------------------------ the batch
def forward_batch(buf, offs, kind, old_act, fwd_silo, fwd_act, routes, order, max_fc, local_silo, cfg,
                  form=forward_splice):
    """routes = (silo, act, status, placed, new_type) arrays (placed / new_type may be None) or None.
    Returns (out bytes, out_off u64[n + 1], fwd_status u8[n], target u64[n, 3]): output frame j = input order[j]."""
    n = len(offs)
    g = lambda a, i: None if a is None else int(a[i])
    frames, st, target = [], np.zeros(n, np.uint8), np.zeros((n, 3), np.uint64)
    for i in range(n):
        route = None if routes is None else tuple(g(a, i) for a in routes)
        fs = None if fwd_silo is None or fwd_act is None else int(fwd_silo[i])
        s, fr, tg = form(buf, int(offs[i]), int(kind[i]), g(old_act, i), fs, g(fwd_act, i), route, max_fc,
                         local_silo, cfg)
        st[i] = s
        target[i] = tg
        frames.append(fr)
    idx = range(n) if order is None else [int(x) for x in order]
    out_off = np.zeros(n + 1, np.uint64)
    parts, pos = [], 0
    for j, i in enumerate(idx):
        out_off[j] = pos
        parts.append(frames[i])
        pos += len(frames[i])
    out_off[n] = pos
    return b"".join(parts), out_off, st, target


# ------------------------------------------------------------------ test batches
SILOS = [(bytes(12) + bytes([10, 0, 0, 1 + s]), 11000 + s, 100 + 7 * s) for s in range(5)]
SILO_TUPLES = [(f"10.0.0.{1 + s}", 11000 + s, 100 + 7 * s) for s in range(5)]
TYPE_NAMES = ["Grains.Ping", "", "Grains.A.Much.Longer.ClassName`1[[System.Int32]]", "G"]
LOCAL_SILO = 2
MAX_FC = 2


def make_config(rng, n_act=512):
    ids = rng.integers(1, 1 << 62, size=(n_act, 3)).astype(np.uint64)
    ids[rng.random(n_act) < 0.03] = 0
    return Config(SILOS, TYPE_NAMES, ids)


def rand_key(rng, cat=3, p_ext=0.3):
    ext = None
    if cat == 6 or rng.random() < p_ext:
        ext = "k" * int(rng.integers(0, 40))
        cat = 6
    return ((int(rng.integers(0, 1 << 60)), int(rng.integers(0, 1 << 60)), (cat << 56) | int(rng.integers(0, 1 << 30))),
            ext)


def rand_entries(rng, k):
    return [(H.w_silo(*SILOS[int(rng.integers(0, 5))]), rand_key(rng), ((int(rng.integers(1, 1 << 60)), 5, 0), None))
            for _ in range(k)]


def normal_frame(rng, n_old=None, fc="draw", p=None):
    """A request frame in serializer-normal form: every optional field drawn independently, only values the
    reference's GetHeadersMask keeps (the ForwardCount argument aside: absent, or the given value)."""
    draw = lambda q: rng.random() < (p if p is not None else q)
    h = {}
    if n_old is None:
        n_old = int(rng.choice([0, 0, 0, 1, 2, 3]))
    if n_old:
        h["cache_invalidation"] = w_invalidation(rand_entries(rng, n_old))
    if draw(0.8):
        h["category"] = int(rng.integers(1, 3))
    if draw(0.3):
        h["debug_context"] = "d" * int(rng.integers(1, 30))
    if draw(0.9):
        h["direction"] = 0
    if draw(0.5):
        h["time_to_live"] = int(rng.integers(1, 1 << 40))
    if fc == "draw":
        fc = [None, None, 0, 1, 2, -1][int(rng.integers(0, 6))]
    if fc is not None:
        h["forward_count"] = fc
    if draw(0.2):
        h["generic_grain_type"] = "[[T" + "x" * int(rng.integers(0, 9)) + "]]"
    if draw(0.9):
        h["correlation_id"] = int(rng.integers(1, 1 << 62))
    for f in ("always_interleave", "is_new_placement", "read_only", "is_unordered"):
        if draw(0.3):
            h[f] = True
    if draw(0.15):
        h["new_grain_type"] = "Grains.Old" + "y" * int(rng.integers(0, 30))
    if draw(0.05):
        h["rejection_info"] = "old"
    if draw(0.05):
        h["rejection_type"] = 1
    if draw(0.1):
        h["resend_count"] = 2
    if draw(0.05):
        h["result"] = 1
    if draw(0.7):
        h["sending_activation"] = rand_key(rng, p_ext=0)
    if draw(0.8):
        h["sending_grain"] = rand_key(rng)
    if draw(0.8):
        h["sending_silo"] = SILOS[int(rng.integers(0, 5))]
    if draw(0.7):
        h["target_activation"] = rand_key(rng, p_ext=0)
    h["target_grain"] = rand_key(rng)
    if draw(0.7):
        h["target_silo"] = SILOS[int(rng.integers(0, 5))]
    if draw(0.1):
        h["is_using_interface_version"] = True
    tail = rng.random()
    if tail < 0.08:
        h["target_observer"] = bytes(rng.integers(0, 256, size=int(rng.integers(1, 20)), dtype=np.uint8))
    elif tail < 0.16:
        h["transaction_info"] = bytes(rng.integers(0, 256, size=int(rng.integers(1, 30)), dtype=np.uint8))
    return H.encode_frame(h, bytes(rng.integers(0, 256, size=int(rng.integers(0, 48)), dtype=np.uint8)))


def odd_frame(rng):
    """Frames for the other statuses: malformed, fallback, system target, no TargetGrain."""
    k = int(rng.integers(0, 6))
    if k == 0:                                               # the header ends inside a field
        fr = bytearray(normal_frame(rng, p=0.0))
        struct.pack_into("<i", fr, 0, struct.unpack_from("<i", fr, 0)[0] - 9)
        return bytes(fr)
    if k == 1:                                               # a negative invalidation count
        return H.encode_frame({"cache_invalidation": struct.pack("<i", -2), "target_grain": rand_key(rng)}, b"xy")
    if k == 2:
        return H.encode_frame({"category": 2, "request_context": struct.pack("<i", 1) + b"\x08" * 11,
                               "target_grain": rand_key(rng)}, b"")
    if k == 3:
        return H.encode_frame({"target_grain": rand_key(rng, p_ext=0), "target_observer": b"\x01\x02",
                               "transaction_info": b"\x03"}, b"b")
    if k == 4:
        return H.encode_frame({"category": 2, "correlation_id": 5, "sending_grain": rand_key(rng)}, b"")
    return H.encode_frame({"category": 1, "target_grain": rand_key(rng, cat=CAT_SYSTEM_TARGET, p_ext=0)}, b"sys")


def pack_frames(frames, pad=b""):
    buf, offs = pad, []
    for f in frames:
        offs.append(len(buf))
        buf += f
    return buf, np.array(offs, dtype=np.uint64)


def random_batch(n, rng, cfg, p_odd=0.1, pad=None):
    """n frames with every per-message input drawn.  Returns the arguments of forward_batch up to `routes`:
    (buf, offs, kind, old_act, fwd_silo, fwd_act, (silo, act, status, placed, new_type))."""
    frames = [odd_frame(rng) if rng.random() < p_odd else normal_frame(rng) for _ in range(n)]
    buf, offs = pack_frames(frames, bytes(int(rng.integers(0, 4))) if pad is None else pad)
    n_act = len(cfg.act_ids)
    kind = rng.choice([FWD_FORWARD, FWD_NONE, 7], size=n, p=[0.9, 0.08, 0.02]).astype(np.uint8)
    old_act = rng.integers(0, n_act, size=n).astype(np.uint32)
    old_act[rng.random(n) < 0.3] = NONE32
    old_act[rng.random(n) < 0.02] = n_act + 9
    fwd_silo = rng.integers(0, len(cfg.silos), size=n).astype(np.uint32)
    fwd_silo[rng.random(n) < 0.5] = NONE32
    fwd_silo[rng.random(n) < 0.02] = len(cfg.silos) + 1
    fwd_act = rng.integers(0, n_act, size=n).astype(np.uint32)
    fwd_act[rng.random(n) < 0.02] = n_act + 5
    silo = rng.integers(0, len(cfg.silos), size=n).astype(np.uint32)
    silo[rng.random(n) < 0.02] = len(cfg.silos) + 3
    act = rng.integers(0, n_act, size=n).astype(np.uint32)
    act[rng.random(n) < 0.02] = NONE32
    status = rng.choice([0, 1, 4, 7], size=n, p=[0.6, 0.3, 0.05, 0.05]).astype(np.uint8)
    placed = rng.integers(0, 4, size=n).astype(np.uint8)
    new_type = np.full(n, NONE32, np.uint32)
    typed = rng.random(n) < 0.3
    new_type[typed] = rng.integers(0, len(cfg.type_names) + 1, size=int(typed.sum())).astype(np.uint32)
    return buf, offs, kind, old_act, fwd_silo, fwd_act, (silo, act, status, placed, new_type)
