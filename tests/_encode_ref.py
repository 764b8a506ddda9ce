"""Reference for the frame encoder (gd_encode_frames*) -- TEST INFRASTRUCTURE ONLY.

Message.SetTargetPlacement (Message.cs:629-639, reached from Dispatcher.cs:753-767) followed by
Message.Serialize (Message.cs:481-516, HeadersContainer.Serializer :1126-1245), per frame, in two
independent forms:

  * encode_splice: the literal form.  Walks the header in Serializer order, notes where the four fields
    stand (or would stand) and splices bytes: nothing is parsed that is not needed to find a position.
  * encode_reparse: parses the whole header into the dict oracle/headers.py's encode_headers takes, sets the
    four fields on it as SetTargetPlacement does, and re-encodes with encode_frame.  Opaque
    (object-serialized) fields are kept as raw bytes.

Both return (status, frame bytes); the two agree on canonical frames (tokens 3 / 4, valid UTF-8).  The
per-frame status rule (enc_status_rule) and the batch layout (encode_batch: order, out_off) are here too.
"""
import struct

import numpy as np

import headers as H

ENC_OK, ENC_COPIED, ENC_SKIPPED, ENC_FALLBACK, ENC_MALFORMED, ENC_NO_ID, ENC_NO_SILO = range(7)
ROUTE_OK, ROUTE_MISS, ROUTE_SYSTEM_TARGET, ROUTE_MEMBERSHIP, ROUTE_KEYEXT = range(5)
ROUTE_ADDRESSED, ROUTE_UNDECODED, ROUTE_MULTI_ACT = 5, 6, 7
PLACED_NEW = 1
NO_TYPE = 0xFFFFFFFF


class Bad(Exception):
    pass


class Config:
    """What gd_encode_configure and gd_activation_ids_set hold: silos[s] = 24 wire bytes (ip[16], port,
    generation), type_names[t] = str, act_ids = (m, 3) u64 (all-zero row: no id)."""

    def __init__(self, silos, type_names, act_ids):
        self.silos = [s if isinstance(s, bytes) else H.w_silo(*s) for s in silos]
        self.type_names = list(type_names)
        self.act_ids = np.asarray(act_ids, dtype=np.uint64).reshape(-1, 3)

    def act_id(self, act):
        if act >= len(self.act_ids) or not self.act_ids[act].any():
            return None
        return tuple(int(x) for x in self.act_ids[act])

    def type_name(self, idx):
        """The string SetTargetPlacement would set, or None for String.IsNullOrEmpty / no type."""
        if idx is None or idx == NO_TYPE or idx >= len(self.type_names) or not self.type_names[idx]:
            return None
        return self.type_names[idx]


def frame_lengths(buf, off):
    """(headerLength, bodyLength) or None when the decoder's MALFORMED length conditions hold."""
    n = len(buf)
    if off > n or n - off < 8:
        return None
    hl, bl = struct.unpack_from("<ii", buf, off)
    if hl < 4 or bl < 0 or hl + bl > n - off - 8:
        return None
    return hl, bl


# ------------------------------------------------------------------ form 1: literal splice
def _walk_positions(buf, off, hl):
    """Positions (from the frame start) of the four fields and the bytes each holds now.
    Returns (mask, p_inp, r_inp, p_ngt, r_ngt, p_ta, r_ta, p_ts, r_ts)."""
    m = struct.unpack_from("<I", buf, off + 8)[0]
    p, end = 12, 8 + hl

    def take(k):
        nonlocal p
        if p + k > end:
            raise Bad()
        p += k

    def string():
        take(4)
        ln = struct.unpack_from("<i", buf, off + p - 4)[0]
        if ln < -1:
            raise Bad()
        if ln > 0:
            take(ln)

    def key():
        take(24)
        string()

    if m & H.CATEGORY:
        take(1)
    if m & H.DEBUG_CONTEXT:
        string()
    if m & H.DIRECTION:
        take(1)
    if m & H.TIME_TO_LIVE:
        take(8)
    if m & H.FORWARD_COUNT:
        take(4)
    if m & H.GENERIC_GRAIN_TYPE:
        string()
    if m & H.CORRELATION_ID:
        take(8)
    if m & H.ALWAYS_INTERLEAVE:
        take(1)
    p_inp = p
    r_inp = 1 if m & H.IS_NEW_PLACEMENT else 0
    take(r_inp)
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
    if m & H.TARGET_GRAIN:
        key()
    r_ts = 24 if m & H.TARGET_SILO else 0
    if m & H.TARGET_OBSERVER:        # opaque, runs to TargetSilo: the silo is the header's last field
        if end - p < r_ts:
            raise Bad()
        p_ts = end - r_ts
    else:
        p_ts = p
        take(r_ts)
    return m, p_inp, r_inp, p_ngt, r_ngt, p_ta, r_ta, p_ts, r_ts


def _is_fallback(m):
    return bool(m & (H.CACHE_INVALIDATION_HEADER | H.REQUEST_CONTEXT)) or \
        bool(m & H.TARGET_OBSERVER and m & H.TRANSACTION_INFO)


def encode_splice(buf, off, silo, act, route_status, placed, new_type, cfg):
    """(enc status, output frame bytes) for the frame at buf[off:]."""
    if route_status not in (ROUTE_OK, ROUTE_ADDRESSED):
        return ENC_SKIPPED, b""
    ln = frame_lengths(buf, off)
    if ln is None:
        return ENC_MALFORMED, b""
    hl, bl = ln
    frame = bytes(buf[off:off + 8 + hl + bl])
    if route_status == ROUTE_ADDRESSED:
        return ENC_COPIED, frame
    if _is_fallback(struct.unpack_from("<I", frame, 8)[0]):
        return ENC_FALLBACK, b""
    try:
        m, p_inp, r_inp, p_ngt, r_ngt, p_ta, r_ta, p_ts, r_ts = _walk_positions(buf, off, hl)
    except Bad:
        return ENC_MALFORMED, b""
    if silo >= len(cfg.silos):
        return ENC_NO_SILO, b""
    aid = cfg.act_id(act)
    if aid is None:
        return ENC_NO_ID, b""
    ta = struct.pack("<QQQi", *aid, -1)
    ts = cfg.silos[silo]
    m |= H.TARGET_ACTIVATION | H.TARGET_SILO
    if placed == PLACED_NEW:
        m |= H.IS_NEW_PLACEMENT
        inp = bytes([H.TRUE_TOKEN])
    else:
        inp, r_inp = b"", 0                       # the frame's own token, if any, is copied with the run
    name = cfg.type_name(new_type)
    if name is not None:
        m |= H.NEW_GRAIN_TYPE
        ngt = H.w_string(name)
    else:
        ngt, r_ngt = b"", 0
    hdr = (frame[12:p_inp] + inp + frame[p_inp + r_inp:p_ngt] + ngt + frame[p_ngt + r_ngt:p_ta] + ta +
           frame[p_ta + r_ta:p_ts] + ts + frame[p_ts + r_ts:8 + hl])
    out = struct.pack("<iiI", 4 + len(hdr), bl, m) + hdr + frame[8 + hl:]
    return ENC_OK, out


# ------------------------------------------------------------------ form 2: parse and re-encode
def parse_headers(frame, hl):
    """The header of `frame` as encode_headers' dict, plus (extra mask bits encode_headers does not model,
    raw bytes after the last modelled field)."""
    m = struct.unpack_from("<I", frame, 8)[0]
    p, end = 12, 8 + hl
    h = {}

    def take(k):
        nonlocal p
        if p + k > end:
            raise Bad()
        b = frame[p:p + k]
        p += k
        return b

    def string():
        ln = struct.unpack("<i", take(4))[0]
        if ln < -1:
            raise Bad()
        return None if ln == -1 else take(ln).decode("utf-8")

    def key():
        k = struct.unpack("<QQQ", take(24))
        return k, string()

    def silo():
        b = take(24)
        return b[:16], *struct.unpack("<ii", b[16:])

    def token():
        return take(1)[0] == H.TRUE_TOKEN

    simple = [("category", H.CATEGORY, lambda: take(1)[0]), ("debug_context", H.DEBUG_CONTEXT, string),
              ("direction", H.DIRECTION, lambda: take(1)[0]),
              ("time_to_live", H.TIME_TO_LIVE, lambda: struct.unpack("<q", take(8))[0]),
              ("forward_count", H.FORWARD_COUNT, lambda: struct.unpack("<i", take(4))[0]),
              ("generic_grain_type", H.GENERIC_GRAIN_TYPE, string),
              ("correlation_id", H.CORRELATION_ID, lambda: struct.unpack("<q", take(8))[0]),
              ("always_interleave", H.ALWAYS_INTERLEAVE, token), ("is_new_placement", H.IS_NEW_PLACEMENT, token),
              ("read_only", H.READ_ONLY, token), ("is_unordered", H.IS_UNORDERED, token),
              ("new_grain_type", H.NEW_GRAIN_TYPE, string), ("rejection_info", H.REJECTION_INFO, string),
              ("rejection_type", H.REJECTION_TYPE, lambda: take(1)[0]),
              ("resend_count", H.RESEND_COUNT, lambda: struct.unpack("<i", take(4))[0]),
              ("result", H.RESULT, lambda: take(1)[0]), ("sending_activation", H.SENDING_ACTIVATION, key),
              ("sending_grain", H.SENDING_GRAIN, key), ("sending_silo", H.SENDING_SILO, silo),
              ("target_activation", H.TARGET_ACTIVATION, key), ("target_grain", H.TARGET_GRAIN, key)]
    for name, bit, rd in simple:
        if m & bit:
            h[name] = rd()
    trailing = b""
    if m & H.TARGET_OBSERVER:
        r_ts = 24 if m & H.TARGET_SILO else 0
        if end - p < r_ts:
            raise Bad()
        h["target_observer"] = take(end - r_ts - p)
        if r_ts:
            h["target_silo"] = silo()
    else:
        if m & H.TARGET_SILO:
            h["target_silo"] = silo()
        rest = take(end - p)
        if m & H.TRANSACTION_INFO:
            h["transaction_info"] = rest
        else:
            trailing = rest
    if m & H.IS_USING_INTERFACE_VERSION:
        h["is_using_interface_version"] = True
    modelled = struct.unpack_from("<I", H.encode_headers(h), 0)[0]
    return h, m & ~modelled, trailing


def encode_reparse(buf, off, silo, act, route_status, placed, new_type, cfg):
    if route_status not in (ROUTE_OK, ROUTE_ADDRESSED):
        return ENC_SKIPPED, b""
    ln = frame_lengths(buf, off)
    if ln is None:
        return ENC_MALFORMED, b""
    hl, bl = ln
    frame = bytes(buf[off:off + 8 + hl + bl])
    if route_status == ROUTE_ADDRESSED:
        return ENC_COPIED, frame
    if _is_fallback(struct.unpack_from("<I", frame, 8)[0]):
        return ENC_FALLBACK, b""
    try:
        h, extra, trailing = parse_headers(frame, hl)
    except Bad:
        return ENC_MALFORMED, b""
    if silo >= len(cfg.silos):
        return ENC_NO_SILO, b""
    aid = cfg.act_id(act)
    if aid is None:
        return ENC_NO_ID, b""
    # Message.SetTargetPlacement (Message.cs:629-639)
    h["target_activation"] = (aid, None)
    w = cfg.silos[silo]
    h["target_silo"] = (w[:16], *struct.unpack("<ii", w[16:]))
    if placed == PLACED_NEW:
        h["is_new_placement"] = True
    name = cfg.type_name(new_type)
    if name is not None:
        h["new_grain_type"] = name
    hdr = bytearray(H.encode_headers(h) + trailing)
    struct.pack_into("<I", hdr, 0, struct.unpack_from("<I", hdr, 0)[0] | extra)
    return ENC_OK, struct.pack("<ii", len(hdr), bl) + bytes(hdr) + frame[8 + hl:]


# ------------------------------------------------------------------ the batch
def encode_batch(buf, offs, silo, act, status, placed, new_type, order, cfg, form=encode_splice):
    """(out bytes, out_off u64[n + 1], enc_status u8[n]): output frame j = input frame order[j]."""
    n = len(offs)
    frames, est = [], np.zeros(n, np.uint8)
    for i in range(n):
        st, fr = form(buf, int(offs[i]), int(silo[i]), int(act[i]), int(status[i]),
                      None if placed is None else int(placed[i]), None if new_type is None else int(new_type[i]), cfg)
        est[i] = st
        frames.append(fr)
    idx = range(n) if order is None else [int(x) for x in order]
    out_off = np.zeros(n + 1, np.uint64)
    parts, pos = [], 0
    for j, i in enumerate(idx):
        out_off[j] = pos
        parts.append(frames[i])
        pos += len(frames[i])
    out_off[n] = pos
    return b"".join(parts), out_off, est


# ------------------------------------------------------------------ test batches
SILOS = [(bytes(12) + bytes([10, 0, 0, 1 + s]), 11000 + s, 100 + 7 * s) for s in range(5)]
TYPE_NAMES = ["Grains.Ping", "", "Grains.A.Much.Longer.ClassName`1[[System.Int32]]", "G"]


def make_config(rng, n_act=512):
    """Activation ids with holes (all-zero rows) and a map shorter than the act values a batch uses."""
    ids = rng.integers(1, 1 << 62, size=(n_act, 3)).astype(np.uint64)
    ids[rng.random(n_act) < 0.03] = 0
    return Config(SILOS, TYPE_NAMES, ids)


def synthetic_routes(buf, offs, rng, cfg):
    """Route outputs for the frames that cover every route status, acts without an id (zero row, past the
    map), silos out of range, every place status and every type index (none, empty, past the table)."""
    n = len(offs)
    n_act = len(cfg.act_ids)
    silo = rng.integers(0, len(cfg.silos), size=n).astype(np.uint32)
    silo[rng.random(n) < 0.02] = len(cfg.silos) + 3
    silo[rng.random(n) < 0.01] = 0xFFFFFFFF
    act = rng.integers(0, n_act, size=n).astype(np.uint32)
    act[rng.random(n) < 0.02] = n_act + 5
    act[rng.random(n) < 0.01] = 0xFFFFFFFF
    status = np.zeros(n, np.uint8)
    for i in range(n):
        f = H.decode_frame(buf, int(offs[i]))
        if (f["flags"] & H.F_COMPLETE) and rng.random() < 0.8:
            status[i] = ROUTE_ADDRESSED
        elif (f["flags"] & (H.F_FALLBACK | H.F_MALFORMED)) and rng.random() < 0.5:
            status[i] = ROUTE_UNDECODED
    other = rng.random(n) < 0.08
    status[other] = rng.choice([ROUTE_MISS, ROUTE_SYSTEM_TARGET, ROUTE_MEMBERSHIP, ROUTE_KEYEXT, ROUTE_UNDECODED,
                                ROUTE_MULTI_ACT, ROUTE_ADDRESSED], size=int(other.sum())).astype(np.uint8)
    placed = rng.integers(0, 4, size=n).astype(np.uint8)
    new_type = np.full(n, NO_TYPE, np.uint32)
    typed = rng.random(n) < 0.3
    new_type[typed] = rng.integers(0, len(cfg.type_names) + 1, size=int(typed.sum())).astype(np.uint32)
    return silo, act, status, placed, new_type


def random_batch(n, rng, cfg, **kw):
    """n frames of oracle/headers.py random_frames (every optional field) with synthetic route outputs."""
    import oracle as o
    keys = o.grain_keys(77, rng.integers(0, 1 << 20, size=max(n, 1)))[:n]
    buf, offs = H.random_frames(n, keys, rng, p_fallback=kw.get("p_fallback", 0.03),
                                p_complete=kw.get("p_complete", 0.05), p_malformed=kw.get("p_malformed", 0.01))
    return (buf, offs) + synthetic_routes(buf, offs, rng, cfg)
