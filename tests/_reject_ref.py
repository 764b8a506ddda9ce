"""Reference for the forward rejections (gd_forward_reject_frames*) -- TEST INFRASTRUCTURE ONLY.

The failure arm of Dispatcher.TryForwardRequest (Dispatcher.cs:526-570): AddToCacheInvalidationHeader(oldAddress)
ahead of MayForward (:549-552, Message.cs:333-343), TryForwardMessage false at ForwardCount >= MaxForwardCount
(:591-599, :627-630), RejectMessage(message, Transient, exc, str) (:203-222), which answers a Request with
MessageFactory.CreateRejectionResponse (MessageFactory.cs:49-111; CreateResponseMessage copies the request's
CacheInvalidationHeader, :90) and drops any other direction, then Message.Serialize.  Per source frame, in two forms:

  * reject_fields: the field form.  Parses the frame into the message's fields (_forward_ref.parse_fields), applies
    the reference's steps in the reference's order on those fields and serializes the answer with
    oracle/headers.py's encoder.
  * reject_compose: a composition of the references the stages already have.  The appended entry is spliced into
    the request frame (mask bit 1 set, count up, headerLength grown), a default-valued Category byte -- which the
    answer drops anyway -- is cut out with its bit, and the frame goes, unchanged otherwise, to _cih_ref.respond_walk
    with kind REJECTION, rejection type 0.

Status, in this order (include/graindispatch.h): kind not FORWARD -> SKIPPED; the forward writer's MALFORMED
conditions -> MALFORMED; its FALLBACK conditions -> FALLBACK; ForwardCount < max -> MAY_FORWARD; a Direction byte
present and != 0 -> DISCARDED; an old address and local_silo past the table -> NO_SILO; an old address without an
ActivationId -> NO_ID; else OK.  The first four come from _forward_ref.forward_splice with no addresses given: its
SKIPPED / MALFORMED / FALLBACK / REJECT are the rule's own words.

Both forms return (status, answer bytes).  reject_batch (order, out_off) and the batches the tests use are here too.
"""
import struct

import numpy as np

import headers as H
import _cih_ref as C
import _forward_ref as F
import _respond_ref as R
from _encode_ref import frame_lengths

(ST_OK, ST_SKIPPED, ST_MALFORMED, ST_FALLBACK, ST_MAY_FORWARD, ST_DISCARDED, ST_NO_SILO, ST_NO_ID) = range(8)
NONE32 = F.NONE32
NO_INFO = R.NO_INFO
INFOS = R.INFOS
CIH = H.CACHE_INVALIDATION_HEADER
# the statuses gd_forward_frames* gives the frames this stage marks so (the partition property)
FWD_REJECT_SET = (ST_DISCARDED, ST_NO_SILO, ST_NO_ID, ST_OK)


def _gate(buf, off, kind, max_fc, cfg):
    """The status the forward writer's rule decides, or None for a frame that may not forward."""
    st = F.forward_splice(buf, off, kind, None, None, None, None, max_fc, 0, cfg)[0]
    if st == F.ST_REJECT:
        return None
    return {F.ST_SKIPPED: ST_SKIPPED, F.ST_MALFORMED: ST_MALFORMED, F.ST_FALLBACK: ST_FALLBACK}.get(st, ST_MAY_FORWARD)


def _old_address(cfg, old_act, local_silo):
    """(append, NO_SILO / NO_ID or None)."""
    if old_act is None or old_act == NONE32:
        return False, None
    if local_silo >= len(cfg.silos):
        return True, ST_NO_SILO
    if cfg.act_id(old_act) is None:
        return True, ST_NO_ID
    return True, None


# ------------------------------------------------------------------ form (a): the fields
def reject_fields(buf, off, kind, old_act, info, body, max_fc, local_silo, cfg, infos=INFOS):
    st = _gate(buf, off, kind, max_fc, cfg)
    if st is not None:
        return st, b""
    hl, bl = frame_lengths(buf, off)
    frame = bytes(buf[off:off + 8 + hl + bl])
    req = F.parse_fields(frame, hl)[0]
    if req.get("direction", 0) != 0:                         # RejectMessage :209-221: only a Request is answered
        return ST_DISCARDED, b""
    append, bad = _old_address(cfg, old_act, local_silo)
    if bad is not None:
        return bad, b""
    tg, ta = req["target_grain"], req.get("target_activation")
    # TryForwardRequest :549-552: message.AddToCacheInvalidationHeader(oldAddress) -- ahead of MayForward
    inval = list(req.get("invalidation", []))
    if append:
        inval.append((cfg.silos[local_silo], tg, (cfg.act_id(old_act), None)))
    # MessageFactory.CreateResponseMessage (:49-100); a value GetHeadersMask drops is not set
    rsp = {"direction": 1}
    if inval:
        rsp["cache_invalidation"] = F.w_invalidation(inval)
    if req.get("category"):
        rsp["category"] = req["category"]
    if req.get("debug_context"):
        rsp["debug_context"] = req["debug_context"]
    for k in ("time_to_live", "correlation_id", "transaction_info"):
        if k in req:
            rsp[k] = req[k]
    for k in ("read_only", "always_interleave"):
        if req.get(k):
            rsp[k] = True
    if "sending_silo" in req:
        rsp["target_silo"] = req["sending_silo"]
    if "sending_grain" in req:
        rsp["target_grain"] = req["sending_grain"]
        if "sending_activation" in req:
            rsp["target_activation"] = req["sending_activation"]
    if "target_silo" in req:
        rsp["sending_silo"] = req["target_silo"]
    rsp["sending_grain"] = tg
    if ta is not None:
        rsp["sending_activation"] = ta
    # CreateRejectionResponse (:102-111): Result = Rejection, RejectionType = Transient (the enum default), the info
    rsp["result"] = 2
    rinfo = R.info_bytes(infos, info)
    if rinfo is not None:
        rsp["rejection_info"] = rinfo.decode("utf-8")
    return ST_OK, H.encode_frame(rsp, bytes(body))


# ------------------------------------------------------------------ form (b): splice, then the responder's reference
def reject_compose(buf, off, kind, old_act, info, body, max_fc, local_silo, cfg, infos=INFOS):
    st = _gate(buf, off, kind, max_fc, cfg)
    if st is not None:
        return st, b""
    hl, bl = frame_lengths(buf, off)
    frame = bytes(buf[off:off + 8 + hl + bl])
    m = struct.unpack_from("<I", frame, 8)[0]
    w = C._Walk(frame, 0, hl)
    opt = lambda bit, rd: rd() if m & bit else None
    byte = lambda: w.take(1)
    cnt = opt(CIH, w.invalidation) or 0
    e_cih = w.p
    cat = opt(H.CATEGORY, byte)
    opt(H.DEBUG_CONTEXT, w.string)
    direction = opt(H.DIRECTION, byte)
    if direction is not None and direction[0] != 0:
        return ST_DISCARDED, b""
    append, bad = _old_address(cfg, old_act, local_silo)
    if bad is not None:
        return bad, b""
    opt(H.TIME_TO_LIVE, lambda: w.take(8))
    opt(H.FORWARD_COUNT, lambda: w.take(4))
    opt(H.GENERIC_GRAIN_TYPE, w.string)
    opt(H.CORRELATION_ID, lambda: w.take(8))
    for bit in (H.ALWAYS_INTERLEAVE, H.IS_NEW_PLACEMENT, H.READ_ONLY, H.IS_UNORDERED):
        opt(bit, byte)
    opt(H.NEW_GRAIN_TYPE, w.string)
    opt(H.REJECTION_INFO, w.string)
    opt(H.REJECTION_TYPE, byte)
    opt(H.RESEND_COUNT, lambda: w.take(4))
    opt(H.RESULT, byte)
    opt(H.SENDING_ACTIVATION, w.key)
    opt(H.SENDING_GRAIN, w.key)
    opt(H.SENDING_SILO, lambda: w.take(24))
    opt(H.TARGET_ACTIVATION, w.key)
    p_tg = w.p
    w.key()
    e_tg = w.p
    field = frame[12:e_cih]
    if append:
        entry = cfg.silos[local_silo] + frame[p_tg:e_tg] + struct.pack("<QQQi", *cfg.act_id(old_act), -1)
        field = struct.pack("<i", cnt + 1) + frame[16:e_cih] + entry
        m |= CIH
    rest = frame[e_cih:]
    if cat is not None and cat[0] == 0:                      # the answer drops it: GetHeadersMask, Message.cs:1075-1117
        rest = rest[1:]
        m &= ~H.CATEGORY
    spliced = struct.pack("<iiI", 4 + len(field) + len(rest) - bl, bl, m) + field + rest
    st, out = C.respond_walk(spliced, 0, R.RSP_REJECTION, None, R.REJ_TRANSIENT, info, body, infos)
    assert st == R.ST_OK, st
    return ST_OK, out


# ------------------------------------------------------------------ the batch
def reject_batch(buf, offs, kind, old_act, info, body, body_off, order, max_fc, local_silo, cfg, infos=INFOS,
                 form=reject_compose):
    """(out bytes, out_off u64[n + 1], rej_status u8[n]): output frame j answers input frame order[j]."""
    n = len(offs)
    g = lambda a, i: None if a is None else int(a[i])
    frames, st = [], np.zeros(n, np.uint8)
    for i in range(n):
        b = b"" if body is None or body_off is None else body[int(body_off[i]):int(body_off[i + 1])]
        s, fr = form(buf, int(offs[i]), int(kind[i]), g(old_act, i), g(info, i), b, max_fc, local_silo, cfg, infos)
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
def set_direction(frame, d):
    """The frame with its Direction byte (when it has one, and the walk reaches it) set to d."""
    ln = frame_lengths(frame, 0)
    if ln is None:
        return frame
    m = struct.unpack_from("<I", frame, 8)[0]
    w = C._Walk(frame, 0, ln[0])
    try:
        if m & CIH:
            w.invalidation()
        if m & H.CATEGORY:
            w.take(1)
        if m & H.DEBUG_CONTEXT:
            w.string()
        if not m & H.DIRECTION:
            return frame
        w.take(1)
    except C.Bad:
        return frame
    return frame[:w.p - 1] + bytes([d]) + frame[w.p:]


def mixed_frames(n, rng, max_fc=F.MAX_FC, p_limit=0.6):
    """n frames: _cih_ref's family in turn (every kind the stages tell apart, the responder's split run 0 among
    them), then _forward_ref's normal frames -- old entry counts 0-3, KeyExt strings in entries and in TargetGrain,
    ForwardCount absent, below, at and above max_fc -- and its odd frames; some OneWay and Response directions."""
    fam = C.family(rng)
    frames = []
    for i in range(n):
        if i < len(fam):
            frames.append(fam[i])
        elif rng.random() < 0.1:
            frames.append(F.odd_frame(rng))
        else:
            if rng.random() < p_limit:
                fc = max_fc + int(rng.integers(0, 2))
            else:
                fc = [None, max_fc - 1, 0, -1][int(rng.integers(0, 4))]
            fr = F.normal_frame(rng, fc=fc)
            if rng.random() < 0.08:
                fr = set_direction(fr, int(rng.choice([1, 2])))
            frames.append(fr)
    if n >= len(fam):
        frames = [frames[i] for i in rng.permutation(n)]
    return frames


def random_batch(n, rng, cfg, max_fc=F.MAX_FC, pad=None, body=True):
    """(buf, offs, kind, old_act, info, body, body_off) with every per-message input drawn."""
    frames = mixed_frames(n, rng, max_fc)
    buf, offs = F.pack_frames(frames, bytes(int(rng.integers(0, 4))) if pad is None else pad)
    n_act = len(cfg.act_ids)
    kind = rng.choice([F.FWD_FORWARD, F.FWD_NONE, 7], size=n, p=[0.9, 0.08, 0.02]).astype(np.uint8)
    old_act = rng.integers(0, n_act, size=n).astype(np.uint32)
    old_act[rng.random(n) < 0.3] = NONE32
    old_act[rng.random(n) < 0.02] = n_act + 9
    info = rng.integers(0, len(INFOS) + 2, size=n).astype(np.uint32)
    info[rng.random(n) < 0.2] = NO_INFO
    if not body:
        return buf, offs, kind, old_act, info, None, None
    lens = rng.integers(0, 40, size=n)
    lens[rng.random(n) < 0.3] = 0
    body_off = np.zeros(n + 1, np.uint64)
    body_off[1:] = np.cumsum(lens)
    bodies = bytes(rng.integers(0, 256, size=int(body_off[n]), dtype=np.uint8))
    return buf, offs, kind, old_act, info, bodies, body_off
