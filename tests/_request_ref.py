"""Reference for the request writer (gd_request_*) -- TEST INFRASTRUCTURE ONLY.

MessageFactory.CreateMessage (MessageFactory.cs:21-47) + InsideRuntimeClient.SendRequestMessage
(InsideRuntimeClient.cs:120-229) + Message.SetTargetPlacement (Message.cs:629-639) + Message.Serialize
(Message.cs:481-516, HeadersContainer.Serializer :1126-1245, mask: GetHeadersMask :1075-1117), per message, in two
independent forms:

  * request_fields: builds the field dict as CreateMessage -> SendRequestMessage -> SetTargetPlacement set the
    message's properties and hands it to oracle/headers.py's encode_frame (the mask-only bit 28, which that
    encoder does not know, is set in the finished frame).
  * request_literal: a literal byte builder, field by field in Serializer order, with its own mask.

The rule (include/graindispatch.h): Category 2, DebugContext (a non-empty configured string), Direction 0 / 2
(one-way), TimeToLive (the batch's, unless GD_TTL_NONE, one-way or NO_TTL), GenericGrainType (a non-empty configured
string), CorrelationId id_base + i, True tokens for AlwaysInterleave / IsNewPlacement (addressed and placed == NEW) /
ReadOnly / IsUnordered, NewGrainType (addressed, a non-empty type string), SendingActivation, SendingGrain,
SendingSilo = silos[my_silo], TargetActivation and TargetSilo when addressed, TargetGrain, mask bits 26 / 28.
"Addressed": route arrays given and status == ROUTE_OK.  Status, in this order (request_status): a KeyExt length of
-2 -> FALLBACK; a system-target TargetGrain -> FALLBACK; sender_act without an ActivationId -> NO_ID; addressed and
silo >= n_silos -> NO_SILO; addressed and act without an ActivationId -> NO_ID; addressed -> OK; else UNADDRESSED
(written without TargetActivation, TargetSilo, IsNewPlacement, NewGrainType).  Only OK and UNADDRESSED frames have bytes.

A batch is a dict: target (n,3) u64, target_ext (list of None / str / -2, or None), sender_grain, sender_ext,
sender_act, options, generic, debug, id_base, ttl_ticks, body, body_off; a route is a dict silo, act, status,
placed, new_type (or None).  request_batch gives (out bytes, out_off, req_status); the test batches are here too.
"""
import struct

import numpy as np

import headers as H

(OPT_ONE_WAY, OPT_NO_TTL, OPT_ALWAYS_INTERLEAVE, OPT_READ_ONLY, OPT_UNORDERED, OPT_IFACE_VERSION,
 OPT_TXN_REQUIRED) = (1 << k for k in range(7))
ST_OK, ST_UNADDRESSED, ST_FALLBACK, ST_NO_ID, ST_NO_SILO = range(5)
ROUTE_OK, ROUTE_MISS = 0, 1
PLACED_NEW = 1
TTL_NONE = (1 << 63) - 1
KEYEXT_HOST = -2
CAT_SYSTEM_TARGET = 1
NONE32 = 0xFFFFFFFF
IS_TRANSACTION_REQUIRED = 1 << 28


class Tables:
    """What the handle holds: silos[s] = (ip16, port, generation), my_silo, act_ids (A,3) u64 (a zero row: no id),
    the encoder's type names and gd_request_configure's strings."""

    def __init__(self, silos, my_silo, act_ids, types, strings):
        self.silos, self.my_silo, self.types, self.strings = silos, my_silo, types, strings
        self.act_ids = np.asarray(act_ids, dtype=np.uint64).reshape(-1, 3)

    def act_id(self, a):
        if a >= len(self.act_ids) or not self.act_ids[a].any():
            return None
        return tuple(int(x) for x in self.act_ids[a])


def _string(table, idx_array, i):
    """The non-empty string index idx_array[i] names, or None."""
    if idx_array is None:
        return None
    k = int(idx_array[i])
    return table[k] if k < len(table) and table[k] else None


def _ext(exts, i):
    return None if exts is None else exts[i]


def _addressed(route, i):
    return route is not None and route.get("status") is not None and int(route["status"][i]) == ROUTE_OK


def request_status(b, route, i, t):
    for x in (_ext(b.get("target_ext"), i), _ext(b.get("sender_ext"), i)):
        if isinstance(x, (int, np.integer)) and x == KEYEXT_HOST:
            return ST_FALLBACK
    if int(b["target"][i][2]) >> 56 == CAT_SYSTEM_TARGET:
        return ST_FALLBACK
    if t.act_id(int(b["sender_act"][i])) is None:
        return ST_NO_ID
    if _addressed(route, i):
        if int(route["silo"][i]) >= len(t.silos):
            return ST_NO_SILO
        if t.act_id(int(route["act"][i])) is None:
            return ST_NO_ID
        return ST_OK
    return ST_UNADDRESSED


def _body(b, i):
    if b.get("body") is None or b.get("body_off") is None:
        return b""
    return bytes(b["body"][int(b["body_off"][i]):int(b["body_off"][i + 1])])


def _i64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


# ------------------------------------------------------------------ form 1: the message's properties, then encode_frame
def request_fields(b, route, i, t):
    """(status, frame bytes) for message i."""
    st = request_status(b, route, i, t)
    if st not in (ST_OK, ST_UNADDRESSED):
        return st, b""
    opt = 0 if b.get("options") is None else int(b["options"][i])
    key = lambda a: tuple(int(x) for x in a[i])
    # MessageFactory.CreateMessage
    m = {"category": 2, "direction": 2 if opt & OPT_ONE_WAY else 0, "correlation_id": _i64(int(b["id_base"]) + i)}
    if opt & OPT_READ_ONLY:
        m["read_only"] = True
    if opt & OPT_ALWAYS_INTERLEAVE:
        m["always_interleave"] = True
    if opt & OPT_UNORDERED:
        m["is_unordered"] = True
    if opt & OPT_IFACE_VERSION:
        m["is_using_interface_version"] = True
    # SendRequestMessage
    m["sending_grain"] = (key(b["sender_grain"]), _ext(b.get("sender_ext"), i))
    m["sending_activation"] = (t.act_id(int(b["sender_act"][i])), None)
    m["sending_silo"] = t.silos[t.my_silo]
    m["target_grain"] = (key(b["target"]), _ext(b.get("target_ext"), i))
    dbg, gen = _string(t.strings, b.get("debug"), i), _string(t.strings, b.get("generic"), i)
    if dbg:
        m["debug_context"] = dbg
    if gen:
        m["generic_grain_type"] = gen
    if int(b["ttl_ticks"]) != TTL_NONE and not opt & (OPT_ONE_WAY | OPT_NO_TTL):
        m["time_to_live"] = int(b["ttl_ticks"])
    # AddressMessage + SetTargetPlacement
    if st == ST_OK:
        m["target_activation"] = (t.act_id(int(route["act"][i])), None)
        m["target_silo"] = t.silos[int(route["silo"][i])]
        if route.get("placed") is not None and int(route["placed"][i]) == PLACED_NEW:
            m["is_new_placement"] = True
        ngt = _string(t.types, route.get("new_type"), i)
        if ngt:
            m["new_grain_type"] = ngt
    fr = bytearray(H.encode_frame(m, _body(b, i)))
    if opt & OPT_TXN_REQUIRED:
        struct.pack_into("<I", fr, 8, struct.unpack_from("<I", fr, 8)[0] | IS_TRANSACTION_REQUIRED)
    return st, bytes(fr)


# ------------------------------------------------------------------ form 2: literal bytes
def request_literal(b, route, i, t):
    st = request_status(b, route, i, t)
    if st not in (ST_OK, ST_UNADDRESSED):
        return st, b""
    opt = 0 if b.get("options") is None else int(b["options"][i])
    addressed = st == ST_OK
    mask = (1 << 2) | (1 << 5) | (1 << 3) | (1 << 15) | (1 << 16) | (1 << 17) | (1 << 20)
    u64x3 = lambda k: struct.pack("<QQQ", *(int(x) for x in k))

    def lstr(s):
        raw = s.encode("utf-8") if isinstance(s, str) else bytes(s)
        return struct.pack("<i", len(raw)) + raw

    def ext(x):
        return struct.pack("<i", -1) if x is None else lstr(x)

    out = [b"\x02"]                                                  # Category: Application
    dbg, gen = _string(t.strings, b.get("debug"), i), _string(t.strings, b.get("generic"), i)
    if dbg:
        mask |= 1 << 4
        out.append(lstr(dbg))
    out.append(b"\x02" if opt & OPT_ONE_WAY else b"\x00")            # Direction
    if int(b["ttl_ticks"]) != TTL_NONE and not opt & OPT_ONE_WAY and not opt & OPT_NO_TTL:
        mask |= 1 << 6
        out.append(struct.pack("<q", int(b["ttl_ticks"])))
    if gen:
        mask |= 1 << 9
        out.append(lstr(gen))
    out.append(struct.pack("<Q", (int(b["id_base"]) + i) & ((1 << 64) - 1)))
    if opt & OPT_ALWAYS_INTERLEAVE:
        mask |= 1 << 0
        out.append(b"\x03")
    if addressed and route.get("placed") is not None and int(route["placed"][i]) == PLACED_NEW:
        mask |= 1 << 18
        out.append(b"\x03")
    if opt & OPT_READ_ONLY:
        mask |= 1 << 13
        out.append(b"\x03")
    if opt & OPT_UNORDERED:
        mask |= 1 << 23
        out.append(b"\x03")
    ngt = _string(t.types, route.get("new_type"), i) if addressed else None
    if ngt:
        mask |= 1 << 8
        out.append(lstr(ngt))
    out.append(u64x3(t.act_ids[int(b["sender_act"][i])]) + b"\xff\xff\xff\xff")
    out.append(u64x3(b["sender_grain"][i]) + ext(_ext(b.get("sender_ext"), i)))
    ip, port, gen_no = t.silos[t.my_silo]
    out.append(bytes(ip) + struct.pack("<ii", port, gen_no))
    if addressed:
        mask |= (1 << 19) | (1 << 21)
        out.append(u64x3(t.act_ids[int(route["act"][i])]) + b"\xff\xff\xff\xff")
    out.append(u64x3(b["target"][i]) + ext(_ext(b.get("target_ext"), i)))
    if addressed:
        ip, port, gen_no = t.silos[int(route["silo"][i])]
        out.append(bytes(ip) + struct.pack("<ii", port, gen_no))
    if opt & OPT_IFACE_VERSION:
        mask |= 1 << 26
    if opt & OPT_TXN_REQUIRED:
        mask |= 1 << 28
    hdr = struct.pack("<I", mask) + b"".join(out)
    body = _body(b, i)
    return st, struct.pack("<ii", len(hdr), len(body)) + hdr + body


# ------------------------------------------------------------------ the batch
def request_batch(b, route, order, t, form=request_literal):
    """(out bytes, out_off u64[n + 1], req_status u8[n]): output frame j is message order[j]."""
    n = len(b["target"])
    frames, st = [], np.zeros(n, np.uint8)
    for i in range(n):
        st[i], fr = form(b, route, i, t)
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


def send_ttl(b):
    """The TimeToLive each message carries into gd_send_queues (None: none has one)."""
    n = len(b["target"])
    if int(b["ttl_ticks"]) == TTL_NONE:
        return None
    opt = np.zeros(n, np.uint8) if b.get("options") is None else np.asarray(b["options"], np.uint8)
    return np.where(opt & (OPT_ONE_WAY | OPT_NO_TTL), TTL_NONE, int(b["ttl_ticks"])).astype(np.int64)


# ------------------------------------------------------------------ test tables and batches
SILO_TUPLES = [(f"10.0.0.{1 + s}", 11000 + s, 100 + 7 * s) for s in range(5)]
SILOS = [(bytes(12) + bytes([10, 0, 0, 1 + s]), 11000 + s, 100 + 7 * s) for s in range(5)]
TYPES = ["Grains.Ping", "", "Grains.Generic`1[[System.String]]"]
STRINGS = ["ctx", "", "[[System.Int32]]", "d" * 61, "a debug context of 300 bytes " + "x" * 271]
N_ACT = 64


def tables(my_silo=1, n_act=N_ACT):
    ids = np.zeros((n_act, 3), np.uint64)
    a = np.arange(n_act, dtype=np.uint64)
    ids[:, 0], ids[:, 1], ids[:, 2] = 0x1111000000000000 + a * 977, 0xABCD00000000 + a, 0x0400000000000000
    ids[5::16] = 0                                                  # no ActivationId
    return Tables(SILOS, my_silo, ids, TYPES, STRINGS)


def grain_key(rng, cat=3):
    return (int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 62)), (cat << 56) | int(rng.integers(0, 1 << 31)))


def random_batch(n, rng, t, body_max=64, p_host_ext=0.005):
    """(batch, route): every option, string, KeyExt and route status drawn independently; about 10 % misses, 3 %
    system targets, 2 % unknown sender activations, 2 % silos past the table, KeyExt on 10 % of the targets and of
    the senders with lengths 0, 1, 63 and 300, and a few -2 lengths."""
    n_act = len(t.act_ids)
    good = np.flatnonzero(t.act_ids.any(axis=1))
    bad = np.concatenate([np.flatnonzero(~t.act_ids.any(axis=1)), [n_act, n_act + 7, NONE32]])
    target = np.array([grain_key(rng, CAT_SYSTEM_TARGET if rng.random() < 0.03 else 3) for _ in range(n)],
                      dtype=np.uint64).reshape(n, 3)
    sender = np.array([grain_key(rng) for _ in range(n)], dtype=np.uint64).reshape(n, 3)

    def exts():
        out = []
        for _ in range(n):
            r = rng.random()
            if r < p_host_ext:
                out.append(KEYEXT_HOST)
            elif r < 0.1 + p_host_ext:
                out.append("k" * int(rng.choice([0, 1, 63, 300])))
            else:
                out.append(None)
        return out

    sender_act = rng.choice(good, size=n).astype(np.uint32)
    unknown = rng.random(n) < 0.02
    sender_act[unknown] = rng.choice(bad, size=int(unknown.sum())).astype(np.uint32)
    options = np.zeros(n, np.uint8)
    for bit in range(7):
        options |= ((rng.random(n) < 0.25).astype(np.uint8) << bit).astype(np.uint8)
    idx = lambda: np.where(rng.random(n) < 0.4, rng.integers(0, len(t.strings) + 2, size=n), NONE32).astype(np.uint32)
    blen = rng.integers(0, body_max, size=n) if body_max else np.zeros(n, np.int64)
    blen[rng.random(n) < 0.2] = 0
    body_off = np.zeros(n + 1, np.uint64)
    body_off[1:] = np.cumsum(blen)
    body = bytes(rng.integers(0, 256, size=int(body_off[n]), dtype=np.uint8))
    b = {"target": target, "target_ext": exts(), "sender_grain": sender, "sender_ext": exts(),
         "sender_act": sender_act, "options": options, "generic": idx(), "debug": idx(),
         "id_base": int(rng.integers(-(1 << 62), 1 << 62)), "ttl_ticks": int(rng.integers(1, 1 << 40)),
         "body": body, "body_off": body_off}
    status = rng.choice([ROUTE_OK, ROUTE_MISS, 4, 7], size=n, p=[0.9, 0.08, 0.01, 0.01]).astype(np.uint8)
    silo = rng.integers(0, len(t.silos), size=n).astype(np.uint32)
    silo[rng.random(n) < 0.02] = len(t.silos) + 3
    act = rng.choice(good, size=n).astype(np.uint32)
    noid = rng.random(n) < 0.01
    act[noid] = rng.choice(bad, size=int(noid.sum())).astype(np.uint32)
    route = {"silo": silo, "act": act, "status": status, "placed": rng.integers(0, 4, size=n).astype(np.uint8),
             "new_type": np.where(rng.random(n) < 0.3, rng.integers(0, len(t.types) + 1, size=n), NONE32).astype(np.uint32)}
    return b, route
