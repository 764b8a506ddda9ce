"""Reference for the sniff stage (gd_sniff_*, gd_cache_invalidate*) -- TEST INFRASTRUCTURE ONLY.

InsideRuntimeClient.SniffIncomingMessage (InsideRuntimeClient.cs:253-263) -> LocalGrainDirectory.InvalidateCacheEntry
(LocalGrainDirectory.cs:965-976) -> DirectoryCache.LookUp + RemoveActivations (:1146-1164), in two independent forms:

  * sniff_messages: per message.  Parses the frame's CacheInvalidationHeader with _forward_ref.read_invalidation and
    calls invalidate_cache_entry, a line-by-line restatement, on oracle/dircache.py's DirectoryCacheOracle.
  * sniff_vectorised: a struct walk of its own over the header, then numpy over the whole batch: the first matching
    entry of every key, the hit flags, the generations by prefix sum.

A cache entry's value is (act, silo, version) as the library stores it: act GD_ACT_MULTI = a list C# holds,
silo 0xFFFF = the cached empty list.  Keys are (n0, n1, tcd) or (n0, n1, tcd, KeyExt bytes).
"""
import struct

import numpy as np

import dircache as co
import headers as H
import _forward_ref as F
from _encode_ref import Bad, frame_lengths

SNIFF_NONE, SNIFF_OK, SNIFF_MALFORMED = range(3)
FLAG_RETURNED, FLAG_UNKNOWN = 1, 2
INV_MISS, INV_REMOVED, INV_KEPT, INV_HOST, INV_NO_ID = range(5)
ACT_MULTI, NO_ACT, EMPTY_SILO = 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFF
KEYEXT_NULL = -1
KX_TCD = (6 << 56) | 0x2A2A2A2A
PLAIN_TCD = (3 << 56) | 0x11
KX_LENGTHS = (0, 1, 12, 13, 40, 63, 64, 65, 100)          # around KX_FAST_BYTES (64) and the inline sizes


def is_keyext(tcd):
    return (tcd >> 56) in (6, 7)


def cache_key(grain, ext):
    """The LRU's key: a KeyExt-category grain with a string is keyed by it; any other by its three words."""
    k = tuple(int(x) for x in grain)
    return k + (bytes(ext),) if ext is not None and is_keyext(k[2]) else k


class Cache:
    """DirectoryCacheOracle plus what it does not keep: NumAccesses an entry (AdaptiveGrainDirectoryCache.cs:25,106)."""

    def __init__(self, max_size, act_ids):
        self.lru = co.DirectoryCacheOracle(max_size)
        self.nacc = {}
        self.act_ids = np.asarray(act_ids, np.uint64).reshape(-1, 3)

    def add(self, key, act, silo, version):
        self.lru.add_or_update(key, act, silo, version)
        self.nacc[key] = 0

    def act_id(self, act):
        if act >= len(self.act_ids) or not self.act_ids[act].any():
            return None
        return tuple(int(x) for x in self.act_ids[act])

    def state(self):
        """(entries with generations, NumAccesses an entry, the statistics)."""
        kv = self.lru.key_values()
        return kv, {k: self.nacc[k] for k in kv}, (self.lru.num_accesses, self.lru.num_hits, self.lru.next_generation)


# ------------------------------------------------------------------ form (a): per message
def invalidate_cache_entry(cache, key, activation_id):
    """LocalGrainDirectory.InvalidateCacheEntry (:965-976) with RemoveActivations (:1146-1164).  activation_id: the
    three words, or None for an ActivationId the map cannot hold (one with a KeyExt string)."""
    # :973  if (DirectoryCache.LookUp(grainId, out list, out version))
    r = cache.lru.lookup(key)
    if r is None:
        return INV_MISS
    cache.nacc[key] += 1                                     # AdaptiveGrainDirectoryCache.cs:106
    act, silo, _version = r
    if act == ACT_MULTI:
        return INV_HOST                                      # the list is C#'s
    # :1148  int removeCount = activations.Count(doRemove);   doRemove = t => t.Item2.Equals(activationId)
    if silo == EMPTY_SILO:
        return INV_KEPT                                      # :1149-1152  an empty list: removeCount == 0
    cached = cache.act_id(act)
    if cached is None:
        return INV_NO_ID
    if activation_id is None or cached != tuple(activation_id):
        return INV_KEPT                                      # :1149-1152
    # :1160-1163  no activations left (the library caches one): directoryCache.Remove(key)
    cache.lru.remove(key)
    del cache.nacc[key]
    return INV_REMOVED


def frame_entries(buf, off):
    """(status, flags, entries) of the frame at off; an entry = (silo24, grain, ext bytes or None, ext offset into buf,
    activation id or None)."""
    ln = frame_lengths(buf, off)
    if ln is None:
        return SNIFF_MALFORMED, 0, []
    hl, _ = ln
    frame = bytes(buf[off:off + 8 + hl])
    m = struct.unpack_from("<I", frame, 8)[0]
    flags = FLAG_UNKNOWN if m & H.IS_RETURNED_FROM_REMOTE_CLUSTER else 0
    if not m & H.CACHE_INVALIDATION_HEADER:
        return SNIFF_NONE, flags, []
    try:
        raw, _ = F.read_invalidation(frame, 12, 8 + hl)
    except (Bad, UnicodeDecodeError):                        # bytes that are no entry: the walk leaves the header
        return SNIFF_MALFORMED, flags, []
    out, p = [], 16
    for silo, (g, gx), (a, ax) in raw:
        gxb = None if gx is None else gx.encode("utf-8")
        axb = None if ax is None else ax.encode("utf-8")
        p += 24 + 24 + 4                                     # the silo, the grain's words, its string length
        out.append((bytes(silo), g, gxb, off + p, None if axb is not None else a))
        p += (len(gxb) if gxb else 0) + 24 + 4 + (len(axb) if axb else 0)
    return SNIFF_OK, flags, out


def sniff_messages(buf, offs, cache=None):
    """The batch in order.  Returns a dict of the stage's outputs; with a cache, "inv" too and the cache changed."""
    n = len(offs)
    count, status, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    ents, inv = [], []
    for i in range(n):
        st, fl, es = frame_entries(buf, int(offs[i]))
        status[i], flags[i], count[i] = st, fl, len(es)
        for silo, g, gx, xoff, a in es:                      # InsideRuntimeClient.cs:259-262
            ents.append((i, silo, g, gx, xoff, a))
            if cache is not None:
                inv.append(invalidate_cache_entry(cache, cache_key(g, gx), a))
    m = len(ents)
    ent_off = np.zeros(n + 1, np.uint32)
    ent_off[1:] = np.cumsum(count)
    out = {"count": count, "ent_off": ent_off, "status": status, "flags": flags, "m": m,
           "ent_frame": np.array([e[0] for e in ents], np.uint32),
           "ent_silo": np.array([struct.unpack("<6I", e[1]) for e in ents], np.uint32).reshape(m, 6),
           "ent_grain": np.array([e[2] for e in ents], np.uint64).reshape(m, 3),
           "ent_ext_off": np.array([e[4] for e in ents], np.uint64),
           "ent_ext_len": np.array([KEYEXT_NULL if e[3] is None else len(e[3]) for e in ents], np.int32),
           "ent_act_id": np.array([(0, 0, 0) if e[5] is None else e[5] for e in ents], np.uint64).reshape(m, 3),
           "ent_ext": [e[3] for e in ents]}
    if cache is not None:
        out["inv"] = np.array(inv, np.uint8)
    return out


# ------------------------------------------------------------------ form (b): vectorised
def _walk(buf, off):
    """The frame's entries by a struct walk of its own: (grain, ext bytes or None, act id words, act id has a string),
    or None for a frame that contributes none."""
    n = len(buf)
    if off > n or n - off < 8:
        return None
    hl, bl, = struct.unpack_from("<ii", buf, off)
    if hl < 4 or bl < 0 or hl + bl > n - off - 8:
        return None
    if not struct.unpack_from("<I", buf, off + 8)[0] & 2:
        return None
    end, p, out = off + 8 + hl, off + 12, []
    if p + 4 > end:
        return None
    cnt = struct.unpack_from("<i", buf, p)[0]
    p += 4
    if cnt < 0:
        return None
    for _ in range(cnt):
        rec = []
        p += 24
        for _key in range(2):
            if p + 28 > end:
                return None
            w = struct.unpack_from("<QQQi", buf, p)
            p += 28
            if w[3] < -1 or p + max(w[3], 0) > end:
                return None
            rec.append((w[:3], None if w[3] < 0 else bytes(buf[p:p + w[3]])))
            p += max(w[3], 0)
        out.append((rec[0][0], rec[0][1], rec[1][0], rec[1][1] is not None))
    return out


def invalidate_vectorised(entries, kv, nacc, stats, act_ids):
    """entries: [(cache key, act id words or None)] in batch order; kv / nacc / stats: Cache.state() before the batch.
    Returns (inv u8[m], the state after) without a loop over the entries' outcomes."""
    m = len(entries)
    keys = list(kv)
    index = {k: j for j, k in enumerate(keys)}
    slot = np.array([index.get(k, -1) for k, _ in entries], np.int64).reshape(m)
    ids = np.array([(0, 0, 0) if a is None else a for _, a in entries], np.uint64).reshape(m, 3)
    has_id = np.array([a is not None for _, a in entries], bool).reshape(m)
    c_act = np.array([kv[k][0] for k in keys], np.int64).reshape(len(keys))
    c_silo = np.array([kv[k][1] for k in keys], np.int64).reshape(len(keys))
    c_gen = np.array([kv[k][3] for k in keys], np.int64).reshape(len(keys))
    table = np.asarray(act_ids, np.uint64).reshape(-1, 3)
    found = slot >= 0
    s = np.where(found, slot, 0)
    act, silo = c_act[s], c_silo[s]
    multi = found & (act == ACT_MULTI)
    empty = found & ~multi & (silo == EMPTY_SILO)
    in_map = act < len(table)
    cid = table[np.where(in_map, act, 0)] if len(table) else np.zeros((m, 3), np.uint64)
    no_id = found & ~multi & ~empty & (~in_map | ~cid.any(axis=1))
    match = found & ~multi & ~empty & ~no_id & has_id & (cid == ids).all(axis=1)
    k = np.arange(m)
    first = np.full(len(keys), m, np.int64)
    np.minimum.at(first, s[match], k[match])
    hit = found & (k <= first[s])
    inv = np.full(m, INV_MISS, np.uint8)
    inv[hit] = INV_KEPT
    inv[hit & multi] = INV_HOST
    inv[hit & no_id] = INV_NO_ID
    inv[hit & match] = INV_REMOVED                           # a matching hit is the first matching entry
    accesses, hits, next_gen = stats
    gen_of = next_gen + np.cumsum(hit)                       # hit number j takes generation next_gen + j
    np.maximum.at(c_gen, s[hit], gen_of[hit])                # the last hit of a key wins
    acc = np.array([nacc[q] for q in keys], np.int64).reshape(len(keys))
    np.add.at(acc, s[hit], 1)
    removed = first < m
    kv2 = {q: kv[q][:3] + (int(c_gen[j]),) for j, q in enumerate(keys) if not removed[j]}
    nacc2 = {q: int(acc[j]) for j, q in enumerate(keys) if not removed[j]}
    return inv, (kv2, nacc2, (accesses + m, hits + int(hit.sum()), next_gen + int(hit.sum())))


def sniff_vectorised(buf, offs, state, act_ids):
    entries = []
    for off in offs:
        for g, gx, a, a_ext in _walk(buf, int(off)) or []:
            entries.append((cache_key(g, gx), None if a_ext else a))
    return invalidate_vectorised(entries, *state, act_ids)


# ------------------------------------------------------------------ test batches
def with_invalidation(frame, entries, count=None):
    """`frame` (no invalidation header) with the header spliced in as the serializer's first field."""
    hl, bl, m = struct.unpack_from("<iiI", frame, 0)
    assert not m & H.CACHE_INVALIDATION_HEADER
    field = F.w_invalidation(entries)
    if count is not None:
        field = struct.pack("<i", count) + field[4:]
    return struct.pack("<iiI", hl + len(field), bl, m | H.CACHE_INVALIDATION_HEADER) + field + frame[12:]


def with_mask_bits(frame, bits):
    out = bytearray(frame)
    struct.pack_into("<I", out, 8, struct.unpack_from("<I", out, 8)[0] | bits)
    return bytes(out)


def silo24(s):
    return H.w_silo(*F.SILOS[s])


class Scene:
    """A cache and a received batch that meets the conditions of the GPU tests (check_conditions asserts them)."""

    def __init__(self, n, seed, cache_size=4096):
        rng = np.random.default_rng(seed)
        self.rng = rng
        n_act = 256
        ids = rng.integers(1, 1 << 62, size=(n_act, 3)).astype(np.uint64)
        self.no_id_acts = [3, 77]
        ids[self.no_id_acts] = 0
        self.act_ids = ids
        # the grains: plain ones and KeyExt ones with strings of every length class
        n_g = max(48, min(600, 2 * n))
        self.grains = []
        for j in range(n_g):
            if j % 5 == 0:
                ln = KX_LENGTHS[(j // 5) % len(KX_LENGTHS)]
                self.grains.append(((0, j, KX_TCD), ("s%d/" % j + "x" * ln)[:ln] if ln else ""))
            elif j % 23 == 1:
                self.grains.append(((0, j, KX_TCD), None))    # a KeyExt-category key with a null KeyExt
            else:
                self.grains.append(((int(rng.integers(1, 1 << 60)), j, PLAIN_TCD), None))
        # the cache: most grains; grains 1..4 are the special ones of frame 0
        self.cached = []                                      # (grain index, act, silo, version)
        good = [a for a in range(n_act) if a not in self.no_id_acts]
        for j, _ in enumerate(self.grains):
            if j % 4 == 3:
                continue                                      # never cached: MISS
            act, silo = int(rng.choice(good)), int(rng.integers(0, 5))
            if j == 2 or j % 41 == 7:
                act = ACT_MULTI
            elif j == 4 or j % 43 == 9:
                act = self.no_id_acts[j % 2]
            elif j == 6 or j % 47 == 11:
                act, silo = NO_ACT, EMPTY_SILO
            self.cached.append((j, act, silo, int(rng.integers(0, 1 << 20))))
        self.cache_size = cache_size
        self.frames = self._frames(n)

    def key(self, j):
        g, x = self.grains[j]
        return cache_key(g, None if x is None else x.encode())

    def _entry(self, j, how):
        """An entry naming grain j: how = 'match' (the cached activation's id), 'other', or 'ext' (an id with a string)."""
        c = {e[0]: e for e in self.cached}.get(j)
        a = ((int(self.rng.integers(1, 1 << 60)), 5, 0), None)
        if how == "match" and c is not None and c[1] < len(self.act_ids) and self.act_ids[c[1]].any():
            a = (tuple(int(x) for x in self.act_ids[c[1]]), None)
        elif how == "ext":
            a = ((9, 9, 0), "act")
        return silo24(int(self.rng.integers(0, 5))), self.grains[j], a

    def _frames(self, n):
        rng = self.rng
        plain = lambda: F.normal_frame(rng, n_old=0)
        frames = []
        for i in range(n):
            r = rng.random()
            if i == 0:                                        # one of everything, whatever n is
                es = [self._entry(0, "other"), self._entry(0, "match"), self._entry(3, "match"),
                      self._entry(2, "match"), self._entry(4, "match"), self._entry(6, "ext")]
                frames.append(with_invalidation(plain(), es))
            elif r < 0.30:
                es = []
                for _ in range(int(rng.integers(1, 7))):
                    j = int(rng.integers(0, len(self.grains)))
                    es.append(self._entry(j, str(rng.choice(["match", "match", "other", "ext"], p=[.3, .3, .35, .05]))))
                frames.append(with_invalidation(plain(), es))
            elif r < 0.33:
                frames.append(with_invalidation(plain(), []))   # a count of 0
            elif r < 0.36:
                frames.append(with_mask_bits(plain(), H.IS_RETURNED_FROM_REMOTE_CLUSTER))
            elif r < 0.44:
                frames.append(F.odd_frame(rng))
            else:
                frames.append(plain())
        return frames

    def pack(self, pad=b""):
        return F.pack_frames(self.frames, pad)

    def load_order(self):
        """The cached entries in the order they are added: the empty lists last (they come by a refresh response)."""
        return [c for c in self.cached if c[2] != EMPTY_SILO] + [c for c in self.cached if c[2] == EMPTY_SILO]

    def new_cache(self):
        c = Cache(self.cache_size, self.act_ids)
        for j, act, silo, ver in self.load_order():
            c.add(self.key(j), act, silo, ver)
        return c


def check_conditions(scene, want):
    """The conditions the GPU tests' random batches must meet, on form (a)'s outputs."""
    n, m, inv = len(want["count"]), want["m"], want["inv"]
    with_hdr = ((want["status"] == SNIFF_OK) & (want["count"] >= 1) & (want["count"] <= 6)).sum()
    assert with_hdr >= 0.2 * n, (with_hdr, n)
    for c in (INV_REMOVED, INV_KEPT, INV_MISS):
        assert (inv == c).sum() >= 0.1 * m, (c, (inv == c).sum(), m)
    assert (inv == INV_HOST).any() and (inv == INV_NO_ID).any()
    empty = [j for j, act, silo, _ in scene.cached if silo == EMPTY_SILO]
    on_empty = np.zeros(m, bool)
    for j in empty:
        on_empty |= (want["ent_grain"] == np.array(scene.grains[j][0], np.uint64)).all(axis=1)
    assert on_empty.any() and (inv[on_empty] == INV_KEPT).all(), "an entry on a cached empty list"
    assert (want["ent_act_id"] == 0).all(axis=1).any(), "an ActivationId with a KeyExt string"
    kx = [x for g, x in scene.grains if x is not None]
    assert len(kx) >= 0.1 * len(scene.grains)
    lens = {len(x) for x in kx}
    assert {0, 1, 12, 13} <= lens and any(l >= 40 for l in lens)
