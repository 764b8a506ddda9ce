"""The directory cache's maintainer, for tests/test_maintain_ref.py (CPU) and tests/test_gpu_maintain.py:

(a) a literal transcription of the reference: LRU (src/Orleans.Core/Utils/LRU.cs), AdaptiveGrainDirectoryCache and its
    entry (src/Orleans.Runtime/GrainDirectory/AdaptiveGrainDirectoryCache.cs), AdaptiveDirectoryCacheMaintainer.Run,
    BuildGrainAndETagList and ProcessCacheRefreshResponse (AdaptiveDirectoryCacheMaintainer.cs) and
    RemoteGrainDirectory.LookUpMany (RemoteGrainDirectory.cs:65-96), cited line by line.  The enumeration order of the
    ConcurrentDictionary and DateTime.UtcNow are explicit arguments.
(b) Arrays: the gd_cache_scan / gd_dir_lookup_many / gd_cache_refresh_apply rules in array form -- what the entry points
    must give bit for bit.
(c) generators for the GPU tests; test_maintain_ref.py asserts what they cover.

A key is (n0, n1, tcd) or, for a KeyExt entry, (n0, n1, tcd, bytes).  A value is the address list: [] or [(act, silo)].
"""
import struct

import numpy as np

NONE32 = 0xFFFFFFFF
ACT_MULTI = 0xFFFFFFFE
EMPTY_VAL = (NONE32, 0xFFFF)                       # how the library shows a cached empty address list
NO_ETAG = -1                                       # GrainInfo.NO_ETAG
SEEN, SELF_OWNED, FRESH, DROPPED, REFRESH = range(5)
LM_SAME, LM_ABSENT, LM_UPDATED, LM_HOST = range(4)
CR_UPDATED, CR_REMOVED, CR_NOT_PRESENT, CR_FRESHENED, CR_SKIPPED, CR_DEFERRED = range(6)
TICKS_S = 10_000_000
DEFAULTS = (30 * TICKS_S, 240 * TICKS_S, 2.0)      # GrainDirectoryOptions.cs:31-55


def c_double_to_long(x: float) -> int:
    """(long)x for a double inside the long range: truncation."""
    return int(x)


# ---- (a) the literal transcription ----------------------------------------------------------------------

class TimestampedValue:                            # LRU.cs:51-63
    def __init__(self, lru, v):
        lru.next_generation += 1                   # :59
        self.generation = lru.next_generation
        self.value = v


class LRU:
    def __init__(self, max_size):                  # :76-86
        assert max_size > 0
        self.maximum_size = max_size
        self.next_generation = 0                   # :46
        self.generation_to_free = 0                # :47
        self.cache = {}

    def add(self, key, value):                     # :88-93
        self.adjust_size()
        self.cache[key] = TimestampedValue(self, value)

    def remove_key(self, key):                     # :101-109
        return self.cache.pop(key, None) is not None

    def clear(self):                               # :111-122
        self.cache.clear()

    def try_get_value(self, key):                  # :124-151 (maxAge is TimeSpan.MaxValue: the age check never fires)
        r = self.cache.get(key)
        if r is None:
            return None
        self.next_generation += 1                  # :132
        r.generation = self.next_generation
        return r.value

    def get(self, key):                            # :153-163 (no fetcher)
        return self.try_get_value(key)

    def adjust_size(self):                         # :165-182
        while len(self.cache) >= self.maximum_size:
            self.generation_to_free += 1
            for k, tv in list(self.cache.items()):
                if tv.generation == self.generation_to_free:
                    del self.cache[k]
                    break
            else:
                # generations only grow: once generation_to_free passes every live one nothing would ever match
                assert self.generation_to_free <= self.next_generation


class Entry:                                       # AdaptiveGrainDirectoryCache.cs:9-47; Created (:13) is never read
    def __init__(self, value, etag, expiration_timer, now):   # :27-35
        self.value = value
        self.etag = etag
        self.expiration_timer = expiration_timer
        self.last_refreshed = now
        self.num_accesses = 0

    def is_expired(self, now):                     # :37-40
        return now >= self.last_refreshed + self.expiration_timer

    def refresh(self, new_timer, now):             # :42-46
        self.last_refreshed = now
        self.expiration_timer = new_timer


class AdaptiveCache:
    def __init__(self, initial, max_timer, growth, max_size):   # :63-70
        self.cache = LRU(max_size)
        self.initial, self.max_timer, self.growth = initial, max_timer, growth
        self.num_accesses = 0
        self.num_hits = 0

    def add_or_update(self, key, value, version, now):   # :74-80
        self.cache.add(key, Entry(value, version, self.initial, now))

    def remove(self, key):                         # :82-86
        return self.cache.remove_key(key)

    def clear(self):                               # :88-91
        self.cache.clear()

    def look_up(self, key):                        # :93-110
        self.num_accesses += 1
        tmp = self.cache.try_get_value(key)
        if tmp is None:
            return None
        self.num_hits += 1
        tmp.num_accesses += 1                      # :106
        return tmp.value, tmp.etag

    def mark_as_fresh(self, key, now):             # :127-136
        r = self.cache.try_get_value(key)
        if r is None:
            return False
        new_timer = min(self.max_timer, c_double_to_long(float(r.expiration_timer) * self.growth))   # :132
        r.refresh(new_timer, now)
        return True

    def get(self, key):                            # :138-141
        return self.cache.get(key)

    # what the dumps show
    def dump(self):
        """key -> (act, silo, etag, generation, refreshed, timer, num_accesses)."""
        out = {}
        for k, tv in self.cache.cache.items():
            e = tv.value
            a, s = e.value[0] if e.value else EMPTY_VAL
            out[k] = (a, s, e.etag, tv.generation, e.last_refreshed, e.expiration_timer, e.num_accesses)
        return out


def maintainer_run(cache: AdaptiveCache, order, now, owner_of, my_silos):
    """AdaptiveDirectoryCacheMaintainer.Run's loop body (:57-124) over the keys in `order` (the enumeration of
    cache.GetStoredEntries()), then SendBatchCacheRefreshRequests' lists (:133-153).  Returns (counts, lists):
    counts = [seen, cnt1, cnt2, cnt3, cnt4]; lists = insertion-ordered dict owner -> [(grain, etag)]."""
    fetch = {}                                     # :57
    cnt = [0, 0, 0, 0, 0]
    for grain in order:                            # :66-67
        tv = cache.cache.cache.get(grain)
        assert tv is not None, "the enumeration holds only stored entries"
        entry = tv.value
        cnt[0] += 1
        owner = owner_of(grain)                    # :73
        if owner in my_silos:                      # :79
            cache.remove(grain)                    # :84
            cnt[1] += 1
        elif not entry.is_expired(now):            # :95
            cnt[2] += 1
        elif entry.num_accesses == 0:              # :100
            cache.remove(grain)                    # :103
            cnt[3] += 1
        else:                                      # :106-117
            fetch.setdefault(owner, []).append(grain)
            entry.num_accesses = 0
            cnt[4] += 1
    lists = {}
    for silo in fetch:                             # :135
        lists[silo] = build_grain_and_etag_list(cache, fetch[silo])
    return cnt, lists


def build_grain_and_etag_list(cache: AdaptiveCache, grains):   # :202-224
    out = []
    for grain in grains:
        entry = cache.get(grain)                   # :209 -- LRU.Get: a new generation
        if entry is not None:
            out.append((grain, entry.etag))
    return out


class Partition:
    """What LookUpMany reads of the owner's GrainDirectoryPartition: key -> (tag, act, silo); act ACT_MULTI for
    a multi-activation entry.  valid: the silos passing IsValidSilo."""

    def __init__(self, valid):
        self.d = {}
        self.valid = set(valid)

    def get_grain_etag(self, key):                 # GrainDirectoryPartition.cs:479-491
        e = self.d.get(key)
        return NO_ETAG if e is None else e[0]

    def look_up_activations(self, key):            # :385-441: (addresses, tag); the IsValidSilo filter (:427-434)
        e = self.d.get(key)
        if e is None:
            return None, 0
        if e[1] == ACT_MULTI:
            return "MULTI", e[0]
        return ([(e[1], e[2])] if e[2] in self.valid else []), e[0]


def look_up_many(partition: Partition, items):     # RemoteGrainDirectory.cs:65-96
    result = []
    for grain, etag in items:                      # :72
        cur = partition.get_grain_etag(grain)      # :74
        if cur == etag or cur == NO_ETAG:          # :75
            result.append((grain, cur, None))      # :78
        else:
            addrs, tag = partition.look_up_activations(grain)   # :83
            if addrs is not None:                  # :85
                result.append((grain, tag, addrs)) # :87
            else:
                result.append((grain, NO_ETAG, None))   # :91
    return result


def process_response(cache: AdaptiveCache, response, now):   # AdaptiveDirectoryCacheMaintainer.cs:155-193
    cnt = [0, 0, 0]
    for grain, tag, addrs in response:             # :164
        if addrs is not None:                      # :166
            cache.add_or_update(grain, addrs, tag, now)   # :170
            cnt[0] += 1
        elif tag == -1:                            # :173
            cache.remove(grain)                    # :178
            cnt[1] += 1
        else:
            cache.mark_as_fresh(grain, now)        # :188
            cnt[2] += 1
    return cnt


# ---- (b) the array-form rules ---------------------------------------------------------------------------

class Arrays:
    """The cache as the entry points see it: per entry act, silo, version, gen, refreshed, timer, nacc, in a dict
    whose array-form operations are written independently of (a) (vectorised, by sorting)."""

    def __init__(self, max_size, initial=DEFAULTS[0], max_timer=DEFAULTS[1], growth=DEFAULTS[2]):
        self.max_size, self.initial, self.max_timer, self.growth = max_size, initial, max_timer, growth
        self.e = {}                                # key -> [act, silo, ver, gen, refreshed, timer, nacc]
        self.next_gen = 0
        self.accesses = 0
        self.hits = 0
        self.clock = 0

    def _evict(self):
        while len(self.e) >= self.max_size:
            del self.e[min(self.e, key=lambda k: self.e[k][3])]

    def add(self, keys, acts, silos, vers):
        for k, a, s, v in zip(keys, acts, silos, vers):
            self._evict()
            self.next_gen += 1
            self.e[k] = [int(a), int(s), int(v), self.next_gen, self.clock, self.initial, 0]

    def remove(self, keys):
        return [self.e.pop(k, None) is not None for k in keys]

    def clear(self):
        self.e.clear()

    def lookup(self, keys):
        """Hit k of the batch takes generation next_gen + k; every hit counts one access on its entry."""
        out = []
        for k in keys:
            self.accesses += 1
            r = self.e.get(k)
            if r is not None:
                self.hits += 1
                self.next_gen += 1
                r[3] = self.next_gen
                r[6] += 1
            out.append(None if r is None else (r[0], r[1], r[2]))
        return out

    def scan(self, order, now, owner_of, my_silos):
        """gd_cache_scan: (counts[5], owner[], offsets[], keys[], etags[])."""
        self.clock = now
        order = list(order)
        n = len(order)
        own = np.array([owner_of(k) for k in order], dtype=np.int64)
        rec = [self.e[k] for k in order]
        local = np.array([o in my_silos for o in own], dtype=bool) if n else np.zeros(0, bool)
        expired = np.array([now >= r[4] + r[5] for r in rec], dtype=bool) if n else np.zeros(0, bool)
        accessed = np.array([r[6] != 0 for r in rec], dtype=bool) if n else np.zeros(0, bool)
        cls = np.where(local, SELF_OWNED, np.where(~expired, FRESH, np.where(accessed, REFRESH, DROPPED)))
        counts = [n] + [int((cls == c).sum()) for c in (SELF_OWNED, FRESH, DROPPED, REFRESH)]
        for i in np.nonzero((cls == SELF_OWNED) | (cls == DROPPED))[0]:
            del self.e[order[i]]
        cand = np.nonzero(cls == REFRESH)[0]
        first = {}
        for i in cand:
            first.setdefault(int(own[i]), int(i))
        owners = sorted(first, key=first.get)
        rank = {o: r for r, o in enumerate(owners)}
        grouped = sorted(cand, key=lambda i: (rank[int(own[i])], i))       # stable partition by owner rank
        offsets = [0]
        for o in owners:
            offsets.append(offsets[-1] + int((own[cand] == o).sum()))
        keys, etags = [], []
        for j, i in enumerate(grouped):
            r = self.e[order[i]]
            r[6] = 0
            r[3] = self.next_gen + j + 1
            keys.append(order[i])
            etags.append(r[2])
        self.next_gen += len(grouped)
        return counts, owners, offsets, keys, etags

    def apply(self, now, keys, kinds, vals, tags):
        """gd_cache_refresh_apply: the per-item status.  Raises ValueError where the library gives GD_EINVAL."""
        self.clock = now
        found = [k for k, kd in zip(keys, kinds) if kd != LM_HOST and k in self.e]
        if len(found) != len(set(found)):
            raise ValueError("two items name one cached entry")
        st = []
        for k, kd, v, t in zip(keys, kinds, vals, tags):
            if kd == LM_UPDATED:
                a, s = (EMPTY_VAL if int(v[1]) == NONE32 else (int(v[0]), int(v[1])))
                self.add([k], [a], [s], [t])
                st.append(CR_UPDATED)
            elif kd == LM_ABSENT:
                st.append(CR_REMOVED if self.e.pop(k, None) is not None else CR_NOT_PRESENT)
            elif kd == LM_SAME:
                r = self.e.get(k)
                if r is None:
                    st.append(CR_NOT_PRESENT)
                    continue
                self.next_gen += 1
                r[3] = self.next_gen
                grown = struct.unpack("<q", struct.pack("<q", int(np.float64(r[5]) * np.float64(self.growth))))[0]
                r[5] = min(self.max_timer, grown)
                r[4] = now
                st.append(CR_FRESHENED)
            else:
                st.append(CR_SKIPPED)
        return st

    def dump(self):
        return {k: tuple(r) for k, r in self.e.items()}


def lookup_many_arrays(partition: Partition, keys, etags, is_keyext):
    """gd_dir_lookup_many: (kind, act, silo, tag) per item."""
    out = []
    for k, et, kx in zip(keys, etags, is_keyext):
        if kx:
            out.append((LM_HOST, NONE32, NONE32, -1))
            continue
        e = partition.d.get(k)
        if e is None:
            out.append((LM_ABSENT, NONE32, NONE32, -1))
        elif e[0] == et:
            out.append((LM_SAME, NONE32, NONE32, e[0]))
        elif e[1] == ACT_MULTI:
            out.append((LM_HOST, e[1], e[2], e[0]))
        elif e[2] in partition.valid:
            out.append((LM_UPDATED, e[1], e[2], e[0]))
        else:
            out.append((LM_UPDATED, NONE32, NONE32, e[0]))
    return out


def response_of(kinds_vals):
    """(b)'s (key, kind, act, silo, tag) items as (a)'s response tuples; HOST items are left out."""
    out = []
    for k, kd, a, s, t in kinds_vals:
        if kd == LM_SAME:
            out.append((k, t, None))
        elif kd == LM_ABSENT:
            out.append((k, -1, None))
        elif kd == LM_UPDATED:
            out.append((k, t, [] if s == NONE32 else [(a, s)]))
    return out


# ---- (c) generators -------------------------------------------------------------------------------------

def tag_of(rng):
    return int(rng.integers(0, 1 << 31))


def make_partition(rng, keys, valid, n_silos=8):
    """The owner's entries for `keys`: most single-activation on a random silo, some multi-activation."""
    p = Partition(valid)
    for k in keys:
        multi = rng.random() < 0.1
        p.d[k] = (tag_of(rng), ACT_MULTI if multi else int(rng.integers(0, 1 << 20)), int(rng.integers(0, n_silos)))
    return p


def reregister_third(rng, p: Partition, keys, n_silos=8):
    """Between scan and lookup: a third of the owner's entries change -- removed, or re-registered under a new tag
    (possibly on an invalid silo, possibly as a multi-activation grain)."""
    for k in keys:
        if k not in p.d or rng.random() >= 1 / 3:
            continue
        r = rng.random()
        if r < 0.3:
            del p.d[k]
        else:
            p.d[k] = (tag_of(rng), ACT_MULTI if r > 0.9 else int(rng.integers(0, 1 << 20)), int(rng.integers(0, n_silos)))


def drive(rng, sut, owner, model: Arrays, owner_of, my_silos, universe_keys, steps, cover, ext_of=None):
    """One random history over `sut` (the system under test) and the model (b), compared after every step.

    sut: add(keys, acts, silos, vers), lookup(keys) -> [None | (act, silo, ver)], route(keys) or None, remove(keys) ->
    [bool], clock(now), order() -> the enumeration order, scan(now) -> (counts, [(owner, [keys], [etags])]),
    apply(now, keys, kinds, vals, tags) -> [status], dump() -> model.dump()'s shape, stats() -> (next_gen, accesses, hits).
    owner: ensure(keys, rng) -> [None | (act, silo, tag)] (registers most of the keys it does not hold), churn(keys, rng)
    (a third of them removed or re-registered), lookup_many(keys, etags) -> [(kind, act, silo, tag)].
    cover: a dict of counters the caller asserts on."""
    now = 1_000_000_000
    nk = len(universe_keys)

    def pick():
        k = int(rng.integers(1, max(2, min(nk, 2 * model.max_size + 4))))
        return [universe_keys[int(i)] for i in rng.integers(0, nk, size=k)]

    def check(what):
        assert sut.dump() == model.dump(), what
        assert sut.stats() == (model.next_gen, model.accesses, model.hits), what

    for step in range(steps):
        op = int(rng.integers(0, 7))
        keys = pick()
        if op == 0 or step == 0:
            # what a remote lookup on the owner returned (LocalGrainDirectory.cs:920), or made-up values
            info = owner.ensure(keys, rng)
            acts = [int(rng.integers(0, 1 << 20)) if r is None else r[0] for r in info]
            silos = [int(rng.integers(0, 8)) if r is None else r[1] for r in info]
            vers = [int(rng.integers(0, 1 << 31)) if r is None else r[2] for r in info]
            sut.add(keys, acts, silos, vers)
            model.add(keys, acts, silos, vers)
        elif op == 1:
            assert sut.lookup(keys) == model.lookup(keys), step
        elif op == 2:
            routed = sut.route(keys)
            if routed is not None:
                nl = [k for k in keys if owner_of(k) not in my_silos]
                model.lookup(nl)
        elif op == 3:
            assert list(sut.remove(keys)) == model.remove(keys), step
        elif op == 4:
            now += int(rng.choice([1, model.initial // 2, model.initial, model.max_timer]))
            sut.clock(now)
            model.clock = now
        else:
            # the maintainer's cycle: scan, LookUpMany on the owner, the response
            now += int(rng.choice([0, model.initial // 3, model.initial]))
            order = sut.order()
            assert set(order) == set(model.e), step
            counts, lists = sut.scan(now)
            mc, mo, moff, mk, me = model.scan(order, now, owner_of, my_silos)
            assert list(counts) == mc, (step, counts, mc)
            assert [o for o, _, _ in lists] == mo, step
            assert [k for _, ks, _ in lists for k in ks] == mk, step
            assert [int(t) for _, _, ts in lists for t in ts] == me, step
            assert [len(ks) for _, ks, _ in lists] == [moff[i + 1] - moff[i] for i in range(len(mo))], step
            for c in (SELF_OWNED, FRESH, DROPPED, REFRESH):
                cover[("scan", c)] = cover.get(("scan", c), 0) + mc[c]
            check(("scan", step))
            if mk:
                owner.churn(mk, rng)
                res = owner.lookup_many(mk, me)
                for kind, a, s, t in res:
                    cover[("lm", kind)] = cover.get(("lm", kind), 0) + 1
                    if kind == LM_UPDATED and s == NONE32:
                        cover[("lm", "invalid")] = cover.get(("lm", "invalid"), 0) + 1
                perm = rng.permutation(len(mk))
                bk = [mk[i] for i in perm]
                kinds = [res[i][0] for i in perm]
                vals = [(res[i][1], res[i][2]) for i in perm]
                tags = [res[i][3] for i in perm]
                now += int(rng.integers(0, 3))
                st = list(sut.apply(now, bk, kinds, vals, tags))
                assert st == model.apply(now, bk, kinds, vals, tags), step
                for s in st:
                    cover[("cr", s)] = cover.get(("cr", s), 0) + 1
        check((op, step))


class CpuOwner:
    """The owner side on the CPU: (b)'s rule, checked against (a)'s LookUpMany on every call."""

    def __init__(self, valid, n_silos=8):
        self.p = Partition(valid)
        self.n_silos = n_silos

    def ensure(self, keys, rng):
        out = []
        for k in keys:
            if k not in self.p.d and rng.random() < 0.9:
                multi = rng.random() < 0.1
                self.p.d[k] = (tag_of(rng), ACT_MULTI if multi else int(rng.integers(0, 1 << 20)),
                               int(rng.integers(0, self.n_silos)))
            e = self.p.d.get(k)
            out.append(None if e is None else (e[1], e[2], e[0]))
        return out

    def churn(self, keys, rng):
        reregister_third(rng, self.p, keys, self.n_silos)

    def lookup_many(self, keys, etags):
        res = lookup_many_arrays(self.p, keys, etags, [len(k) == 4 for k in keys])
        lit = look_up_many(self.p, list(zip(keys, etags)))
        want = [(k, t, None if a is None else ("MULTI" if a == "MULTI" else a)) for k, t, a in lit]
        got = []
        for k, (kind, a, s, t) in zip(keys, res):
            if kind == LM_HOST:
                got.append((k, t, "MULTI"))
            else:
                got.extend(response_of([(k, kind, a, s, t)]))
        assert got == want
        return res
