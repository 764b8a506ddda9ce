"""The maintainer's models against each other (CPU): the literal transcription (a) of tests/_maintain_ref.py equals the
array-form rules (b) on random histories; without the maintainer calls (a) equals oracle/dircache.py; and the
generators the GPU tests use produce every case they are meant to."""
import numpy as np
import pytest

import _maintain_ref as M
import dircache as co
import oracle as o

TC = o.grain_type_code(o.PING_GRAIN_CLASS)


def universe(n):
    ks = o.grain_keys(TC, np.arange(n, dtype=np.int64))
    return [tuple(int(x) for x in k) for k in ks]


def owners_of(keys, mode):
    spec = o.ring_spec(o.bench_silos(8), mode)
    arr = np.array(keys, dtype=np.uint64)
    own = o.ring_owner_np(spec, o.jenkins_u64x3_np(arr[:, 0], arr[:, 1], arr[:, 2]))
    return {k: int(w) for k, w in zip(keys, own)}


class LiteralSut:
    """(a) behind the driver's interface; the enumeration order is a random permutation of the stored keys."""

    def __init__(self, cache: M.AdaptiveCache, rng, owner_of, my_silos):
        self.c, self.rng, self.owner_of, self.my = cache, rng, owner_of, my_silos
        self.now = 0
        self._order = None

    def add(self, keys, acts, silos, vers):
        for k, a, s, v in zip(keys, acts, silos, vers):
            self.c.add_or_update(k, [(a, s)], v, self.now)

    def lookup(self, keys):
        out = []
        for k in keys:
            r = self.c.look_up(k)
            out.append(None if r is None else (r[0][0] if r[0] else M.EMPTY_VAL) + (r[1],))
        return out

    def route(self, keys):
        for k in keys:
            if self.owner_of(k) not in self.my:
                self.c.look_up(k)
        return True

    def remove(self, keys):
        return [self.c.remove(k) for k in keys]

    def clock(self, now):
        self.now = now

    def order(self):
        ks = list(self.c.cache.cache)
        self._order = [ks[i] for i in self.rng.permutation(len(ks))]
        return self._order

    def scan(self, now):
        self.now = now
        cnt, lists = M.maintainer_run(self.c, self._order, now, self.owner_of, self.my)
        return cnt, [(ow, [g for g, _ in l], [t for _, t in l]) for ow, l in lists.items()]

    def apply(self, now, keys, kinds, vals, tags):
        self.now = now
        st = []
        for k, kd, v, t in zip(keys, kinds, vals, tags):
            had = k in self.c.cache.cache
            M.process_response(self.c, M.response_of([(k, kd, v[0], v[1], t)]), now)
            st.append({M.LM_UPDATED: M.CR_UPDATED, M.LM_HOST: M.CR_SKIPPED,
                       M.LM_ABSENT: M.CR_REMOVED if had else M.CR_NOT_PRESENT,
                       M.LM_SAME: M.CR_FRESHENED if had else M.CR_NOT_PRESENT}[kd])
        return st

    def dump(self):
        return self.c.dump()

    def stats(self):
        return self.c.cache.next_generation, self.c.num_accesses, self.c.num_hits


@pytest.mark.parametrize("max_size", [1, 7, 64])
@pytest.mark.parametrize("mode", ["D", "V"])
def test_literal_equals_arrays_and_generators_cover(max_size, mode):
    cover = {}
    keys = universe(3 * max_size + 20)
    own = owners_of(keys, mode)
    for li, local in enumerate(([], [0], [0, 3])):
        rng = np.random.default_rng(1000 * max_size + 10 * li + (mode == "V"))
        a = M.AdaptiveCache(*M.DEFAULTS, max_size)
        b = M.Arrays(max_size)
        sut = LiteralSut(a, rng, own.__getitem__, set(local))
        M.drive(rng, sut, M.CpuOwner({0, 1, 2, 3, 4, 6, 7}), b, own.__getitem__, set(local), keys, 120, cover)
    if max_size == 64:
        for c in (M.SELF_OWNED, M.FRESH, M.DROPPED, M.REFRESH):
            assert cover.get(("scan", c), 0) > 0, ("scan class", c, cover)
        for k in (M.LM_SAME, M.LM_ABSENT, M.LM_UPDATED, M.LM_HOST, "invalid"):
            assert cover.get(("lm", k), 0) > 0, ("LookUpMany kind", k, cover)
        for s in (M.CR_UPDATED, M.CR_REMOVED, M.CR_FRESHENED, M.CR_SKIPPED):
            assert cover.get(("cr", s), 0) > 0, ("apply status", s, cover)


@pytest.mark.parametrize("max_size", [1, 7, 64])
def test_literal_without_maintainer_equals_dircache(max_size):
    rng = np.random.default_rng(5 + max_size)
    keys = universe(3 * max_size + 20)
    a = M.AdaptiveCache(*M.DEFAULTS, max_size)
    oc = co.DirectoryCacheOracle(max_size)
    for step in range(300):
        op = int(rng.integers(0, 3))
        for i in rng.integers(0, len(keys), size=int(rng.integers(1, 12))):
            k = keys[int(i)]
            if op == 0:
                act, silo, ver = int(rng.integers(0, 1 << 20)), int(rng.integers(0, 8)), int(rng.integers(0, 1000))
                a.add_or_update(k, [(act, silo)], ver, step)
                oc.add_or_update(k, act, silo, ver)
            elif op == 1:
                r, w = a.look_up(k), oc.lookup(k)
                assert (None if r is None else r[0][0] + (r[1],)) == w
            else:
                assert a.remove(k) == oc.remove(k)
        assert {k: v[:4] for k, v in a.dump().items()} == oc.key_values()
        assert (a.cache.next_generation, a.num_accesses, a.num_hits) == (oc.next_generation, oc.num_accesses, oc.num_hits)


def test_timer_growth_rule():
    b = M.Arrays(4, initial=7, max_timer=100, growth=1.5)
    a = M.AdaptiveCache(7, 100, 1.5, 4)
    k = universe(1)[0]
    b.add([k], [1], [1], [5])
    a.add_or_update(k, [(1, 1)], 5, 0)
    for want in (10, 15, 22, 33, 49, 73, 100, 100):
        b.apply(1, [k], [M.LM_SAME], [(0, 0)], [5])
        a.mark_as_fresh(k, 1)
        assert b.e[k][5] == want and a.dump()[k][5] == want


def test_duplicate_in_response_is_refused():
    b = M.Arrays(4)
    k = universe(1)[0]
    b.add([k], [1], [1], [5])
    with pytest.raises(ValueError):
        b.apply(1, [k, k], [M.LM_SAME, M.LM_ABSENT], [(0, 0)] * 2, [5, -1])


def test_full_cache_apply_evicts_later_same():
    """max_size 7, full: UPDATED items ahead of SAME items whose entries hold the lowest generations -- each
    AdjustSize evicts one of them, and its SAME then finds nothing.  (a) and (b) agree."""
    keys = universe(9)
    a = M.AdaptiveCache(*M.DEFAULTS, 7)
    b = M.Arrays(7)
    for k in keys[:7]:
        a.add_or_update(k, [(1, 1)], 5, 0)
    b.add(keys[:7], [1] * 7, [1] * 7, [5] * 7)
    batch = [keys[7], keys[8], keys[0], keys[1], keys[2]]
    kinds = [M.LM_UPDATED, M.LM_UPDATED, M.LM_SAME, M.LM_SAME, M.LM_SAME]
    vals = [(2, 2)] * 5
    tags = [9, 9, 5, 5, 5]
    st = b.apply(10, batch, kinds, vals, tags)
    assert st == [M.CR_UPDATED, M.CR_UPDATED, M.CR_NOT_PRESENT, M.CR_NOT_PRESENT, M.CR_FRESHENED]
    M.process_response(a, M.response_of([(k, kd, v[0], v[1], t) for k, kd, v, t in zip(batch, kinds, vals, tags)]), 10)
    assert a.dump() == b.dump()
