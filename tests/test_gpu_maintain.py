"""GPU parity for the directory cache's maintainer: the per-entry adaptive state, gd_cache_scan,
gd_dir_lookup_many and gd_cache_refresh_apply through the binding, against the models of tests/_maintain_ref.py.
Entries, generations, ages, per-entry access counts, the statistics and the request lists are compared exactly;
e.cache_entries*() supplies the slot order the model enumerates in."""
import numpy as np
import pytest

import _maintain_ref as M
import keyext as kxo
import oracle as o

pytestmark = pytest.mark.gpu

TC = o.grain_type_code(o.PING_GRAIN_CLASS)
SILOS = [(s.ip, s.port, s.gen) for s in o.bench_silos(8)]
VALID = [0, 1, 2, 3, 4, 6, 7]


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


def tkeys(ids):
    return [tuple(int(x) for x in k) for k in o.grain_keys(TC, np.asarray(ids, dtype=np.int64))]


def karr(keys):
    return np.array([k[:3] for k in keys], dtype=np.uint64).reshape(-1, 3)


def exts_of(keys):
    return None if all(len(k) == 3 for k in keys) else [k[3] if len(k) == 4 else None for k in keys]


class GpuSut:
    def __init__(self, gd, max_size, mode="D", local=(), cfg=None):
        self.e = gd.GrainDispatch(device=0, table_capacity=1024)
        self.e.ring_set_silos(mode, SILOS)
        self.e.cache_configure(max_size, list(local), 8)
        if cfg:
            self.e.cache_maintain_configure(*cfg, 0)

    def add(self, keys, acts, silos, vers):
        self.e.cache_add(karr(keys), acts, silos, vers, exts_of(keys))

    def lookup(self, keys):
        f, a, s, v = self.e.cache_lookup(karr(keys), exts_of(keys))
        return [(int(a[i]), int(s[i]), int(v[i])) if f[i] else None for i in range(len(keys))]

    def route(self, keys):
        self.e.route(karr(keys))
        return True

    def remove(self, keys):
        return [bool(x) for x in self.e.cache_remove(karr(keys), exts_of(keys))]

    def clock(self, now):
        self.e.cache_clock_set(now)

    def order(self):
        return list(self.e.cache_entries_ext())

    def scan(self, now):
        counts, lists = self.e.cache_scan(now)
        out = []
        for ow, (ks, ets, xs) in lists.items():
            keys = [tuple(int(v) for v in k) + (() if x is None else (x,)) for k, x in zip(ks, xs)]
            out.append((ow, keys, [int(t) for t in ets]))
        return counts, out

    def apply(self, now, keys, kinds, vals, tags):
        return [int(x) for x in self.e.cache_refresh_apply(now, karr(keys), kinds, [v[0] for v in vals],
                                                           [v[1] for v in vals], tags, exts_of(keys))]

    def dump(self):
        ent = self.e.cache_entries_ext()
        r, t, a = self.e.cache_entries_age()
        assert len(ent) == len(r)
        return {k: v + (int(r[i]), int(t[i]), int(a[i])) for i, (k, v) in enumerate(ent.items())}

    def stats(self):
        st = self.e.cache_stats()
        return st["next_generation"], st["accesses"], st["hits"]

    def close(self):
        self.e.close()


class GpuOwner:
    """A second handle that owns the grains; the model's partition is read back from it (its VersionTags are the
    library's) and gd_dir_lookup_many is compared with the model on every call."""

    def __init__(self, gd):
        self.e = gd.GrainDispatch(device=0, table_capacity=4096)
        self.e.ring_set_silos("D", SILOS)
        self.e.set_valid_silos(VALID, 8)
        self.p = M.Partition(VALID)
        self.shadow = {}

    def _upsert(self, keys, rng):
        acts = [M.ACT_MULTI if rng.random() < 0.1 else int(rng.integers(0, 1 << 20)) for _ in keys]
        silos = [int(rng.integers(0, 8)) for _ in keys]
        self.e.set_valid_silos(range(8), 8)            # a registration on a silo that stops being valid later
        self.e.upsert(karr(keys), acts, silos)
        self.e.set_valid_silos(VALID, 8)
        for k, a, s in zip(keys, acts, silos):
            self.shadow[k] = (a, s)

    def _sync(self, keys):
        keys = list(dict.fromkeys(keys))
        if not keys:
            return
        _, _, tags, found = self.e.lookup_tagged(karr(keys))
        for k, t, f in zip(keys, tags, found):
            if f:
                self.p.d[k] = (int(t),) + self.shadow[k]
            else:
                self.p.d.pop(k, None)
                self.shadow.pop(k, None)

    def ensure(self, keys, rng):
        new = [k for k in dict.fromkeys(keys) if k not in self.p.d and rng.random() < 0.9]
        if new:
            self._upsert(new, rng)
        self._sync(keys)
        return [None if k not in self.p.d else (self.p.d[k][1], self.p.d[k][2], self.p.d[k][0]) for k in keys]

    def churn(self, keys, rng):
        gone, again = [], []
        for k in dict.fromkeys(keys):
            if k not in self.p.d or rng.random() >= 1 / 3:
                continue
            if rng.random() < 0.3 and self.p.d[k][1] != M.ACT_MULTI:
                gone.append(k)
            else:
                again.append(k)
        if gone:
            self.e.unregister(karr(gone), [self.p.d[k][1] for k in gone])
        if again:
            self._upsert(again, rng)
        self._sync(gone + again)

    def lookup_many(self, keys, etags):
        kind, act, silo, tag = self.e.dir_lookup_many(karr(keys), etags)
        got = [(int(kind[i]), int(act[i]), int(silo[i]), int(tag[i])) for i in range(len(keys))]
        assert got == M.lookup_many_arrays(self.p, keys, etags, [False] * len(keys))
        return got

    def close(self):
        self.e.close()


@pytest.mark.parametrize("max_size", [1, 7, 64])
def test_random_histories(gd, max_size):
    cover = {}
    keys = tkeys(np.arange(3 * max_size + 20))
    for mode in ("D", "V"):
        for li, local in enumerate(([], [0], [0, 3])):
            rng = np.random.default_rng(1000 * max_size + 10 * li + (mode == "V"))
            sut, owner = GpuSut(gd, max_size, mode, local), GpuOwner(gd)
            own = dict(zip(keys, (int(x) for x in sut.e.ring_owner(karr(keys)))))
            M.drive(rng, sut, owner, M.Arrays(max_size), own.__getitem__, set(local), keys, 40, cover)
            sut.close()
            owner.close()
    if max_size == 64:
        for c in (M.SELF_OWNED, M.FRESH, M.DROPPED, M.REFRESH):
            assert cover.get(("scan", c), 0) > 0, ("scan class", c, cover)
        for k in (M.LM_SAME, M.LM_ABSENT, M.LM_UPDATED, M.LM_HOST, "invalid"):
            assert cover.get(("lm", k), 0) > 0, ("LookUpMany kind", k, cover)


def _pair(gd, max_size, cfg=None, mode="D", local=()):
    sut = GpuSut(gd, max_size, mode, local, cfg)
    m = M.Arrays(max_size, *(cfg or M.DEFAULTS))
    return sut, m


def _own(sut, keys):
    if exts_of(keys) is None:
        w = sut.e.ring_owner(karr(keys))
    else:
        w = sut.e.ring_owner_ext(karr(keys), exts_of(keys))
    return dict(zip(keys, (int(x) for x in w)))


def _scan_both(sut, m, now, own, local=()):
    order = sut.order()
    counts, lists = sut.scan(now)
    mc, mo, moff, mk, me = m.scan(order, now, own.__getitem__, set(local))
    assert list(counts) == mc
    assert [ow for ow, _, _ in lists] == mo
    assert [k for _, ks, _ in lists for k in ks] == mk
    assert [t for _, _, ts in lists for t in ts] == me
    assert [len(ks) for _, ks, _ in lists] == [moff[i + 1] - moff[i] for i in range(len(mo))]
    assert sut.dump() == m.dump()
    assert sut.stats() == (m.next_gen, m.accesses, m.hits)
    return mc, mo, mk, me


def _fill(sut, m, keys, now, touch=()):
    sut.clock(now)
    m.clock = now
    n = len(keys)
    args = (list(range(n)), [i % 8 for i in range(n)], [100 + i for i in range(n)])
    sut.add(keys, *args)
    m.add(keys, *args)
    if touch:
        assert sut.lookup(list(touch)) == m.lookup(list(touch))


def test_expiry_edges(gd):
    sut, m = _pair(gd, 16, (100, 1000, 2.0))
    keys = tkeys(range(4))
    own = _own(sut, keys)
    _fill(sut, m, keys, 5000, touch=[keys[0]])
    mc, *_ = _scan_both(sut, m, 5099, own)              # one tick early: nothing is expired
    assert mc == [4, 0, 4, 0, 0]
    mc, _, mk, _ = _scan_both(sut, m, 5100, own)        # now == refreshed + timer: everything is
    assert mc == [4, 0, 0, 3, 1] and mk == [keys[0]]    # accessed once: refreshed; never accessed: dropped
    sut.close()


def _freshen(sut, m, k, now):
    assert sut.lookup([k]) == m.lookup([k])
    st = sut.apply(now, [k], [M.LM_SAME], [(0, 0)], [0])
    assert st == m.apply(now, [k], [M.LM_SAME], [(0, 0)], [0]) == [M.CR_FRESHENED]
    assert sut.dump() == m.dump()
    return m.e[k][5]


@pytest.mark.parametrize("cfg,want", [
    (None, [60 * M.TICKS_S, 120 * M.TICKS_S, 240 * M.TICKS_S, 240 * M.TICKS_S]),
    ((7, 1000, 1.5), [10, 15, 22]),
    ((7, 1000, 1.0), [7, 7]),
    ((100, 50, 2.0), [50, 50]),
])
def test_timer_growth(gd, cfg, want):
    sut, m = _pair(gd, 4, cfg)
    k = tkeys([1])[0]
    _fill(sut, m, [k], 10)
    assert [_freshen(sut, m, k, 20 + i) for i in range(len(want))] == want
    sut.close()


def test_configure_refusals(gd):
    e = gd.GrainDispatch(device=0, table_capacity=1024)
    bad = [(-1, 10, 2.0), (10, -1, 2.0), (10, 10, 0.0), (10, 10, -1.0), (10, 10, float("nan")), (10, 10, float("inf")),
           (1 << 61, 10, 2.0), (10, 1 << 61, 2.0)]
    with pytest.raises(gd.GrainDispatchError):          # no cache configured
        e.cache_maintain_configure(10, 10, 2.0, 0)
    e.ring_set_silos("D", SILOS)
    e.cache_configure(4, [], 8)
    for b in bad:
        with pytest.raises(gd.GrainDispatchError) as ei:
            e.cache_maintain_configure(*b, 0)
        assert ei.value.code == gd.GD_EINVAL, b
    e.cache_maintain_configure((1 << 61) - 1, 10, 1.0, 0)
    e.close()


@pytest.mark.parametrize("shape", ["mixed", "one_owner", "own_owner"])
def test_list_ordering(gd, shape):
    sut, m = _pair(gd, 256, (100, 1000, 2.0))
    pool = tkeys(range(600))
    own = _own(sut, pool)
    if shape == "mixed":
        keys = pool[:200]
    elif shape == "one_owner":
        keys = [k for k in pool if own[k] == own[pool[0]]][:40]
    else:
        keys = list({own[k]: k for k in pool}.values())
    _fill(sut, m, keys, 0, touch=keys)
    mc, mo, mk, _ = _scan_both(sut, m, 100, own)
    assert mc[M.REFRESH] == len(keys)
    if shape == "mixed":
        assert len(mo) == len({own[k] for k in keys}) >= 4 and mo != sorted(mo)   # first seen in non-ascending silo order
    elif shape == "one_owner":
        assert len(mo) == 1
    else:
        assert len(mo) == len(keys) >= 4
    sut.close()


@pytest.mark.parametrize("max_size,cands", [(32, [0, 1]), (4096, [63, 64, 65, 300, 4096])])
def test_seams(gd, max_size, cands):
    """Candidate counts around a wave and above a workgroup's share, on the smallest table the library builds (1,024
    slots: a 64-slot one does not exist) and on one of 8,192 slots."""
    sut, m = _pair(gd, max_size, (100, 1000, 2.0))
    keys = tkeys(range(max_size))
    own = _own(sut, keys)
    assert sut.e.cache_stats()["capacity"] == max(1024, 2 * max_size)
    now = 0
    for c in cands:
        sut.e.cache_clear()
        m.clear()
        _fill(sut, m, keys, now, touch=keys[::max(1, max_size // c)][:c] if c else ())
        now += 100
        mc, *_ = _scan_both(sut, m, now, own)
        assert mc[M.REFRESH] == c and mc[M.DROPPED] == max_size - c
    sut.close()


def test_full_cache_apply_and_device_only_path(gd):
    sut, m = _pair(gd, 7)
    keys = tkeys(range(9))
    _fill(sut, m, keys[:7], 0)
    batch = [keys[7], keys[8], keys[0], keys[1], keys[2]]
    kinds = [M.LM_UPDATED, M.LM_UPDATED, M.LM_SAME, M.LM_SAME, M.LM_SAME]
    vals, tags = [(2, 2), (M.NONE32, M.NONE32), (0, 0), (0, 0), (0, 0)], [9, 9, 5, 5, 5]
    st = sut.apply(10, batch, kinds, vals, tags)
    assert st == m.apply(10, batch, kinds, vals, tags)
    assert st == [M.CR_UPDATED, M.CR_UPDATED, M.CR_NOT_PRESENT, M.CR_NOT_PRESENT, M.CR_FRESHENED]
    assert sut.dump() == m.dump() and sut.dump()[keys[8]][:2] == M.EMPTY_VAL
    # a batch without UPDATED items: the device-only path (the launch record shows no kernel of the host simulation)
    sut.e.set_kernel_timing(True)
    sut.e.kernel_times_reset()
    batch, kinds = [keys[3], keys[2], keys[0], keys[4]], [M.LM_SAME, M.LM_ABSENT, M.LM_ABSENT, M.LM_HOST]
    st = sut.apply(20, batch, kinds, [(0, 0)] * 4, [0] * 4)
    assert st == m.apply(20, batch, kinds, [(0, 0)] * 4, [0] * 4)
    assert st == [M.CR_FRESHENED, M.CR_REMOVED, M.CR_NOT_PRESENT, M.CR_SKIPPED]
    names = set(sut.e.kernel_times())
    sut.e.set_kernel_timing(False)
    assert {"k_cm_find", "k_cm_apply"} <= names
    assert not names & {"k_cache_find", "k_cache_apply", "k_cache_insert", "k_cache_count_le", "k_cache_age_of"}
    assert sut.dump() == m.dump() and sut.stats() == (m.next_gen, m.accesses, m.hits)
    # two items on one cached entry: GD_EINVAL, nothing changes (both paths)
    for kinds in ([M.LM_SAME, M.LM_ABSENT], [M.LM_UPDATED, M.LM_SAME]):
        with pytest.raises(gd.GrainDispatchError) as ei:
            sut.apply(30, [keys[3], keys[3]], kinds, [(1, 1)] * 2, [1, 1])
        assert ei.value.code == gd.GD_EINVAL
        assert sut.dump() == m.dump() and sut.stats() == (m.next_gen, m.accesses, m.hits)
    sut.close()


def test_keyext_entries(gd):
    sut, m = _pair(gd, 64, (100, 1000, 2.0))
    tcd = kxo.string_grain(TC, "x")[0]
    strings = ["plain", "grüße 世界", "", "another-key"]
    keys = [tcd + (s.encode("utf-8"),) for s in strings] + [tcd] + tkeys([5, 6])     # tcd alone: KeyExt null
    own = _own(sut, keys)
    _fill(sut, m, keys, 0, touch=keys)
    mc, mo, mk, _ = _scan_both(sut, m, 100, own)
    assert mc[M.REFRESH] == len(keys) and set(mk) == set(keys)
    # dead strings, then enough new ones to compact the heap between two scans
    big = [tcd + (bytes([65 + i]) * 3000,) for i in range(30)]
    own.update(_own(sut, big))
    for part in (big[:15], big[15:]):
        _fill(sut, m, part, 100)
        assert sut.remove(part[:10]) == m.remove(part[:10])
    assert sut.lookup(keys) == m.lookup(keys)
    mc, mo, mk, _ = _scan_both(sut, m, 200, own)
    assert set(keys) <= set(mk)
    st = sut.apply(200, keys, [M.LM_SAME] * len(keys), [(0, 0)] * len(keys), [0] * len(keys))
    assert st == m.apply(200, keys, [M.LM_SAME] * len(keys), [(0, 0)] * len(keys), [0] * len(keys))
    assert sut.dump() == m.dump()
    sut.close()


def test_state_survives_rehash_silo_removal_and_clear(gd):
    sut, m = _pair(gd, 64, (100, 1000, 2.0))
    keys = tkeys(range(900))
    own = _own(sut, keys)
    _fill(sut, m, keys[:50], 7, touch=keys[:20] + keys[:5])
    cap = sut.e.cache_stats()["capacity"]
    _fill(sut, m, keys[50:900], 9)                       # a batch past the load limit: the table grows
    assert sut.e.cache_stats()["capacity"] > cap
    assert sut.dump() == m.dump()
    _scan_both(sut, m, 50, own)
    got = sut.e.remove_silos([5])                        # AdjustLocalCache's pass
    for k in [k for k, r in m.e.items() if r[1] == 5]:
        del m.e[k]
    assert got["cache_removed"] > 0 and sut.dump() == m.dump()
    assert sut.lookup(keys[880:900]) == m.lookup(keys[880:900])
    _scan_both(sut, m, 109, own)
    sut.e.cache_clear()
    m.clear()
    assert sut.dump() == {}
    _fill(sut, m, keys[:10], 200)
    assert sut.dump() == m.dump()
    sut.close()


def test_capture_refuses_scan_and_apply(gd):
    import torch
    sut, m = _pair(gd, 16)
    keys = tkeys(range(4))
    _fill(sut, m, keys, 0, touch=keys)
    s = torch.cuda.Stream()
    x = torch.zeros(16, device="cuda:0")
    torch.cuda.synchronize()
    sut.e.set_stream(s.cuda_stream)
    codes = []
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        x.add_(1)
        for call in (lambda: sut.e.cache_scan(10 ** 12),
                     lambda: sut.apply(5, keys[:1], [M.LM_SAME], [(0, 0)], [0]),
                     lambda: sut.apply(5, keys[:1], [M.LM_UPDATED], [(1, 1)], [1])):
            with pytest.raises(gd.GrainDispatchError) as ei:
                call()
            codes.append((ei.value.code, "stream capture" in str(ei.value)))
    sut.e.set_stream(None)
    assert codes == [(gd.GD_ESTATE, True)] * 3
    assert sut.dump() == m.dump()
    sut.close()
