"""The directory table and its probe indexes on long, wrapped and tombstoned chains.

The other GPU tests keep the table at load 0.03-0.3 with consecutive ids, where nearly every grain sits in
its home group of 8 slots.  Here the keys are built to share one home (_chain_keys.py), so that the code
that only matters on long chains runs on purpose: index walks past the first 64-B read, the max_probe
bound of every lookup, chains that wrap from the last slots to slot 0, tombstone reuse inside a chain, the
registration's claim protocol with many new grains colliding on one first free slot, and asynchronous
errors.  Tables of 4,096 slots (one case needs 2^18); every case under GD_OPT_PROBE 0 (the directory
probe), 2 / 3 (16-B index: group / slot reads) and 4 (8-B index); every comparison is bit-exact against
the oracle (o.route_batch_np, o.DirectoryPartition)."""
from functools import lru_cache

import numpy as np
import pytest

import oracle as o
from _chain_keys import home_slot_np, keys_with_home

pytestmark = pytest.mark.gpu

TC = o.grain_type_code(o.PING_GRAIN_CLASS)
TC2 = o.grain_type_code("UnitTests.OtherGrain")
CAP = 4096
PROBES = (0, 2, 3, 4)
HOME_MID = 2312                      # a mid-table home (8-aligned)
N_ACT = 1 << 17                      # every activation number the tests hand out is below it
SILOS = o.bench_silos(8)
BG_BASE = 1 << 28                    # background ids: far above any id the key builder reaches


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


@lru_cache(maxsize=None)
def _spec(mode):
    return o.ring_spec(SILOS, mode)


@lru_cache(maxsize=None)
def _home_keys(cap, home, count):
    """`count` keys of one home, computed once and shared (read-only)."""
    k = keys_with_home(TC, cap, home, count)
    assert int(k[-1, 1]) < BG_BASE
    k.setflags(write=False)
    return k


def _bg(lo, hi, tc=TC):
    """Background grains: consecutive ids, so their homes scatter evenly."""
    return o.grain_keys(tc, BG_BASE + np.arange(lo, hi))


def _t(k):
    return (int(k[0]), int(k[1]), int(k[2]))


class _Model:
    """An engine beside the oracle's partition: every report of a directory call is compared with
    o.DirectoryPartition item by item, routes with o.route_batch_np over the partition's entries."""

    def __init__(self, gd, probe, mode="D", cap=CAP):
        self.gd = gd
        self.e = gd.GrainDispatch(device=0, table_capacity=cap, options={"probe": probe})
        self.e.ring_set_silos(mode, [(s.ip, s.port, s.gen) for s in SILOS])
        self.spec = _spec(mode)
        self.part = o.DirectoryPartition()
        self.rng = np.random.default_rng(1000 + probe)
        self.next_act = 1

    def close(self):
        self.e.close()

    def acts(self, n):
        """n fresh activation numbers (never handed out before, all below N_ACT)."""
        a = np.arange(self.next_act, self.next_act + n, dtype=np.uint32)
        self.next_act += n
        assert self.next_act < N_ACT
        return a

    def owner(self, keys):
        return o.ring_owner_np(self.spec, o.jenkins_u64x3_np(keys[:, 2], keys[:, 0], keys[:, 1])).astype(np.uint32)

    def _want_register(self, keys, acts, silos):
        return np.array([self.part.add_single_activation(_t(k), int(a), int(s))
                         for k, a, s in zip(keys, acts, silos)], np.int64).reshape(-1, 3)

    def register(self, keys, acts=None, silos=None):
        acts = self.acts(len(keys)) if acts is None else acts
        silos = self.owner(keys) if silos is None else silos
        a, s, ins = self.e.register(keys, acts, silos)
        want = self._want_register(keys, acts, silos)
        np.testing.assert_array_equal(a, want[:, 0])
        np.testing.assert_array_equal(s, want[:, 1])
        np.testing.assert_array_equal(ins, want[:, 2])
        return ins

    def register_async(self, keys, acts=None, silos=None):
        """gd_dir_register_device_async + gd_synchronize (which must not report an error)."""
        import torch
        dev = torch.device("cuda:0")
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        acts = self.acts(len(keys)) if acts is None else acts
        silos = self.owner(keys) if silos is None else silos
        v = np.ascontiguousarray(np.stack([acts, silos], 1).astype(np.uint32))
        dk = torch.from_numpy(keys.view(np.int64)).to(dev)
        dv = torch.from_numpy(v.view(np.int32)).to(dev)
        ov = torch.empty((len(keys), 2), dtype=torch.int32, device=dev)
        oi = torch.empty(len(keys), dtype=torch.uint8, device=dev)
        self.e.register_device_async(dk.data_ptr(), dv.data_ptr(), len(keys), ov.data_ptr(), oi.data_ptr())
        self.e.synchronize()
        want = self._want_register(keys, acts, silos)
        ov = ov.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(oi.cpu().numpy(), want[:, 2])
        np.testing.assert_array_equal(ov[:, 0], want[:, 0])
        np.testing.assert_array_equal(ov[:, 1], want[:, 1])

    def unregister(self, keys, acts):
        rem = self.e.unregister(keys, acts)
        want = [int(self.part.remove_activation(_t(k), int(a))) for k, a in zip(keys, acts)]
        np.testing.assert_array_equal(rem, want)

    def unregister_cas(self, keys, acts):
        """gd_dir_unregister_device without a report: the one-launch CAS form (k_unreg_cas)."""
        import torch
        dev = torch.device("cuda:0")
        dk = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64)).to(dev)
        da = torch.from_numpy(np.ascontiguousarray(acts, dtype=np.uint32).view(np.int32)).to(dev)
        self.e.unregister_device(dk.data_ptr(), da.data_ptr(), len(keys), None)
        self.e.synchronize()
        for k, a in zip(keys, acts):
            self.part.remove_activation(_t(k), int(a))

    def upsert(self, keys, acts, silos):
        ins = self.e.upsert(keys, acts, silos)
        made = {}
        for j, (k, a, s) in enumerate(zip(keys, acts, silos)):
            k = _t(k)
            if k not in self.part.data or k in made:
                made.setdefault(k, []).append(j)
            self.part.data[k] = (int(a), int(s))           # overwrite in batch order: the last item wins
        for k, items in made.items():                      # one item of each new grain created its entry
            assert int(ins[items].sum()) == 1, (k, items)
        assert int(ins.sum()) == len(made)

    def act_of(self, keys):
        return np.array([self.part.data[_t(k)][0] for k in keys], np.uint32)

    def directory(self):
        if not self.part.data:
            return o.DirectoryArrays(np.zeros((0, 3), np.uint64), [], [])
        keys = np.array(list(self.part.data.keys()), np.uint64).reshape(-1, 3)
        vals = np.array(list(self.part.data.values()), np.uint32).reshape(-1, 2)
        return o.DirectoryArrays(keys, vals[:, 0], vals[:, 1])

    def check(self, chain, misses, pool, n=3000):
        """Routes (gd_route and gd_route_bucket), lookups and the live count against the oracle.  The batch:
        every key of the chain under test, the unregistered keys of the same home (misses that walk the
        whole chain), background keys; shuffled."""
        assert len(misses) >= 20
        q = np.concatenate([chain, misses, pool[self.rng.integers(0, len(pool), size=n - len(chain) - len(misses))]])
        q = np.ascontiguousarray(q[self.rng.permutation(len(q))])
        want = o.route_batch_np(q, self.spec, self.directory())
        st, silo, act = self.e.route(q)
        np.testing.assert_array_equal(st, want[0])
        np.testing.assert_array_equal(silo, want[1])
        np.testing.assert_array_equal(act, want[2])
        st, silo, act, perm, off = self.e.route_bucket(q, N_ACT)
        np.testing.assert_array_equal(st, want[0])
        np.testing.assert_array_equal(silo, want[1])
        np.testing.assert_array_equal(act, want[2])
        wp, wo = o.bucket_stable(want[2], N_ACT)
        np.testing.assert_array_equal(perm, wp)
        np.testing.assert_array_equal(off, wo)
        lk = np.concatenate([chain, misses, pool[:200]])
        la, ls, lf = self.e.lookup(lk)
        for i, k in enumerate(lk):
            v = self.part.lookup(_t(k))
            if v is None:
                assert (lf[i], la[i], ls[i]) == (0, o.M32, o.M32), i
            else:
                assert lf[i] == 1 and (la[i], ls[i]) == v, i
        for k in misses:
            assert _t(k) not in self.part.data
        self.check_live()

    def check_live(self):
        assert self.e.stats()["table_live"] == len(self.part.data)


def _again_with_other_values(m, keys):
    """Registered grains registered again with other values: none inserted, the old values reported
    (_Model.register compares them with the oracle's)."""
    ins = m.register(keys, m.acts(len(keys)), (m.owner(keys) + 1) % 8)
    assert not ins.any()


# ----------------------------------------------------------------------------- the chains
MID_CHAIN, MID_NEW, MID_NEW2, MID_NEW3, MID_MISS = slice(0, 40), slice(40, 60), slice(60, 80), slice(80, 100), \
    slice(105, 130)


def _mid_chain(m, cap=CAP, home=HOME_MID, n_bg=1000):
    """1,000 background grains and 40 grains of one mid-table home in one synchronous batch: the 40
    side by side in the batch, across two waves (the claim's hardest order: they collide on every
    free slot of the chain).  Returns (the home's 130 keys, the registered background, the route pool)."""
    mid = _home_keys(cap, home, 130)
    assert (home_slot_np(mid, cap) == home).all()
    bg = _bg(0, n_bg)
    m.register(np.concatenate([bg[:500], mid[MID_CHAIN], bg[500:]]))
    return mid, bg, np.concatenate([bg, _bg(n_bg, n_bg + 300)])


WRAP_A, WRAP_A_NEW, WRAP_A_MISS = slice(0, 20), slice(20, 40), slice(45, 70)
WRAP_B, WRAP_B_NEW, WRAP_B_MISS = slice(0, 12), slice(12, 22), slice(25, 50)


def _wrap_chain(m, order):
    """20 grains of the table's last home and 12 of home 0: one chain from slot cap - 8 through slot 0
    to about slot 23.  order "ab": the last home's grains first (they wrap; home 0's grains sit behind
    them), "ba": home 0's first (the last home's wrap around them)."""
    a, b = _home_keys(CAP, CAP - 8, 70), _home_keys(CAP, 0, 50)
    bg = _bg(0, 1000)
    m.register(bg)
    for grp in order:
        m.register(a[WRAP_A] if grp == "a" else b[WRAP_B])
    chain = np.concatenate([a[WRAP_A], b[WRAP_B]])
    misses = np.concatenate([a[WRAP_A_MISS], b[WRAP_B_MISS]])
    return a, b, chain, misses, np.concatenate([bg, _bg(1000, 1300)])


@pytest.mark.parametrize("mode,probe", [("D", p) for p in PROBES] + [("V", 4)])
def test_long_chain(gd, mode, probe):
    """Case 1: 40 grains of one home.  Hits at the far end of the chain and misses of the same home need
    max_probe to cover the whole chain and the index walks to go on past their first read."""
    m = _Model(gd, probe, mode)
    mid, bg, pool = _mid_chain(m)
    m.check(mid[MID_CHAIN], mid[MID_MISS], pool)
    _again_with_other_values(m, mid[MID_CHAIN])
    m.check(mid[MID_CHAIN], mid[MID_MISS], pool)
    assert m.e.stats()["table_capacity"] == CAP
    m.close()


@pytest.mark.parametrize("order", ["ab", "ba"])
@pytest.mark.parametrize("probe", PROBES)
def test_wrapped_chain(gd, probe, order):
    """Case 2: a chain across the end of the table ((s + k) & mask in the table walk, both index walks
    and the registration's four-slot step)."""
    m = _Model(gd, probe)
    a, b, chain, misses, pool = _wrap_chain(m, order)
    m.check(chain, misses, pool)
    _again_with_other_values(m, chain)
    m.check(chain, misses, pool)
    assert m.e.stats()["table_capacity"] == CAP
    m.close()


def _tombstone_chain(m, cap=CAP, home=HOME_MID, n_bg=1000):
    """_mid_chain, then the first 30 registered grains of the chain removed: each item twice (the first
    removes) and wrong activations (remove nothing).  30 tombstones, 10 grains behind them."""
    mid, bg, pool = _mid_chain(m, cap, home, n_bg)
    m.check(mid[MID_CHAIN], mid[MID_MISS], pool)                       # builds the probe index
    gone, kept = mid[0:30], mid[30:40]
    uk = np.concatenate([gone, gone, kept, bg[:50]])
    ua = np.concatenate([m.act_of(gone), m.act_of(gone), m.act_of(kept) ^ 1, m.act_of(bg[:50]) + 1])
    m.unregister(uk, ua)
    assert all(_t(k) not in m.part.data for k in gone) and all(_t(k) in m.part.data for k in kept)
    st = m.e.stats()
    assert st["table_tombstones"] == 30 and st["table_live"] == n_bg + 10
    return mid, bg, pool


@pytest.mark.parametrize("probe", PROBES)
def test_tombstones_inside_a_chain(gd, probe):
    """Case 3: removed grains miss, the ones behind the tombstones still hit; 20 new grains of the home
    each reuse a tombstone of the chain (found behind them: the key is not in the chain), re-projected
    into the indexes; then the one-launch removal (k_unreg_cas) of the grains at the chain's far end."""
    m = _Model(gd, probe)
    mid, bg, pool = _tombstone_chain(m)
    m.check(mid[MID_CHAIN], mid[MID_MISS], pool)
    ins = m.register(mid[MID_NEW])
    assert ins.all()
    st = m.e.stats()
    # every new grain took a tombstone of the chain: the keys do share a chain (the builder's homes are the
    # device's) and no grain was placed behind the chain instead
    assert st["table_tombstones"] == 10 and st["table_live"] == 1000 + 30 and st["table_capacity"] == CAP
    chain = np.concatenate([mid[MID_CHAIN], mid[MID_NEW]])
    m.check(chain, mid[MID_MISS], pool)
    far = mid[30:40]
    m.unregister_cas(np.concatenate([far, far[:3], mid[MID_NEW][:2]]),
                     np.concatenate([m.act_of(far), m.act_of(far[:3]), m.act_of(mid[MID_NEW][:2]) ^ 1]))
    assert all(_t(k) not in m.part.data for k in far)
    m.check(chain, mid[MID_MISS], pool)
    assert m.e.stats()["table_tombstones"] == 20
    m.close()


# ----------------------------------------------------------------------------- asynchronous batches
def _second_async_batch(m, registered, lo):
    """An ordinary asynchronous batch after the one under test: 40 new scattered grains, 60 registered."""
    m.register_async(np.concatenate([_bg(lo, lo + 40), registered[:60]]))


@pytest.mark.parametrize("probe", PROBES)
def test_async_fresh_chain(gd, probe):
    """Case 4a: 40 new grains of one home side by side in an asynchronous batch of 3,000 (otherwise
    scattered new grains, 160 of them repeated with another value: the first wins) into an empty table.
    The batch has 1 + 3 claim passes (REG_PASSES_SMALL), so the 40 must settle in them: a grain that
    loses a slot to another of the batch walks on in the same pass."""
    m = _Model(gd, probe)
    mid = _home_keys(CAP, HOME_MID, 130)
    pool = _bg(0, 3200)
    m.check(mid[MID_CHAIN], mid[MID_MISS], pool)                       # the index of an empty table
    sc = _bg(0, 2800)
    m.register_async(np.concatenate([sc[:1000], mid[MID_CHAIN], sc[1000:], sc[::17][:160]]))
    m.check(mid[MID_CHAIN], mid[MID_MISS], pool)
    _second_async_batch(m, mid[MID_CHAIN], 2800)
    m.check(mid[MID_CHAIN], mid[MID_MISS], pool)
    assert m.e.stats()["table_capacity"] == CAP
    m.close()


def _async_onto_tombstones(m, mid, bg, pool, pad, cap=CAP):
    """20 new grains of the home onto the chain's 30 tombstones, every third repeated inside the batch
    with another value (the first wins), among registered grains (reported) and scattered new ones (none
    homed within 256 slots of the chain: they would take its tombstones); padded to `pad` items with
    grains that are registered already."""
    new = mid[MID_NEW]
    sc = _bg(len(bg), len(bg) + 150)
    home = int(home_slot_np(mid[:1], cap)[0])
    sc = sc[np.abs(home_slot_np(sc, cap).astype(np.int64) - home) > 256]
    k = np.concatenate([bg[100:200], new, sc, new[::3]])
    if pad > len(k):
        k = np.concatenate([k, bg[m.rng.integers(0, len(bg), size=pad - len(k))]])
    m.register_async(k)
    st = m.e.stats()
    assert st["table_tombstones"] == 10                                # each of the 20 reused one
    chain = np.concatenate([mid[MID_CHAIN], new])
    m.check(chain, mid[MID_MISS], pool)
    _second_async_batch(m, chain, len(bg) + 150)
    m.check(chain, mid[MID_MISS], pool)


@pytest.mark.parametrize("probe", PROBES)
def test_async_onto_tombstoned_chain(gd, probe):
    """Case 4b: the batch's 20 new grains all meet the chain's first tombstone; the ones that lose it take
    the next ones in the same pass (deferred, 20 of them would need 20 passes and the batch has 4)."""
    m = _Model(gd, probe)
    mid, bg, pool = _tombstone_chain(m)
    _async_onto_tombstones(m, mid, bg, pool, 0)
    assert m.e.stats()["table_capacity"] == CAP
    m.close()


@pytest.mark.parametrize("probe", PROBES)
def test_async_onto_tombstoned_chain_large_batch(gd, probe):
    """Case 4c: the same in a batch of 70,000 items (above 65,536: REG_PASSES), in a table of 2^18 slots
    (60,000 grains, so it does not grow)."""
    cap = 1 << 18
    m = _Model(gd, probe, cap=cap)
    mid, bg, pool = _tombstone_chain(m, cap, (cap >> 1) + 264, 60_000)
    _async_onto_tombstones(m, mid, bg, pool, 70_000, cap)
    assert m.e.stats()["table_capacity"] == cap
    m.close()


# ----------------------------------------------------------------------------- upsert
@pytest.mark.parametrize("chain_kind", ["mid", "wrap"])
@pytest.mark.parametrize("probe", PROBES)
def test_upsert_on_chains(gd, probe, chain_kind):
    """Case 5: gd_dir_upsert (overwrite in batch order, GD_ACT_MULTI values) on the long and the wrapped
    chain: grains of the chain, new grains of its homes, background grains old and new, repeats."""
    m = _Model(gd, probe)
    if chain_kind == "mid":
        mid, bg, pool = _mid_chain(m)
        chain, new, misses = mid[MID_CHAIN], mid[MID_NEW3], mid[MID_MISS]
    else:
        a, b, chain, misses, pool = _wrap_chain(m, "ab")
        new = np.concatenate([a[WRAP_A_NEW], b[WRAP_B_NEW]])
        bg = pool[:1000]
    m.check(chain, misses, pool)
    k = np.concatenate([chain, bg[:200], new, pool[1000:1100], chain[::2], new[::3], bg[100:150]])
    k = np.ascontiguousarray(k[m.rng.permutation(len(k))])
    acts = m.acts(len(k))
    acts[m.rng.random(len(k)) < 0.3] = gd.GD_ACT_MULTI
    m.upsert(k, acts, m.rng.integers(0, 8, size=len(k)).astype(np.uint32))
    full = np.concatenate([chain, new])
    want = o.route_batch_np(full, m.spec, m.directory())
    assert (want[0] == o.ST_MULTI_ACT).sum() >= 5 and (want[0] == o.ST_OK).sum() >= 5
    q = np.concatenate([full, misses, pool[m.rng.integers(0, len(pool), size=2000)]])
    want = o.route_batch_np(q, m.spec, m.directory())
    for got in (m.e.route(q), m.e.route_bucket(q, N_ACT)[:3]):
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
    m.check_live()
    assert m.e.stats()["table_capacity"] == CAP
    m.close()


# ----------------------------------------------------------------------------- high load
@pytest.mark.parametrize("probe", PROBES)
def test_high_load_churn(gd, probe):
    """Case 6: 2,400 scattered grains of two classes in 4,096 slots (load 0.59, with the tombstones up to
    0.7: long chains everywhere, many across group boundaries), then 6 rounds that remove 100 and register
    100 new ones, a synchronous and an asynchronous round in turn; routes against the oracle after every
    round.  The table must not grow: maybe_grow_table rehashes when live + tombstones + incoming exceeds
    3/4 of the capacity, 3,072.  Round 6 registers into 2,300 live grains and at most 500 tombstones (if no
    new grain ever reused one): 2,300 + 500 + 100 = 2,900, whatever the order of the claims.  (2,600 grains
    and 200 a round reach 3,120 in round 4 in a sequential model of the table, and the table grows.)"""
    m = _Model(gd, probe)
    both = lambda lo, hi: np.concatenate([_bg(lo, hi), _bg(lo, hi, TC2)])          # noqa: E731
    m.register(both(0, 1200))
    nxt = 1200
    misses = _home_keys(CAP, HOME_MID, 130)[MID_MISS]
    for rnd in range(6):
        live = np.array(list(m.part.data.keys()), np.uint64).reshape(-1, 3)
        pick = m.rng.permutation(len(live))
        gone, wrong = live[pick[:100]], live[pick[100:150]]
        uk = np.concatenate([gone, gone, wrong])
        ua = np.concatenate([m.act_of(gone), m.act_of(gone), m.act_of(wrong) ^ 1])
        new = both(nxt, nxt + 50)
        nxt += 50
        if rnd % 2 == 0:
            m.unregister(uk, ua)
            assert m.register(new).all()
        else:
            m.unregister_cas(uk, ua)
            m.register_async(new)
        live = np.array(list(m.part.data.keys()), np.uint64).reshape(-1, 3)
        m.check(live[m.rng.integers(0, len(live), size=500)], misses, np.concatenate([gone, both(nxt, nxt + 200)]))
        st = m.e.stats()
        assert st["table_capacity"] == CAP and st["table_live"] == 2400, (rnd, st)
    m.close()


# ----------------------------------------------------------------------------- asynchronous errors
def _bad_async_batch(m):
    """An asynchronous registration whose device values carry one silo index 0xFFFF (device error bit 4:
    the one device error a caller can produce with valid keys)."""
    import torch
    dev = torch.device("cuda:0")
    k = np.ascontiguousarray(_bg(5000, 5064))
    v = np.stack([m.acts(64), m.owner(k)], 1).astype(np.uint32)
    v[17, 1] = 0xFFFF
    dk = torch.from_numpy(k.view(np.int64)).to(dev)
    dv = torch.from_numpy(v.view(np.int32)).to(dev)
    m.e.register_device_async(dk.data_ptr(), dv.data_ptr(), 64)
    return dk, dv


@pytest.mark.parametrize("probe", PROBES)
def test_async_error_reported_once_by_stats(gd, probe):
    """gd_stats_get is a synchronising call: it reports the asynchronous batch's error, once."""
    m = _Model(gd, probe)
    mid, bg, pool = _mid_chain(m)
    keep = _bad_async_batch(m)
    with pytest.raises(gd.GrainDispatchError) as ei:
        m.e.stats()
    assert ei.value.code == gd.GD_EINVAL
    st = m.e.stats()                                                   # reported once: clean now
    assert m.e.stats() == st
    m.e.synchronize()
    good = np.concatenate([_bg(5000, 5017), _bg(5018, 5064)])          # the batch's other grains are registered
    assert m.e.lookup(good)[2].all()
    st2, _, act = m.e.route(mid[MID_CHAIN])                            # and the directory still routes
    assert (st2 == o.ST_OK).all() and np.array_equal(act, m.act_of(mid[MID_CHAIN]))
    del keep
    m.close()


@pytest.mark.parametrize("probe", PROBES)
def test_async_error_does_not_poison_the_next_registration(gd, probe):
    """A synchronous registration after the bad asynchronous batch reports that batch's error first and
    does no work (nothing of its own batch is registered, nothing half claimed); repeated, it registers
    all of its 40 same-home grains."""
    m = _Model(gd, probe)
    bg = _bg(0, 1000)
    m.register(bg)
    mid = _home_keys(CAP, HOME_MID, 130)
    keep = _bad_async_batch(m)
    chain = mid[MID_CHAIN]
    acts, silos = m.acts(40), m.owner(chain)
    with pytest.raises(gd.GrainDispatchError) as ei:
        m.e.register(chain, acts, silos)
    assert ei.value.code == gd.GD_EINVAL
    st = m.e.stats()                                                   # the error was reported once
    live = st["table_live"]                                            # (whether the bad item left an entry is open)
    assert live in (1000 + 63, 1000 + 64) and st["table_tombstones"] == 0
    assert not m.e.lookup(chain)[2].any()
    st, _, act = m.e.route(chain)
    assert (st == o.ST_MISS).all() and (act == o.M32).all()
    ins = m.register(chain, acts, silos)                               # the same call again
    assert ins.all()
    assert m.e.stats()["table_live"] == live + 40
    la, ls, lf = m.e.lookup(chain)
    assert lf.all() and np.array_equal(la, acts) and np.array_equal(ls, silos)
    good = np.concatenate([_bg(5000, 5017), _bg(5018, 5064)])          # the bad batch's other grains are live
    assert m.e.lookup(good)[2].all()
    del keep
    m.close()
