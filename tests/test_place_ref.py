"""CPU tests of the placement rule's restatement (_place_ref.py): the literal loop and the numpy form
agree, one hand-written message per branch, the HASH order through gd_silo_compare, and the argument
paths of the gd_place_* / gd_route_place* entry points that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import _place_ref as P
import oracle as o
from dirstate import DirectoryState
from orleans_amd import graindispatch as g

TC = o.grain_type_code(o.PING_GRAIN_CLASS)
MY, SEED = 2, 6


def _world(rng, n_silos=8, compatible=None, local_active=True, n_grains=500):
    silos = o.bench_silos(n_silos)
    spec = o.ring_spec(silos, "D")
    cfg = P.PlaceConfig(silos, compatible, local_active, my_silo=MY)
    d = DirectoryState()
    reg = o.grain_keys(TC, np.arange(n_grains))
    acts = np.arange(n_grains, dtype=np.uint32)
    acts[::17] = o.ACT_MULTI
    d.upsert(reg, acts, rng.integers(0, n_silos, size=n_grains))
    return silos, spec, cfg, d


def _clone(d):
    c = DirectoryState()
    c.entries = {k: list(v) for k, v in d.entries.items()}
    c.op, c.n_valid, c.valid = d.op, d.n_valid, set(d.valid)
    return c


def _both(keys, spec, cfg, d, strategy, given, act_base=1000):
    route = P.route_of(keys, spec, d, MY, SEED)
    d1, d2 = _clone(d), _clone(d)
    a = P.place_loop(keys, route, strategy, given, act_base, cfg, d1)
    b = P.place_np(keys, route, strategy, given, act_base, cfg, d2)
    for name, x, y in zip(("status", "silo", "act", "placed", "new_idx"), a, b):
        assert x.dtype == y.dtype, name
        np.testing.assert_array_equal(x, y, err_msg=name)
    assert a[5] == b[5]
    assert d1.entries == d2.entries and d1.op == d2.op
    return a, d1, route


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("strategy", [P.PLACE_NONE, P.PLACE_HASH, P.PLACE_LOCAL, P.PLACE_GIVEN, "mixed"])
def test_loop_equals_numpy(seed, strategy):
    """A few thousand messages with duplicate new grains, client / KeyExt / system targets, given silos that are
    out of range, incompatible or invalid; LOCAL with the local silo active (seed 1, 3) and not (seed 2)."""
    rng = np.random.default_rng(seed * 101 + (9 if strategy == "mixed" else strategy))
    n = 3000 + seed * 517
    compatible = np.ones(8, bool)
    compatible[[1, 5]] = False
    silos, spec, cfg, d = _world(rng, compatible=compatible, local_active=seed != 2)
    d.set_valid([0, 1, 2, 4, 6], 7)                           # silos 3 and 5 invalid, silo 7 past the range: valid
    keys = P.mixed_keys(rng, n, TC, 500)
    given = rng.integers(0, 10, size=n).astype(np.uint32)     # 8, 9: out of range; 1, 5: incompatible
    given[rng.random(n) < 0.02] = P.NO_SILO
    strat = rng.integers(0, 5, size=n).astype(np.uint8) if strategy == "mixed" else strategy   # 4: no known value
    (st, silo, act, placed, new_idx, c), d1, route = _both(keys, spec, cfg, d, strat, given)
    if strategy == P.PLACE_NONE:
        assert c == 0 and len(new_idx) == 0 and d1.entries == d.entries
        np.testing.assert_array_equal(st, route[0])
        return
    local_all = strategy == P.PLACE_LOCAL and seed != 2       # every candidate lands on the local silo
    assert set(np.unique(placed).tolist()) == ({0, 1, 2} if local_all else {0, 1, 2, 3})
    assert c == int(((placed == P.PLACED_NEW) | (placed == P.PLACED_JOINED)).sum()) > len(new_idx) > 0
    untouched = placed == P.PLACED_NONE
    for got, want in zip((st, silo, act), route):
        np.testing.assert_array_equal(got[untouched], want[untouched])
    assert (st[placed == P.PLACED_SKIPPED] == o.ST_MISS).all()
    # sparse numbers: act_base + the rank of the grain's first placing message among the placing candidates
    rank = np.cumsum((placed == P.PLACED_NEW) | (placed == P.PLACED_JOINED)) - 1
    np.testing.assert_array_equal(act[new_idx], 1000 + rank[new_idx])
    assert (np.diff(new_idx.astype(np.int64)) > 0).all()


def _one(key, strategy, given=None, compatible=None, local_active=True, valid=None):
    rng = np.random.default_rng(0)
    silos, spec, cfg, d = _world(rng, compatible=compatible, local_active=local_active, n_grains=20)
    if valid is not None:
        d.set_valid(valid, 8)
    keys = np.array([key], dtype=np.uint64)
    gv = None if given is None else np.array([given], np.uint32)
    (st, silo, act, placed, new_idx, c), d1, route = _both(keys, spec, cfg, d, strategy, gv, act_base=77)
    return int(st[0]), int(silo[0]), int(act[0]), int(placed[0]), new_idx.tolist(), c, route, cfg, d1


NEW = (0, 123456, o.type_code_data(o.CAT_GRAIN, TC))


def test_one_message_per_branch():
    h = o.jenkins_u64x3(NEW[2], NEW[0], NEW[1]) & 0x7FFFFFFF
    # NONE: stays MISS with the ring owner, nothing registered
    st, silo, act, placed, new, c, route, cfg, d1 = _one(NEW, P.PLACE_NONE)
    assert (st, silo, act, placed, new, c) == (o.ST_MISS, int(route[1][0]), 0xFFFFFFFF, P.PLACED_SKIPPED, [], 0)
    assert NEW not in d1.entries
    # HASH over all 8 and over a compatible subset
    st, silo, act, placed, new, c, route, cfg, d1 = _one(NEW, P.PLACE_HASH)
    assert (st, silo, act, placed, new, c) == (o.ST_OK, cfg.sorted[h % 8], 77, P.PLACED_NEW, [0], 1)
    assert d1.entries[NEW][:2] == [77, silo]
    comp = [0, 1, 1, 0, 1, 0, 0, 0]
    st, silo, act, placed, new, c, route, cfg, d1 = _one(NEW, P.PLACE_HASH, compatible=comp)
    assert cfg.sorted == [1, 2, 4] and (st, silo, placed) == (o.ST_OK, [1, 2, 4][h % 3], P.PLACED_NEW)
    # LOCAL: active and compatible; inactive with and without a given silo; local not compatible
    assert _one(NEW, P.PLACE_LOCAL)[:4] == (o.ST_OK, MY, 77, P.PLACED_NEW)
    assert _one(NEW, P.PLACE_LOCAL, given=4, local_active=False)[:4] == (o.ST_OK, 4, 77, P.PLACED_NEW)
    assert _one(NEW, P.PLACE_LOCAL, local_active=False)[3] == P.PLACED_SKIPPED
    assert _one(NEW, P.PLACE_LOCAL, given=1, compatible=[1, 1, 0, 1, 1, 1, 1, 1])[:4] == (o.ST_OK, 1, 77, P.PLACED_NEW)
    # GIVEN: applied; out of range; incompatible; invalid; no given array
    assert _one(NEW, P.PLACE_GIVEN, given=5)[:4] == (o.ST_OK, 5, 77, P.PLACED_NEW)
    for kw in (dict(given=8), dict(given=P.NO_SILO), dict(given=3, compatible=[1, 1, 1, 0, 1, 1, 1, 1]),
               dict(given=3, valid=[0, 1, 2, 4, 5, 6, 7]), dict()):
        r = _one(NEW, P.PLACE_GIVEN, **kw)
        assert (r[0], r[2], r[3], r[4], r[5]) == (o.ST_MISS, 0xFFFFFFFF, P.PLACED_SKIPPED, [], 0), kw
        assert NEW not in r[8].entries
    # an empty compatible set skips every strategy
    for s in (P.PLACE_HASH, P.PLACE_LOCAL, P.PLACE_GIVEN):
        assert _one(NEW, s, given=1, compatible=[0] * 8)[3] == P.PLACED_SKIPPED
    # not a candidate: a client, a KeyExt grain, a system target, the membership grain, a hit, a multi-activation grain
    mt = o.MEMBERSHIP_TABLE_ID
    for key, want in (((7, 11, o.type_code_data(o.CAT_CLIENT, 0)), o.ST_MISS),
                      ((0, 5, o.type_code_data(o.CAT_KEYEXT_GRAIN, TC)), o.ST_KEYEXT),
                      ((0, 9, o.type_code_data(o.CAT_SYSTEM_TARGET, 12)), o.ST_SYSTEM_TARGET),
                      ((mt.n0, mt.n1, mt.tcd), o.ST_MEMBERSHIP),
                      (tuple(int(x) for x in o.grain_keys(TC, [3])[0]), o.ST_OK),
                      (tuple(int(x) for x in o.grain_keys(TC, [17])[0]), o.ST_MULTI_ACT)):
        st, silo, act, placed, new, c, route, cfg, d1 = _one(key, P.PLACE_HASH)
        assert (st, placed, new, c) == (want, P.PLACED_NONE, [], 0)
        assert (silo, act) == (int(route[1][0]), int(route[2][0]))


def test_batch_order_first_wins_and_skipped_first_message():
    rng = np.random.default_rng(5)
    silos, spec, cfg, d = _world(rng, n_grains=20)
    a, b = o.grain_keys(TC, [900])[0], o.grain_keys(TC, [901])[0]
    keys = np.array([a, b, a, a, b], dtype=np.uint64)
    strat = np.array([P.PLACE_NONE, P.PLACE_GIVEN, P.PLACE_GIVEN, P.PLACE_GIVEN, P.PLACE_HASH], np.uint8)
    given = np.array([1, 3, 4, 5, 6], np.uint32)
    (st, silo, act, placed, new_idx, c), d1, _ = _both(keys, spec, cfg, d, strat, given, act_base=10)
    assert placed.tolist() == [P.PLACED_SKIPPED, P.PLACED_NEW, P.PLACED_NEW, P.PLACED_JOINED, P.PLACED_JOINED]
    assert st.tolist() == [o.ST_MISS, 0, 0, 0, 0]             # the skipped message stays MISS though a later one places
    assert act[1:].tolist() == [10, 11, 11, 10] and silo[1:].tolist() == [3, 4, 4, 3]
    assert new_idx.tolist() == [1, 2] and c == 4              # numbers 12 and 13 were proposed and stay unused


SILO_SETS = {
    "address": [o.Silo(f"10.0.{i % 3}.{250 - i}", 11111, 1) for i in range(9)],
    "port": [o.Silo("10.0.0.1", 30000 - 7 * i, 1) for i in range(7)],
    "generation": [o.Silo("10.0.0.1", 11111, 50 - i) for i in range(6)],
    "mixed": [o.Silo(f"10.1.{i % 4}.{i % 5 + 1}", 11111 + i % 3, 1 + (i * 7) % 4) for i in range(40)],
    "ipv6": [o.Silo(ip, 11111 + i % 2, 1 + i % 3) for i, ip in enumerate(
        ["fe80::2", "fe80::1", "2001:db8::ff", "10.0.0.9", "2001:db8::1", "10.0.0.1", "::1"])],
}


@pytest.mark.parametrize("name", sorted(SILO_SETS))
def test_hash_order_through_gd_silo_compare(name):
    silos = SILO_SETS[name]
    addrs = [g.silo_addr(s.ip, s.port, s.gen) for s in silos]
    lib_cmp = lambda a, b: g.lib.gd_silo_compare(C.byref(addrs[silos.index(a)]), C.byref(addrs[silos.index(b)]))
    compatible = [i % 5 != 3 for i in range(len(silos))]
    by_lib = P.PlaceConfig(silos, compatible, compare=lib_cmp)
    by_oracle = P.PlaceConfig(silos, compatible)
    assert by_lib.sorted == by_oracle.sorted
    assert by_lib.sorted != sorted(by_lib.sorted)             # the order is not the index order


def test_abi_argument_paths_without_a_gpu():
    lib = g.lib
    arr = (g.gd_silo_addr * 2)(g.silo_addr("10.0.0.1", 1, 1), g.silo_addr("10.0.0.2", 1, 1))
    assert lib.gd_place_configure(None, arr, 2, None, 1) == g.GD_EINVAL
    assert b"null" in lib.gd_last_error(None)
    assert lib.gd_place_configure(None, arr, 0, None, 1) == g.GD_EINVAL
    assert lib.gd_place_configure(None, arr, 0xFFFF, None, 1) == g.GD_EINVAL
    nn, npr = C.c_uint32(9), C.c_uint32(9)
    head = (None, None, 0, None, g.PLACE_HASH, None, 0, None, None, None, None, None, C.byref(nn), C.byref(npr))
    assert lib.gd_route_place_device(*head) == g.GD_ESTATE
    assert b"gd_place_configure" in lib.gd_last_error(None)
    assert lib.gd_route_place(*head) == g.GD_ESTATE
    assert lib.gd_route_place_bucket_device(*head, 4, None, None) == g.GD_ESTATE
    assert lib.gd_route_place_bucket(*head, 4, None, None) == g.GD_ESTATE
    bad = head[:4] + (4,) + head[5:]                          # the argument check comes before the state check
    assert lib.gd_route_place_device(*bad) == g.GD_EINVAL
    assert lib.gd_route_place_bucket(*bad, 4, None, None) == g.GD_EINVAL
    assert (g.PLACE_NONE, g.PLACE_HASH, g.PLACE_LOCAL, g.PLACE_GIVEN) == (0, 1, 2, 3)
    assert (g.PLACED_NONE, g.PLACED_NEW, g.PLACED_JOINED, g.PLACED_SKIPPED) == (0, 1, 2, 3)
