"""The direct N1-indexed table (gd_probe.h CxdArgs, eng_route.hip cxd_prepare): while the 8-B probe index is
pure -- one grain class, N0 = 0, N1 < 2^32, every live entry held -- and the N1s are dense, k_route reads
direct[N1] instead of probing.  The table is built (k_cxd_build) only after one whole route found the
directory unchanged, is tied to a snapshot of the directory and never read stale.

Every route here is compared bit for bit (status, silo, act) with the oracle and with a second engine that
probes the directory table itself (GD_OPT_PROBE 0).  Parity alone would pass with the form never taken, so
every case also counts the k_cxd_build launches in the per-kernel timing table: exactly one more where a
build is expected, none where it is not."""
import numpy as np
import pytest

import oracle as o

pytestmark = pytest.mark.gpu

TC = o.grain_type_code(o.PING_GRAIN_CLASS)
TCD = o.type_code_data(o.CAT_GRAIN, TC)
CAP = 1 << 14                     # 8-B index 128 KiB: the table may take up to 64 KiB, d <= 16,384


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


def _pair(gd, mode="D", cap=CAP, **opts):
    """(engine under test: the 8-B index, per-kernel timing on; engine probing the directory table)."""
    silos = o.bench_silos(8)
    out = []
    for probe in (4, 0):
        e = gd.GrainDispatch(device=0, table_capacity=cap, options=dict(opts, probe=probe))
        e.ring_set_silos(mode, [(s.ip, s.port, s.gen) for s in silos])
        out.append(e)
    out[0].set_kernel_timing(True)
    return out, o.ring_spec(silos, mode)


def _owner(spec, k):
    return o.ring_owner_np(spec, o.jenkins_u64x3_np(k[:, 2], k[:, 0], k[:, 1])).astype(np.uint32)


def _builds(e):
    return e.kernel_times().get("k_cxd_build", (0, 0.0))[0]


def _expect(q, spec, d, invalid=()):
    """Oracle routes; `invalid`: silos IsValidSilo filters (the entry gives a miss at its ring owner)."""
    st, silo, act, owner, _ = o.route_batch_np(q, spec, d)
    bad = (st == o.ST_OK) & np.isin(silo, np.array(list(invalid), np.uint32))
    st, silo, act = st.copy(), silo.copy(), act.copy()
    st[bad] = o.ST_MISS
    silo[bad] = owner[bad]
    act[bad] = o.M32
    return st, silo, act


def _check(a, b, q, spec, d, invalid=()):
    want = _expect(q, spec, d, invalid)
    for e in (a, b):
        got = e.route(q)
        for x, y in zip(got, want):
            np.testing.assert_array_equal(x, y)


def _settle(a, b, q, spec, d, builds, invalid=()):
    """After a read-back (stats) with no batch since: one route finds the directory quiet and runs without
    the table, the next builds it once, later ones reuse it; all exact."""
    a.stats()
    _check(a, b, q, spec, d, invalid)
    assert _builds(a) == builds
    _check(a, b, q, spec, d, invalid)
    assert _builds(a) == builds + 1
    _check(a, b, q, spec, d, invalid)
    assert _builds(a) == builds + 1
    return builds + 1


def _close(*es):
    for e in es:
        e.close()


@pytest.mark.parametrize("mode", ["D", "R", "V"])
def test_dense_keys(gd, mode):
    """Keys 0..G-1: the first route after registration runs without the table, the second builds it, every
    route gives the same result; n is no multiple of the workgroup size, and one batch is a single message."""
    rng = np.random.default_rng(5)
    (a, b), spec = _pair(gd, mode)
    G = 6000
    reg = o.grain_keys(TC, np.arange(G))
    acts, own = (np.arange(G, dtype=np.uint32) * 3 + 1), _owner(spec, o.grain_keys(TC, np.arange(G)))
    for e in (a, b):
        e.register(reg, acts, own)
    d = o.DirectoryArrays(reg, acts, own)
    q = o.grain_keys(TC, rng.integers(0, G + 200, size=20001))
    _check(a, b, q, spec, d)
    assert _builds(a) == 0                                   # quiescence rule: no table yet
    _check(a, b, q, spec, d)
    assert _builds(a) == 1
    _check(a, b, q, spec, d)
    _check(a, b, q[7:8], spec, d)                            # n = 1
    _check(a, b, o.grain_keys(TC, np.array([G])), spec, d)   # n = 1, a miss
    assert _builds(a) == 1
    _close(a, b)


def test_mixed_batch_multi_activation_and_invalid_silo(gd):
    """One launch with every kind of lane: registered keys, unregistered keys below d (empty word), N1 =
    d - 1, d, d + 1, N1 >= 2^32, N0 != 0, a second class, system-target, membership and KeyExt-category
    keys.  Then grains upserted to several activations (GD_ROUTE_MULTI_ACT, at the ring owner), and a silo
    invalidated after the build with no table change: a miss through IsValidSilo at route time, no rebuild."""
    rng = np.random.default_rng(6)
    (a, b), spec = _pair(gd)
    G = 5000
    ids = np.array([i for i in range(G) if i % 7 != 3 or i == G - 1])
    reg = o.grain_keys(TC, ids)
    acts, own = (ids * 2 + 5).astype(np.uint32), _owner(spec, reg)
    for e in (a, b):
        e.register(reg, acts, own)
    D = (G + 15) // 16 * 16                                  # largest live N1 = G - 1
    q = o.grain_keys(TC, rng.integers(0, G, size=50003))     # registered and unregistered, all below d
    q[0:3] = o.grain_keys(TC, np.array([D - 1, D, D + 1]))
    q[3:6] = o.grain_keys(TC, np.array([G - 1, 0, 3]))       # the last entry, the first, an empty word
    q[10::97, 1] += np.uint64(1 << 32)                       # N1 past 2^32 (low word a live entry's)
    q[11::89, 0] = 5                                         # N0 != 0
    q[12::83, 2] = np.uint64(o.type_code_data(o.CAT_GRAIN, 0x777))
    q[13::101] = np.array(o.UniqueKey(0, 7, o.type_code_data(o.CAT_SYSTEM_TARGET, 1)).as_tuple(), dtype=np.uint64)
    q[14::103] = np.array(o.MEMBERSHIP_TABLE_ID.as_tuple(), dtype=np.uint64)
    q[15::107, 2] = np.uint64(o.type_code_data(o.CAT_KEYEXT_GRAIN, TC))
    d = o.DirectoryArrays(reg, acts, own)
    _check(a, b, q, spec, d)
    assert _builds(a) == 0
    _check(a, b, q, spec, d)
    assert _builds(a) == 1
    want = _expect(q, spec, d)
    assert {o.ST_OK, o.ST_MISS, o.ST_SYSTEM_TARGET, o.ST_MEMBERSHIP, o.ST_KEYEXT} <= set(want[0].tolist())
    # several activations
    up = rng.choice(len(ids), size=300, replace=False)
    acts2 = acts.copy()
    acts2[up] = o.ACT_MULTI
    for e in (a, b):
        e.upsert(reg[up], acts2[up], own[up])
    d2 = o.DirectoryArrays(reg, acts2, own)
    _check(a, b, q, spec, d2)                                # at once: the batch itself set the table aside
    assert _builds(a) == 1
    n = _settle(a, b, q, spec, d2, 1)
    assert (_expect(q, spec, d2)[0] == o.ST_MULTI_ACT).sum() > 100
    # IsValidSilo: no table change, no rebuild
    for e in (a, b):
        e.set_valid_silos([s for s in range(8) if s != 3], 8)
    _check(a, b, q, spec, d2, invalid=(3,))
    _check(a, b, q, spec, d2, invalid=(3,))
    assert _builds(a) == n
    assert ((want[0] == o.ST_OK) & (want[1] == 3)).sum() > 100
    _close(a, b)


def test_stale_table_is_never_read(gd):
    """With the table built: removals, new grains (one beyond d) and, later, a Guid grain registered
    asynchronously are all reflected by the very next route; after quiescence the table is rebuilt once
    (never while the Guid grain keeps the index impure); the same after gd_dir_clear and re-registration,
    and after gd_dir_rehash."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    (a, b), spec = _pair(gd)
    G = 6000
    reg = o.grain_keys(TC, np.arange(G))
    acts, own = np.arange(G, dtype=np.uint32) + 9, _owner(spec, reg)
    live = {tuple(k): (int(x), int(s)) for k, x, s in zip(reg.tolist(), acts, own)}

    def snap():
        keys = np.array(list(live.keys()), np.uint64).reshape(-1, 3)
        vals = np.array(list(live.values()), np.uint32).reshape(-1, 2)
        return o.DirectoryArrays(keys, vals[:, 0], vals[:, 1])

    for e in (a, b):
        e.register(reg, acts, own)
    q = o.grain_keys(TC, np.concatenate([rng.integers(0, G + 400, size=30000), [9000, 8999, 9001]]))
    _check(a, b, q, spec, snap())
    _check(a, b, q, spec, snap())
    assert _builds(a) == 1
    # removals and new grains, one of them beyond d
    gone = np.arange(0, G, 5)
    new = o.grain_keys(TC, np.array([G + 1, G + 17, G + 300, 9000]))
    nacts, nown = np.array([1, 2, 3, 4], np.uint32), _owner(spec, new)   # within the index's activation bits
    for e in (a, b):
        e.unregister(reg[gone], acts[gone])
        e.register(new, nacts, nown)
    for k in reg[gone].tolist():
        del live[tuple(k)]
    for k, x, s in zip(new.tolist(), nacts, nown):
        live[tuple(k)] = (int(x), int(s))
    _check(a, b, q, spec, snap())                            # immediately
    assert _builds(a) == 1
    n = _settle(a, b, q, spec, snap(), 1)
    # a Guid grain, asynchronously, right before a route
    guid = o.grain_keys(TC, np.array([123]))
    guid[:, 0] = 0x1234567890
    gv = np.stack([np.array([5], np.uint32), _owner(spec, guid)], 1)
    dk = torch.from_numpy(guid.view(np.int64)).to(dev)
    dv = torch.from_numpy(gv.view(np.int32)).to(dev)
    for e in (a, b):
        e.register_device_async(dk.data_ptr(), dv.data_ptr(), 1)
    live[tuple(guid[0].tolist())] = (5, int(gv[0, 1]))
    qg = np.concatenate([q, guid])
    _check(a, b, qg, spec, snap())                           # no read-back since the batch
    a.stats()
    for _ in range(3):                                       # impure: the table stays aside
        _check(a, b, qg, spec, snap())
    assert _builds(a) == n
    # clear and register again; then rehash
    d0 = o.DirectoryArrays(reg, acts, own)
    # (the first route after either rebuilds the 8-B index, finds it pure and quiet: the next one builds)
    for change in (lambda e: (e.clear(), e.register(reg, acts, own)), lambda e: e.rehash(1 << 15)):
        for e in (a, b):
            change(e)
        _check(a, b, qg, spec, d0)                           # immediately: the Guid grain and 9000 are gone
        assert _builds(a) == n
        _check(a, b, qg, spec, d0)
        assert _builds(a) == n + 1
        _check(a, b, qg, spec, d0)
        assert _builds(a) == n + 1
        n += 1
    _close(a, b)


@pytest.mark.parametrize("case", ["sparse", "two_classes", "big_n1"])
def test_ineligible_directories(gd, case):
    """Sparse keys (the table would outweigh half the 8-B index), two grain classes, one N1 >= 2^32: no
    k_cxd_build launch however quiet the directory, and the same routes."""
    rng = np.random.default_rng(8)
    (a, b), spec = _pair(gd)
    G = 4096
    ids = np.arange(G) * (1000 if case == "sparse" else 1)
    reg = o.grain_keys(TC, ids)
    if case == "two_classes":
        reg = np.concatenate([reg, o.grain_keys(o.grain_type_code("UnitTests.OtherGrain"), np.arange(64))])
    if case == "big_n1":
        reg = np.concatenate([reg, o.grain_keys(TC, np.array([(1 << 32) + 11]))])
    acts, own = np.arange(len(reg), dtype=np.uint32) + 2, _owner(spec, reg)
    for e in (a, b):
        e.register(reg, acts, own)
    d = o.DirectoryArrays(reg, acts, own)
    q = np.concatenate([reg, o.grain_keys(TC, np.arange(G, G + 300))])[rng.integers(0, len(reg) + 300, size=20011)]
    for _ in range(2):
        a.stats()
        for _ in range(3):
            _check(a, b, q, spec, d)
    assert _builds(a) == 0
    _close(a, b)


@pytest.mark.parametrize("wire", [2, 1])
def test_n1_stream_form(gd, wire):
    """Kind 1: a world-1 exchange delivers a one-class batch as N1s alone (GD_OPT_WIRE_HEADERS 2: u32, 1:
    u64) and route_n1_device probes them as received; same directory, same table, same results."""
    rng = np.random.default_rng(9)
    (a, b), spec = _pair(gd, wire_headers=wire, region_probe=0)
    G = 6000
    reg = o.grain_keys(TC, np.arange(G))
    acts, own = np.arange(G, dtype=np.uint32), _owner(spec, reg)
    for e in (a, b):
        e.register(reg, acts, own)
        gd.GrainDispatch.comm_init_local([e])
    d = o.DirectoryArrays(reg, acts, own)
    D = (G + 15) // 16 * 16
    n1 = np.concatenate([rng.integers(0, G + 8, size=40013), [D - 1, D, D + 1, G - 1]])
    if wire == 1:
        n1 = np.concatenate([n1, [(1 << 32) + 5, (1 << 40)]])     # forces u64 headers; low word a live entry's
    q = o.grain_keys(TC, n1)
    for step in range(3):
        for e in (a, b):
            res = e.route_multi(q, G, no_keys=True)
            st, silo, act = _expect(q[res["recv_idx"]], spec, d)
            np.testing.assert_array_equal(res["status"], st)
            np.testing.assert_array_equal(res["silo"], silo)
            np.testing.assert_array_equal(res["act"], act)
        assert _builds(a) == (0 if step == 0 else 1)
    for e in (a, b):
        e.comm_destroy()
    _close(a, b)
