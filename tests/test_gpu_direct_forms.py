"""The direct-table route (gd_route.h k_route_d, eng_route.hip cxd_prepare) in the launch forms, the
n1_max writers and the entry points test_gpu_direct.py does not reach:

  * k_route_d<MODE, 2, false, 0>, two messages a thread, which route_mode takes once the 8-B index is over
    ROUTE_NT_INDEX_BYTES (capacity 2^24), and route_n1_device's k_route_d<MODE, 1, false, 4 | 8>;
  * xcd_tile's edges: grids of 1 to 17 workgroups (nb & 7 and nb >> 3 both vary), n at k * 256 / k * 512 +- 1,
    the edge lanes in the ragged tail and in a thread's second message;
  * every writer of CxCounters::n1_max (k_cx_types on a full build, k_cx_sync for gd_dir_upsert,
    k_reg_commit_elect_cx for the registrations), each with grains at and beyond the table's size d, and the
    untracked writers (merge, split, silo removal) that rebuild through tab_gen;
  * the eligibility edge dd * 4 = capacity * 8 / 2, a built table turning ineligible, the way back by rehash;
  * route_bucket, the pipelined route_bucket_device, route_frames and micro-batches with the table built.

As in test_gpu_direct.py every route is compared bit for bit (status, silo, act) with the oracle and with a
second engine that probes the directory table itself (GD_OPT_PROBE 0), and every case counts the k_cxd_build
launches: parity alone passes with the form never taken.

The last four cases pin the other launch forms of the route (GD_OPT_PROBE 0 / 2 / 3 / 4) that no other test
reaches with a pinned option: the 24-B route's two messages a thread over a 2^24-slot table, the N1 routes over
the 16-B index, the region-mapped routes at every key width and the two k_route_bound forms; n at one
workgroup's share and one to either side, and n = 1.

Not covered: the d <= 2^30 cap of cxd_prepare (it needs a 32 GB directory), and the linear workgroup order
(gd_handle::route_xcd off): no handle option exposes it, so every grid here runs xcd_tile with xcd = 1."""
import numpy as np
import pytest

import dirstate as ds
import oracle as o
from test_gpu_direct import CAP, TC, _builds, _check, _expect, _owner, _pair, _settle

pytestmark = pytest.mark.gpu

BIG = 1 << 24                        # the smallest capacity whose 8-B index is over ROUTE_NT_INDEX_BYTES
ROUTE_NT_INDEX_BYTES = 64 << 20      # eng_route.hip, above route_form: route_mode's M = 2 / temporal threshold
SILOS = o.bench_silos(8)
OTHER_TCD = o.type_code_data(o.CAT_GRAIN, 0x777)


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


def _engine(gd, mode, cap, probe, **opts):
    e = gd.GrainDispatch(device=0, table_capacity=cap, options=dict(opts, probe=probe))
    e.ring_set_silos(mode, [(s.ip, s.port, s.gen) for s in SILOS])
    return e


@pytest.fixture(scope="module")
def big(gd):
    """One 2^24-slot engine for the module (about 0.9 GB with its indexes); the cases clear it, install their
    ring and register again.  A world-1 communicator for the N1-stream case (plain routes never look at it)."""
    e = _engine(gd, "D", BIG, 4, region_probe=0)
    e.set_kernel_timing(True)
    gd.GrainDispatch.comm_init_local([e])
    assert e.stats()["table_capacity"] * 8 > ROUTE_NT_INDEX_BYTES
    yield e
    e.comm_destroy()
    e.close()


def _reset(e, mode):
    e.clear()
    e.ring_set_silos(mode, [(s.ip, s.port, s.gen) for s in SILOS])
    return o.ring_spec(SILOS, mode)


def _d_of(n1_max):
    """cxd_prepare's table size for the largest live N1."""
    return (n1_max + 1 + 15) // 16 * 16


def _sparse_ids(G):
    """0..G-1 with one in seven left out (empty table words); G - 1 stays."""
    return np.array([i for i in range(G) if i % 7 != 3 or i == G - 1])


def _edge_keys(D, live):
    """N1 = d - 1, d, d + 1; N0 != 0; another class; N1 >= 2^32 (low word a live entry's); a system target;
    the membership grain; the KeyExt category."""
    k = o.grain_keys(TC, np.array([D - 1, D, D + 1, live, live, live, 0, 0, live]))
    k[3, 0] = 5
    k[4, 2] = np.uint64(OTHER_TCD)
    k[5, 1] += np.uint64(1 << 32)
    k[6] = np.array(o.UniqueKey(0, 7, o.type_code_data(o.CAT_SYSTEM_TARGET, 1)).as_tuple(), dtype=np.uint64)
    k[7] = np.array(o.MEMBERSHIP_TABLE_ID.as_tuple(), dtype=np.uint64)
    k[8, 2] = np.uint64(o.type_code_data(o.CAT_KEYEXT_GRAIN, TC))
    return k


def _batch(rng, n, hi, D, live):
    """n keys drawn from 0..hi; above 64 messages the edge lanes fill the last 64 positions, the ragged tail
    of the last tile and (two messages a thread) a thread's second message."""
    q = o.grain_keys(TC, rng.integers(0, hi, size=n))
    if n > 64:
        q[n - 64:] = _edge_keys(D, live)[np.arange(64) % 9]
    return q


ALL_STATUSES = {o.ST_OK, o.ST_MISS, o.ST_SYSTEM_TARGET, o.ST_MEMBERSHIP, o.ST_KEYEXT}

# grids of 1, 2, 3, 7, 8, 9, 15, 16, 17 and 40 tiles of 512 (14 * 512 + 1 for the 15)
N_BIG = [1, 2, 255, 256, 257, 511, 512, 513, 1023, 1025, 3583, 3584, 3585, 4096, 4097, 7 * 512 + 300, 8 * 512 + 1,
         14 * 512 + 1, 15 * 512 + 511, 16 * 512, 17 * 512 - 255, 20001]
# grids of 1, 2, 7, 8, 9, 15, 16, 17 and 79 tiles of 256
N_SMALL = [1, 255, 256, 257, 6 * 256 + 1, 7 * 256 + 1, 8 * 256, 8 * 256 + 1, 9 * 256 - 1, 14 * 256 + 255, 16 * 256,
           17 * 256, 20001]
assert {-(-n // 512) for n in N_BIG} == {1, 2, 3, 7, 8, 9, 15, 16, 17, 40}
assert {-(-n // 256) for n in N_SMALL} == {1, 2, 7, 8, 9, 15, 16, 17, 79}


def _tile_edges(a, b, spec, n_list, seed):
    """Registers the sparse 6,000, gets the table built and routes one batch per n; one build in all."""
    rng = np.random.default_rng(seed)
    base = _builds(a)
    G = 6000
    ids = _sparse_ids(G)
    reg = o.grain_keys(TC, ids)
    acts, own = (ids * 2 + 5).astype(np.uint32), _owner(spec, reg)
    for e in (a, b):
        e.register(reg, acts, own)
    d = o.DirectoryArrays(reg, acts, own)
    D = _d_of(G - 1)
    q = _batch(rng, 20001, G + 200, D, 7)
    _check(a, b, q, spec, d)
    assert _builds(a) == base                                # quiescence rule: no table yet
    _check(a, b, q, spec, d)
    assert _builds(a) == base + 1
    assert ALL_STATUSES <= set(_expect(q, spec, d)[0].tolist())
    for n in n_list:
        qn = _batch(rng, n, G + 200, D, int(ids[rng.integers(0, len(ids))]))
        if n > 64:                                           # d - 1 a hit, d and d + 1 misses: not a pass on misses
            assert _expect(qn[n - 64:n - 61], spec, d)[0].tolist() == [o.ST_OK, o.ST_MISS, o.ST_MISS]
        _check(a, b, qn, spec, d)
    assert _builds(a) == base + 1


@pytest.mark.parametrize("mode", ["D", "V"])
def test_large_index_key_form(gd, big, mode):
    """k_route_d<MODE, 2, false, 0> (eng_route.hip route_mode: index_bytes > ROUTE_NT_INDEX_BYTES): base =
    xcd_tile(..) * 512 + tid, the second message at + 256; every grid size from 1 to 17 workgroups."""
    spec = _reset(big, mode)
    assert big.stats()["table_capacity"] * 8 > ROUTE_NT_INDEX_BYTES
    b = _engine(gd, mode, CAP, 0)
    _tile_edges(big, b, spec, N_BIG, 21)
    b.close()


@pytest.mark.parametrize("mode", ["D", "V"])
def test_small_index_tile_edges(gd, mode):
    """k_route_d<MODE, 1, true, 0> over tiles of 256 at the same edges (the handle's default workgroup order:
    XCD ranges; no option turns them off)."""
    (a, b), spec = _pair(gd, mode)
    assert a.stats()["table_capacity"] * 8 <= ROUTE_NT_INDEX_BYTES
    _tile_edges(a, b, spec, N_SMALL, 22)
    a.close()
    b.close()


@pytest.mark.parametrize("wire", [2, 1])
def test_large_index_n1_stream_forms(gd, big, wire):
    """k_route_d<MODE, 1, false, 4> (u32 headers) and <.., 8> (u64): route_n1_device's !nt branches with the table built."""
    rng = np.random.default_rng(23)
    spec = _reset(big, "D")
    big.set_option("wire_headers", wire)
    b = _engine(gd, "D", CAP, 0, wire_headers=wire, region_probe=0)
    gd.GrainDispatch.comm_init_local([b])
    base = _builds(big)
    G = 6000
    ids = _sparse_ids(G)
    reg = o.grain_keys(TC, ids)
    acts, own = ids.astype(np.uint32), _owner(spec, reg)
    for e in (big, b):
        e.register(reg, acts, own)
    d = o.DirectoryArrays(reg, acts, own)
    D = _d_of(G - 1)
    n1 = np.concatenate([rng.integers(0, G + 8, size=40013), [D - 1, D, D + 1, G - 1]])
    if wire == 1:
        n1 = np.concatenate([n1, [(1 << 32) + 7, (1 << 40)]])     # forces u64 headers; low word a live entry's
    q = o.grain_keys(TC, n1)
    try:
        for step in range(3):
            for e in (big, b):
                res = e.route_multi(q, G, no_keys=True)
                st, silo, act = _expect(q[res["recv_idx"]], spec, d)
                np.testing.assert_array_equal(res["status"], st)
                np.testing.assert_array_equal(res["silo"], silo)
                np.testing.assert_array_equal(res["act"], act)
            assert _builds(big) == base + (0 if step == 0 else 1)
        assert (st == o.ST_OK).sum() > 30000 and (st == o.ST_MISS).sum() > 1000
    finally:
        big.set_option("wire_headers", 0)
        b.comm_destroy()
        b.close()


class _Live:
    """The directory as the test believes it: key -> (act, silo)."""

    def __init__(self, keys, acts, silos):
        self.m = {}
        self.put(keys, acts, silos)

    def put(self, keys, acts, silos):
        for k, x, s in zip(np.asarray(keys).tolist(), acts, silos):
            self.m[tuple(k)] = (int(x), int(s))

    def drop(self, keys):
        for k in np.asarray(keys).tolist():
            del self.m[tuple(k)]

    def has(self, keys):
        return np.array([tuple(k) in self.m for k in np.asarray(keys).tolist()])

    def arrays(self):
        keys = np.array(list(self.m.keys()), np.uint64).reshape(-1, 3)
        vals = np.array(list(self.m.values()), np.uint32).reshape(-1, 2)
        return o.DirectoryArrays(keys, vals[:, 0], vals[:, 1])


def _rebuilt_by_full_build(a, b, q, spec, d, builds):
    """After a write that did not re-project its slots (tab_gen): the next route rebuilds the 8-B index and
    finds it quiet, the one after builds the table once."""
    _check(a, b, q, spec, d)
    assert _builds(a) == builds
    _check(a, b, q, spec, d)
    assert _builds(a) == builds + 1
    _check(a, b, q, spec, d)
    assert _builds(a) == builds + 1
    return builds + 1


@pytest.mark.parametrize("writer", ["upsert", "register_async", "register", "merge_split", "remove_silos",
                                    "upsert_values"])
def test_every_n1_max_writer(gd, writer):
    """With the table built over 0..5,999 (d = 6,000) each writer adds grains at N1 = G + 1, d, d + 1 and
    9,000: gd_dir_upsert (k_cx_sync), the asynchronous and the synchronous registration
    (k_reg_commit_elect_cx), gd_dir_merge, gd_dir_split with the moved entries registered again, and
    gd_dir_remove_silos (the full build's k_cx_types).  The very next route is exact and builds nothing;
    once quiet the table is rebuilt once, with the new d.  upsert_values changes silo and activation of
    300 grains and no key: the same d, the same buffer, the new words."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(24)
    (a, b), spec = _pair(gd)
    G = 6000
    reg = o.grain_keys(TC, np.arange(G))
    acts, own = np.arange(G, dtype=np.uint32) + 9, _owner(spec, reg)
    live = _Live(reg, acts, own)
    for e in (a, b):
        e.register(reg, acts, own)
    D = _d_of(G - 1)
    assert D == G
    new_ids = np.unique([G + 1, D, D + 1, 9000])
    D2 = _d_of(9000)
    new = o.grain_keys(TC, new_ids)
    nacts, nown = np.arange(1, len(new) + 1, dtype=np.uint32), _owner(spec, new)   # within the index's activation bits
    q = np.concatenate([_batch(rng, 20001, G + 400, D, 11), new,
                        o.grain_keys(TC, np.array([D - 1, D, D + 1, D2 - 1, D2, D2 + 1, 8999, 9001]))])
    _check(a, b, q, spec, live.arrays())
    _check(a, b, q, spec, live.arrays())
    n = 1
    assert _builds(a) == n

    def new_ok():
        st = _expect(new, spec, live.arrays())[0]
        return (st == o.ST_OK) == live.has(new)

    if writer in ("upsert", "register", "register_async"):
        if writer == "register_async":
            dk = torch.from_numpy(new.view(np.int64)).to(dev)
            dv = torch.from_numpy(np.stack([nacts, nown], 1).view(np.int32)).to(dev)
        for e in (a, b):
            if writer == "upsert":
                assert e.upsert(new, nacts, nown).all()
            elif writer == "register":
                assert e.register(new, nacts, nown)[2].all()
            else:
                e.register_device_async(dk.data_ptr(), dv.data_ptr(), len(new))
        live.put(new, nacts, nown)
        _check(a, b, q, spec, live.arrays())                 # at once: the batch itself set the table aside
        assert _builds(a) == n
        n = _settle(a, b, q, spec, live.arrays(), n)
        assert live.has(new).all() and new_ok().all()
    elif writer == "upsert_values":
        up = rng.choice(G, size=300, replace=False)
        before = _expect(reg[up], spec, live.arrays())
        acts2, own2 = acts[up] + 1000, (own[up] + 1) % 8     # both within the index's bits
        for e in (a, b):
            assert not e.upsert(reg[up], acts2, own2).any()
        live.put(reg[up], acts2, own2)
        _check(a, b, q, spec, live.arrays())
        assert _builds(a) == n
        n = _settle(a, b, q, spec, live.arrays(), n)
        for e in (a, b):                                     # the rebuilt words
            st, silo, act = e.route(reg[up])
            assert (st == o.ST_OK).all()
            np.testing.assert_array_equal(silo, own2)
            np.testing.assert_array_equal(act, acts2)
            assert (silo != before[1]).all() and (act != before[2]).all()
    elif writer == "merge_split":
        for e in (a, b):
            st = e.merge(new, nacts, nown)[0]
            assert (st == ds.MERGE_INSERTED).all(), st       # absent grains
        live.put(new, nacts, nown)
        n = _rebuilt_by_full_build(a, b, q, spec, live.arrays(), n)
        assert new_ok().all()
        gone = int(nown[-1])                                 # the silo owning 9,000 hands its grains off
        keep = [s for s in range(8) if s != gone]
        moved = [e.split(keep, move=True) for e in (a, b)]
        mk, ma, ms = moved[0]
        assert len(mk) > 100 and (ms == gone).all()
        assert sorted(map(tuple, mk.tolist())) == sorted(map(tuple, moved[1][0].tolist()))
        assert sorted(map(tuple, mk.tolist())) == sorted(k for k, v in live.m.items() if v[1] == gone)
        live.drop(mk)
        _check(a, b, q, spec, live.arrays())                 # the moved grains miss (9,000 among them)
        assert _builds(a) == n and not live.has(new[-1:]).any()
        for e in (a, b):
            assert e.register(mk, ma, ms)[2].all()
        live.put(mk, ma, ms)
        # the route after the split rebuilt the 8-B index, so this registration projected its own slots
        # (k_reg_commit_elect_cx raises n1_max back to 9,000): pure again only after a read-back
        _check(a, b, q, spec, live.arrays())
        assert _builds(a) == n
        n = _settle(a, b, q, spec, live.arrays(), n)
        assert live.has(new).all() and new_ok().all()
    else:
        for e in (a, b):
            e.register(new, nacts, nown)
        live.put(new, nacts, nown)
        n = _settle(a, b, q, spec, live.arrays(), n)
        gone = int(nown[-1])                                 # 9,000 goes: the full build finds a smaller d
        dropped = [k for k, v in live.m.items() if v[1] == gone]
        for e in (a, b):
            assert e.remove_silos([gone])["removed"] == len(dropped)
        live.drop(np.array(dropped, np.uint64))
        n = _rebuilt_by_full_build(a, b, q, spec, live.arrays(), n)
        assert not live.has(new[-1:]).any() and live.has(new).sum() >= 1 and new_ok().all()
    a.close()
    b.close()


def test_eligibility_edge_and_the_way_back(gd):
    """cxd_prepare's dd * 4 > capacity * 8 / 2 at its edge: capacity 2^14, largest N1 16,383 gives dd = 16,384
    (eligible), 16,384 gives 16,400 (not).  A built table turns ineligible (the cx_snap++ line) and comes
    back after a rehash to 2^15; removals leave n1_max, an upper bound, where it was."""
    rng = np.random.default_rng(25)
    (a, b), spec = _pair(gd)
    ids = np.concatenate([np.arange(2999), [16383]])
    reg = o.grain_keys(TC, ids)
    acts, own = np.arange(len(ids), dtype=np.uint32) + 3, _owner(spec, reg)
    live = _Live(reg, acts, own)
    for e in (a, b):
        e.register(reg, acts, own)
    assert _d_of(16383) * 4 == CAP * 8 // 2 and _d_of(16384) * 4 > CAP * 8 // 2
    edge = o.grain_keys(TC, np.array([16383, 16384, 16382, 16385, 16399, 16400, 16401]))
    q = np.concatenate([_batch(rng, 20001, 3400, 16384, 11), edge])
    _check(a, b, q, spec, live.arrays())
    assert _builds(a) == 0
    _check(a, b, q, spec, live.arrays())
    assert _builds(a) == 1
    assert _expect(edge[:2], spec, live.arrays())[0].tolist() == [o.ST_OK, o.ST_MISS]
    # one grain more: the table would outweigh half the 8-B index
    more = o.grain_keys(TC, np.array([16384]))
    for e in (a, b):
        e.register(more, [7], _owner(spec, more))
    live.put(more, [7], _owner(spec, more))
    _check(a, b, q, spec, live.arrays())
    a.stats()
    for _ in range(3):
        _check(a, b, q, spec, live.arrays())
    assert _builds(a) == 1
    assert _expect(edge[:2], spec, live.arrays())[0].tolist() == [o.ST_OK, o.ST_OK]
    # a larger index: eligible again
    for e in (a, b):
        e.rehash(1 << 15)
    assert a.stats()["table_capacity"] == 1 << 15
    n = _rebuilt_by_full_build(a, b, q, spec, live.arrays(), 1)
    # both edge grains leave; d stays (n1_max only grows between full builds)
    for e in (a, b):
        assert e.unregister(edge[:2], [int(acts[-1]), 7]).all()
    live.drop(edge[:2])
    _check(a, b, q, spec, live.arrays())
    assert _builds(a) == n
    n = _settle(a, b, q, spec, live.arrays(), n)
    want = _expect(edge[:2], spec, live.arrays())
    assert want[0].tolist() == [o.ST_MISS, o.ST_MISS]
    np.testing.assert_array_equal(want[1], _owner(spec, edge[:2]))
    a.close()
    b.close()


def _dense_pair(gd, G=6000, **opts):
    (a, b), spec = _pair(gd, **opts)
    reg = o.grain_keys(TC, np.arange(G))
    acts, own = np.arange(G, dtype=np.uint32), _owner(spec, reg)
    for e in (a, b):
        e.register(reg, acts, own)
    return a, b, spec, reg, acts, own


def test_route_bucket_with_the_table(gd):
    """gd_route_bucket (the fused path the benchmark times): the third call reads the table; status, silo
    and act against the oracle, perm and offsets against the stable partition."""
    rng = np.random.default_rng(26)
    G = 6000
    a, b, spec, reg, acts, own = _dense_pair(gd, G)
    d = o.DirectoryArrays(reg, acts, own)
    q = _batch(rng, 70001, G * 5 // 4, _d_of(G - 1), 11)       # a fifth unregistered
    want = _expect(q, spec, d)
    assert 0.15 < (want[0] == o.ST_MISS).mean() < 0.25
    wp, wo = o.bucket_stable(want[2], G)
    for call in range(3):
        for e in (a, b):
            st, silo, act, perm, off = e.route_bucket(q, G)
            for x, y in zip((st, silo, act, perm, off), want + (wp, wo)):
                np.testing.assert_array_equal(x, y)
        assert _builds(a) == (0 if call == 0 else 1)
    a.close()
    b.close()


def test_pipelined_route_bucket_with_the_table(gd):
    """gd_route_bucket_device with a bucket stream (gd_set_bucket_stream): five batches back to back with no
    host synchronisation; the table is built on the handle's stream between batch 1's route and batch
    2's, under batch 1's bucketing."""
    import torch
    from orleans_amd.sharded import DeviceEngine
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(27)
    G, N = 6000, (1 << 16) + 17
    a, b, spec, reg, acts, own = _dense_pair(gd, G)
    d = o.DirectoryArrays(reg, acts, own)
    eng = DeviceEngine(a, dev, pipeline=True)
    batches = [_batch(rng, N, G + 300, _d_of(G - 1), 11 + i) for i in range(5)]
    with torch.cuda.stream(eng.stream):
        keys = [torch.from_numpy(q.view(np.int64)).to(dev) for q in batches]
        res = [eng.route_bucket(k, G) for k in keys]          # no host synchronisation between batches
        eng.stream.wait_stream(eng.bstream)
    torch.cuda.synchronize()
    a.synchronize()                                            # surfaces any deferred device error
    for q, (st, silo, act, perm, off) in zip(batches, res):
        want = _expect(q, spec, d)
        np.testing.assert_array_equal(st.cpu().numpy(), want[0])
        np.testing.assert_array_equal(silo.cpu().numpy().view(np.uint32), want[1])
        np.testing.assert_array_equal(act.cpu().numpy().view(np.uint32), want[2])
        wp, wo = o.bucket_stable(want[2], G)
        np.testing.assert_array_equal(perm.cpu().numpy().view(np.uint32), wp)
        np.testing.assert_array_equal(off.cpu().numpy().view(np.uint32), wo)
        for x, y in zip(b.route(q), want):
            np.testing.assert_array_equal(x, y)
    assert _builds(a) == 1
    a.set_bucket_stream(None)
    a.set_stream(None)
    a.close()
    b.close()


def test_route_frames_with_the_table(gd):
    """gd_route_frames: decode -> route over frames written by the oracle's header writer, after two plain
    routes have built the table."""
    import headers as H
    rng = np.random.default_rng(28)
    G = 6000
    a, b, spec, reg, acts, own = _dense_pair(gd, G)
    d = o.DirectoryArrays(reg, acts, own)
    q = _batch(rng, 20001, G + 200, _d_of(G - 1), 11)
    _check(a, b, q, spec, d)
    _check(a, b, q, spec, d)
    assert _builds(a) == 1
    n = 3001
    keys = _batch(rng, n, G + 500, _d_of(G - 1), 12)
    buf, off = H.random_frames(n, keys, rng, p_fallback=0.03, p_complete=0.1, p_malformed=0.02)
    f, wst, wsilo, wact = H.route_frames_np(buf, off, spec, d)
    assert (wst == o.ST_OK).sum() > 2000 and (wst == o.ST_MISS).sum() > 100
    wp, wo = o.bucket_stable(wact, G)
    for e in (a, b):
        dec, st, silo, act, perm, offs = e.route_frames(buf, off, n_act=G)
        np.testing.assert_array_equal(dec["target_grain"], f["target_grain"])
        np.testing.assert_array_equal(st, wst)
        np.testing.assert_array_equal(silo, wsilo)
        np.testing.assert_array_equal(act, wact)
        np.testing.assert_array_equal(perm, wp)
        np.testing.assert_array_equal(offs, wo)
    assert _builds(a) == 1
    a.close()
    b.close()


@pytest.mark.parametrize("zero_copy", [0, 1])
def test_microbatch_with_the_table(gd, zero_copy):
    """Micro-batches beside a built table.  Staged micro-batches (GD_OPT_MB_ZEROCOPY 0) route through
    route_device (eng_abi.hip mb_enqueue, its `else if (n)` branch): an eager run reads the table; a capture
    takes the directory probe (cx_ensure under capture) and its cxd_prepare(cx = false) clears cxd_seen.
    Zero-copy ones launch k_mb_route and never reach cxd_prepare.  The expected build counts follow
    cxd_prepare: a table built under the current snapshot id is read without the quiet condition (the
    `cxd_ok && cxd_snap_at == snap` test), so a capture costs no rebuild; a new table is built only when the
    previous k_route launch found the index pure under the same id, so on a staged handle a capture between
    two quiet routes puts the build off by one route, and on a zero-copy handle it does not."""
    rng = np.random.default_rng(29)
    G = 6000
    a, b, spec, reg, acts, own = _dense_pair(gd, G, mb_zerocopy=zero_copy)
    live = _Live(reg, acts, own)
    q = _batch(rng, 20001, G + 200, _d_of(G - 1), 11)
    _check(a, b, q, spec, live.arrays())
    _check(a, b, q, spec, live.arrays())
    assert _builds(a) == 1
    mbs = [gd.MicroBatch(e, 4096, G) for e in (a, b)]

    def run(n, use_graph):
        want = _expect(q[-n:], spec, live.arrays())
        for mb in mbs:
            mb.keys[:n] = q[-n:]
            mb.run(n, use_graph)
            np.testing.assert_array_equal(mb.status[:n], want[0])
            np.testing.assert_array_equal(mb.silo[:n], want[1])
            np.testing.assert_array_equal(mb.act[:n], want[2])
        return want

    assert ALL_STATUSES <= set(run(4096, False)[0].tolist())
    assert _builds(a) == 1
    run(4096, True)
    assert _builds(a) == 1
    _check(a, b, q, spec, live.arrays())                     # the snapshot id did not move: the same table
    assert _builds(a) == 1
    # a change: every path shows it at once
    up = np.concatenate([reg[rng.choice(G, size=200, replace=False)], o.grain_keys(TC, np.array([G + 5]))])
    uacts, uown = np.arange(len(up), dtype=np.uint32) + 1, (_owner(spec, up) + 3) % 8
    for e in (a, b):
        e.upsert(up, uacts, uown)
    live.put(up, uacts, uown)
    q[-len(up) - 64:-64] = up
    want = run(4096, False)
    assert (want[0] == o.ST_OK).sum() > 3000
    np.testing.assert_array_equal(want[2][-len(up) - 64:-64], uacts)
    run(4096, True)
    _check(a, b, q, spec, live.arrays())
    assert _builds(a) == 1
    # quiet again, with a capture (a new batch size) between the two quiet routes
    a.stats()
    _check(a, b, q, spec, live.arrays())
    assert _builds(a) == 1
    run(4095, True)
    _check(a, b, q, spec, live.arrays())
    assert _builds(a) == (2 if zero_copy else 1)
    _check(a, b, q, spec, live.arrays())
    assert _builds(a) == 2
    _check(a, b, q, spec, live.arrays())
    run(4096, False)
    assert _builds(a) == 2
    for mb in mbs:
        mb.close()
    a.close()
    b.close()


def _two_classes(spec, G):
    """G grains of the ping class and 50 of another: the 8-B index holds two types, so it is never pure."""
    reg = np.concatenate([o.grain_keys(TC, np.arange(G)), o.grain_keys(0x777, np.arange(50))])
    assert (reg[G:, 2] == np.uint64(OTHER_TCD)).all()
    return reg, (np.arange(len(reg), dtype=np.uint32) * 2 + 1), _owner(spec, reg)


def _share_batches(rng, share, hi):
    """n = 1 and one below, at and one past one workgroup's share of messages; keys 0..hi-1 (some unregistered)
    with an N0 != 0 key and a key of the other class among them."""
    out = []
    for n in (1, share - 1, share, share + 1):
        q = o.grain_keys(TC, rng.integers(0, hi, size=n))
        if n > 8:
            q[n - 2, 0] = 5
            q[n - 1] = o.grain_keys(0x777, np.array([3]))[0]
        out.append(q)
    return out


@pytest.mark.parametrize("probe", [0, 2, 3, 4])
def test_large_index_pinned_forms(gd, big, probe):
    """k_route_m<MODE, 2, false, 0, ...> (route_mode over a 2^24-slot table: two messages a thread, temporal
    keys) in the directory form (GD_OPT_PROBE 0), the 16-B index in group reads (2) and slot reads (3) and the
    8-B index with a directory fallback (4, two grain classes: not pure, so neither the PURE form nor the
    direct table); a workgroup's share is 512 messages."""
    rng = np.random.default_rng(30 + probe)
    spec = _reset(big, "D")
    big.set_option("probe", probe)
    b = _engine(gd, "D", CAP, 0)
    try:
        base = _builds(big)
        G = 6000
        reg, acts, own = _two_classes(spec, G)
        for e in (big, b):
            e.register(reg, acts, own)
        d = o.DirectoryArrays(reg, acts, own)
        assert big.stats()["table_capacity"] * 8 > ROUTE_NT_INDEX_BYTES
        qs = _share_batches(rng, 512, G + 600)
        for q in qs + qs:
            _check(big, b, q, spec, d)
        want = _expect(qs[3], spec, d)[0]
        assert (want == o.ST_OK).sum() > 400 and (want == o.ST_MISS).sum() > 10
        assert _builds(big) == base
    finally:
        big.set_option("probe", 4)
        b.close()


@pytest.mark.parametrize("wire", [2, 1])
@pytest.mark.parametrize("probe", [2, 3])
def test_n1_stream_index16_forms(gd, probe, wire):
    """k_route_m<MODE, 1, false, 4 | 8, true, CX_GROUP | 1>: the N1 routes (u32 and u64 headers of a world-1
    exchange) over the 16-B index in group reads (GD_OPT_PROBE 2) and slot reads (3); a workgroup's share is
    256 messages."""
    rng = np.random.default_rng(40 + probe * 2 + wire)
    spec = o.ring_spec(SILOS, "D")
    es = [_engine(gd, "D", CAP, p, wire_headers=wire, region_probe=0) for p in (probe, 0)]
    G = 6000
    reg = o.grain_keys(TC, np.arange(G))
    acts, own = np.arange(G, dtype=np.uint32) + 7, _owner(spec, reg)
    for e in es:
        e.register(reg, acts, own)
        gd.GrainDispatch.comm_init_local([e])
    d = o.DirectoryArrays(reg, acts, own)
    try:
        for n in (1, 255, 256, 257):
            n1 = rng.integers(0, G + 600, size=n)
            if wire == 1 and n > 1:
                n1[0] = (1 << 32) + 5                            # above 2^32; its low word a live entry's
            q = o.grain_keys(TC, n1)
            for e in es:
                res = e.route_multi(q, G, no_keys=True)
                st, silo, act = _expect(q[res["recv_idx"]], spec, d)
                np.testing.assert_array_equal(res["status"], st)
                np.testing.assert_array_equal(res["silo"], silo)
                np.testing.assert_array_equal(res["act"], act)
            if n > 1:
                assert (st == o.ST_OK).sum() > n // 2 and (st == o.ST_MISS).sum() >= 1
    finally:
        for e in es:
            e.comm_destroy()
            e.close()


@pytest.mark.parametrize("form", ["keys", "u32", "u64"])
def test_region_forms(gd, form):
    """k_route_region<MODE, 0 | 4 | 8>: a world-1 exchange with GD_OPT_REGION_PROBE 1 hands the owner its chunk
    grouped by table region, as 24-B keys (a batch of two grain classes does not compact), u32 N1s
    (GD_OPT_WIRE_HEADERS 2) or u64 N1s (1); a workgroup's share is 256 messages of one region."""
    wire = 1 if form == "u64" else 2
    rng = np.random.default_rng(50 + wire + (form == "keys"))
    spec = o.ring_spec(SILOS, "D")
    es = [_engine(gd, "D", CAP, p, wire_headers=wire, region_probe=1) for p in (4, 0)]
    G = 6000
    reg = o.grain_keys(TC, np.arange(G))
    acts, own = np.arange(G, dtype=np.uint32) + 7, _owner(spec, reg)
    for e in es:
        e.register(reg, acts, own)
        gd.GrainDispatch.comm_init_local([e])
    es[0].set_kernel_timing(True)
    d = o.DirectoryArrays(reg, acts, own)
    try:
        for n in (1, 255, 256, 257, 8 * 256 + 1):
            q = o.grain_keys(TC, rng.integers(0, G + 600, size=n))
            if form == "keys" and n > 1:
                q[n // 2, 2] = np.uint64(OTHER_TCD)              # a second class: 24-B headers
            for keep in (False, True):                           # no_keys: the N1s probed as received
                for e in es:
                    res = e.route_multi(q, G, no_keys=not keep)
                    assert sorted(res["recv_idx"].tolist()) == list(range(n))
                    st, silo, act = _expect(q[res["recv_idx"]], spec, d)
                    np.testing.assert_array_equal(res["status"], st)
                    np.testing.assert_array_equal(res["silo"], silo)
                    np.testing.assert_array_equal(res["act"], act)
                    r = o.table_region_np(q[res["recv_idx"]])    # grouped by region
                    assert (np.diff(r.astype(np.int64)) >= 0).all()
    finally:
        for e in es:
            e.comm_destroy()
            e.close()


@pytest.mark.parametrize("large", [False, True])
def test_route_bound_forms(gd, big, large):
    """k_route_bound<2, true> (an index up to ROUTE_NT_INDEX_BYTES) and <2, false> (the 2^24-slot table): a
    diagnostic, not a route -- it reads the home group of the 8-B index only.  With one grain class, N0 = 0 and
    N1 < 2^32 a slot matching the key's low N1 word is the key's own entry, so every message it reports found
    (status 0) carries the oracle's silo and activation, and a key the directory does not hold is never found;
    at load 0.37 or less most entries lie in their home group.  A workgroup's share is 512 messages."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(60 + large)
    if large:
        a, spec = big, _reset(big, "D")
    else:
        a, spec = _engine(gd, "D", CAP, 4), o.ring_spec(SILOS, "D")
    b = _engine(gd, "D", CAP, 0)
    try:
        assert (a.stats()["table_capacity"] * 8 > ROUTE_NT_INDEX_BYTES) == large
        G = 6000
        reg = o.grain_keys(TC, np.arange(G))
        acts, own = np.arange(G, dtype=np.uint32) + 7, _owner(spec, reg)
        for e in (a, b):
            e.register(reg, acts, own)
        d = o.DirectoryArrays(reg, acts, own)
        found = total = 0
        for n in (1, 511, 512, 513, 4 * 512 + 1):
            q = o.grain_keys(TC, rng.integers(0, G + 600, size=n))
            _check(a, b, q, spec, d)
            wst, wsilo, wact = _expect(q, spec, d)
            dk = torch.from_numpy(q.view(np.int64)).to(dev)
            silo = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            act = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            st = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()                             # the fills ran on torch's stream
            a.route_bound_device(dk.data_ptr(), n, silo.data_ptr(), act.data_ptr(), st.data_ptr())
            a.synchronize()
            silo, act, st = silo.cpu().numpy().view(np.uint32), act.cpu().numpy().view(np.uint32), st.cpu().numpy()
            assert (silo[n:] == 0x5A5A5A5A).all() and (act[n:] == 0x5A5A5A5A).all() and (st[n:] == 0x5A).all()
            hit = st[:n] == 0
            assert set(st[:n].tolist()) <= {0, 1}
            assert (wst[hit] == o.ST_OK).all()
            np.testing.assert_array_equal(silo[:n][hit], wsilo[hit])
            np.testing.assert_array_equal(act[:n][hit], wact[hit])
            found += int(hit.sum())
            total += int((wst == o.ST_OK).sum())
        assert found > total // 2
    finally:
        b.close()
        if not large:
            a.close()
