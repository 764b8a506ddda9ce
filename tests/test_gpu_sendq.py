"""GPU parity for the sender-queue stage: gd_send_queues / gd_route_send through the C
ABI against the literal restatement of OutboundMessageQueue.SendMessage's queue rule (_sendq_ref.py),
bit for bit: send status, bucket id, the per-queue index lists (perm) and their starts (offsets)."""
import numpy as np
import pytest

import _sendq_ref as R
import oracle as o

pytestmark = pytest.mark.gpu

TILE = 4096                      # k_sendq_scatter's messages per workgroup (gd_sendq.h SQ_TILE)
MY = 2


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


def _engine(gd, sh, nq, my_silo=MY, **kw):
    e = gd.GrainDispatch(device=0, table_capacity=1024, my_silo=my_silo, **kw)
    e.send_configure(sh, nq)
    return e


def _check(got, want):
    for name, a, b in zip(("send_status", "queue", "perm", "offsets"), got, want):
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a, b, err_msg=name)


def _run(e, batch, sh, nq, my_silo=MY):
    silo, rs, cat, ttl = batch
    _check(e.send_queues(silo, rs, cat, ttl), R.send_queues_loop(silo, rs, cat, ttl, sh, nq, my_silo))


SHAPES = [(0, 1), (0, 252), (1, 2), (1, 1024), (63, 7), (63, 64), (64, 1), (64, 252), (65, 2), (65, 7),
          (TILE - 1, 64), (TILE - 1, 1024), (TILE, 7), (TILE, 252), (TILE + 1, 1), (TILE + 1, 64),
          (3 * TILE + 17, 2), (3 * TILE + 17, 1024), (200003, 64), (200003, 252)]


@pytest.mark.parametrize("n,nq", SHAPES)
def test_shapes_mixed_batch(gd, n, nq):
    """Every n with two queue counts, every queue count with three or more n; all seven statuses and
    every category in the batch once it has a few hundred messages."""
    rng = np.random.default_rng(n * 31 + nq)
    n_silos = 8 if (n + nq) % 2 else 300
    sh = R.hashes_with_edges(rng, n_silos)
    with _engine(gd, sh, nq) as e:
        batch = R.mixed_batch(rng, n, n_silos, MY)
        _run(e, batch, sh, nq)
        if n >= 4000 and (n_silos == 8 or n > 100000):
            st = R.send_queues_np(*batch, sh, nq, MY)[0]
            assert set(np.unique(st).tolist()) == set(range(7))
            assert {0, 1, 2} <= set(np.unique(batch[2]).tolist())


def _distribution(kind, rng, n, n_silos):
    """(silo, route status, category, ttl); None = the optional array is not passed."""
    if kind in ("uniform8", "uniform300"):
        return rng.integers(0, n_silos, size=n).astype(np.uint32), None, None, None
    if kind == "hot":                # every message to one remote silo: one hot bucket
        return np.full(n, (MY + 3) % n_silos, np.uint32), None, None, None
    if kind == "loopback":
        return np.full(n, MY, np.uint32), None, None, None
    if kind == "expired":            # every bucket but the trailing one is empty
        return (rng.integers(0, n_silos, size=n).astype(np.uint32), None, None,
                -rng.integers(0, 1 << 40, size=n).astype(np.int64))
    return R.mixed_batch(rng, n, n_silos, MY)


@pytest.mark.parametrize("no_lane_order", [False, True])
@pytest.mark.parametrize("kind", ["uniform8", "uniform300", "hot", "loopback", "expired", "mix"])
def test_distributions(gd, kind, no_lane_order):
    """3 * TILE + 17 messages; with and without the LDS lane order (GD_CFG_NO_LANE_ORDER: ballot ranks).
    uniform / hot / loopback pass no optional array at all."""
    rng = np.random.default_rng(7)
    n, nq = 3 * TILE + 17, 7
    n_silos = 300 if kind == "uniform300" else 8
    sh = R.hashes_with_edges(rng, n_silos)
    if kind == "hot":
        sh[(MY + 3) % n_silos] = 12345               # an ordinary hash: the hot bucket is an application queue
    with _engine(gd, sh, nq, no_lane_order=no_lane_order) as e:
        _run(e, _distribution(kind, rng, n, n_silos), sh, nq)
        # classification only (perm + offsets NULL) gives the same status and bucket ids
        silo, rs, cat, ttl = _distribution(kind, rng, 1000, n_silos)
        st, q = e.send_queues(silo, rs, cat, ttl, bucket=False)
        want = R.send_queues_loop(silo, rs, cat, ttl, sh, nq, MY)
        np.testing.assert_array_equal(st, want[0])
        np.testing.assert_array_equal(q, want[1])


def test_hot_bucket_every_shape_of_rank(gd):
    """One hot application queue at 1,024 queues (11-bit bucket ids), ballot ranks and lane-order ranks."""
    rng = np.random.default_rng(11)
    n, nq, n_silos = 3 * TILE + 17, 1024, 8
    sh = R.hashes_with_edges(rng, n_silos)
    sh[5] = -1000003
    batch = (np.full(n, 5, np.uint32), None, None, None)
    for nlo in (False, True):
        with _engine(gd, sh, nq, no_lane_order=nlo) as e:
            _run(e, batch, sh, nq)


def test_real_silo_table(gd):
    silos = o.bench_silos(8)
    sh = np.array([gd.silo_consistent_hash(s.ip, s.port, s.gen) for s in silos], np.int32)
    assert sh.tolist() == [s.consistent_hash() for s in silos]
    rng = np.random.default_rng(3)
    for nq in (1, 16):
        with _engine(gd, sh, nq) as e:
            _run(e, R.mixed_batch(rng, 20000, 8, MY), sh, nq)


def test_synthetic_table_edges(gd):
    """INT32_MIN (Math.Abs throws), -1, 0, 1 and INT32_MAX, every silo hit by every category."""
    sh = np.array([R.INT32_MIN, -1, 0, 1, (1 << 31) - 1, 77], np.int32)
    n = 6 * 4 * 50
    silo = np.tile(np.arange(6, dtype=np.uint32), n // 6)
    cat = np.repeat(np.array([0, 1, 2, 7], np.uint8), n // 4)
    for nq in (1, 2, 7, 1024):
        with _engine(gd, sh, nq, my_silo=5) as e:
            _run(e, (silo, None, cat, None), sh, nq, my_silo=5)
            st, q = e.send_queues(silo, None, cat, None, bucket=False)
            assert (st[(silo == 0) & (cat >= 2)] == gd.SEND_THROWS).all()
            assert (q[(silo == 0) & (cat == 0)] == 1).all()        # a Ping to the INT32_MIN silo is queued


def test_table_past_lds(gd):
    """n_silos = 9,000: 36 KB of table, read through global memory instead of LDS."""
    rng = np.random.default_rng(5)
    n_silos, nq = 9000, 64
    sh = R.hashes_with_edges(rng, n_silos)
    with _engine(gd, sh, nq) as e:
        _run(e, R.mixed_batch(rng, 2 * TILE + 5, n_silos, MY), sh, nq)


def test_configure_again_between_batches(gd):
    rng = np.random.default_rng(9)
    sh = R.hashes_with_edges(rng, 8)
    batch = R.mixed_batch(rng, TILE + 100, 12, MY)
    with _engine(gd, sh, 7) as e:
        _run(e, batch, sh, 7)
        sh2 = R.hashes_with_edges(rng, 12)                          # the silo table grew; another queue count
        e.send_configure(sh2, 252)
        _run(e, batch, sh2, 252)
        e.send_configure(sh, 2)
        _run(e, batch, sh, 2)


def test_unconfigured_handle_is_estate(gd):
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        e.send_n_queues = 4
        with pytest.raises(gd.GrainDispatchError) as ei:
            e.send_queues(np.zeros(4, np.uint32))
        assert ei.value.code == gd.GD_ESTATE and "gd_send_configure" in str(ei.value)
        with pytest.raises(gd.GrainDispatchError) as ei:
            e.send_configure(np.zeros(4, np.int32), 1025)
        assert ei.value.code == gd.GD_EINVAL


def _directory_world(gd, rng):
    """A small directory in ring mode D: registered, unregistered and multi-activation grains, a
    system target, a KeyExt key and the membership table grain; (engine args, keys, oracle route)."""
    silos = o.bench_silos(8)
    spec = o.ring_spec(silos, "D")
    tc = o.grain_type_code(o.PING_GRAIN_CLASS)
    G = 3000
    reg = o.grain_keys(tc, np.arange(G))
    owner = o.ring_owner_np(spec, o.jenkins_u64x3_np(reg[:, 2], reg[:, 0], reg[:, 1])).astype(np.uint32)
    host = rng.integers(0, 8, size=G).astype(np.uint32)            # the activation's silo, any of the 8
    acts = np.arange(G, dtype=np.uint32)
    acts[::17] = o.ACT_MULTI
    n = 2 * TILE + 77
    keys = o.grain_keys(tc, rng.integers(0, G + 400, size=n))      # ~12 % unregistered
    special = np.zeros((3, 3), np.uint64)
    special[0] = (0, 9, o.type_code_data(o.CAT_SYSTEM_TARGET, 12))
    special[1] = (0, 5, o.type_code_data(o.CAT_KEYEXT_GRAIN, tc))
    mt = o.MEMBERSHIP_TABLE_ID
    special[2] = (mt.n0, mt.n1, mt.tcd)
    keys[rng.choice(n, size=300, replace=False)] = np.tile(special, (100, 1))
    want = o.route_batch_np(keys, spec, o.DirectoryArrays(reg, acts, host), my_silo=MY, seed_silo=6)
    return silos, reg, acts, host, keys, want


def test_route_send_fused(gd):
    import torch
    rng = np.random.default_rng(21)
    silos, reg, acts, host, keys, want = _directory_world(gd, rng)
    assert {o.ST_OK, o.ST_MISS, o.ST_SYSTEM_TARGET, o.ST_MEMBERSHIP, o.ST_KEYEXT, o.ST_MULTI_ACT} <= set(want[0].tolist())
    n, nq = len(keys), 16
    sh = np.array([s.consistent_hash() for s in silos], np.int32)
    cat = rng.choice(np.array([2, 2, 2, 0, 1], np.uint8), size=n)
    ttl = rng.integers(-(1 << 30), 1 << 40, size=n).astype(np.int64)
    ttl[::3] = R.TTL_NONE
    ttl[1::7] = 0
    with gd.GrainDispatch(device=0, table_capacity=8192, my_silo=MY, seed_silo=6) as e:
        e.ring_set_silos("D", [(s.ip, s.port, s.gen) for s in silos])
        e.upsert(reg, acts, host)
        e.send_configure(sh, nq)
        r_st, r_silo, r_act = e.route(keys)
        st, silo, act, sst, q, perm, off = e.route_send(keys, cat, ttl)
        for a, b, w in ((st, r_st, want[0]), (silo, r_silo, want[1]), (act, r_act, want[2])):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, w)
        ref = R.send_queues_loop(want[1], want[0], cat, ttl, sh, nq, MY)
        _check((sst, q, perm, off), ref)
        assert set(np.unique(sst).tolist()) >= {R.SEND_QUEUED, R.SEND_LOOPBACK, R.SEND_EXPIRED, R.SEND_HELD}
        # the device form, once with perm / offsets NULL and no category / ttl
        dev = torch.device("cuda:0")
        d_keys = torch.from_numpy(keys.view(np.int64)).to(dev)
        d_silo = torch.empty(n, dtype=torch.int32, device=dev)
        d_act = torch.empty(n, dtype=torch.int32, device=dev)
        d_st = torch.empty(n, dtype=torch.uint8, device=dev)
        d_sst = torch.empty(n, dtype=torch.uint8, device=dev)
        d_q = torch.empty(n, dtype=torch.int32, device=dev)
        e.route_send_device(d_keys.data_ptr(), n, None, None, d_silo.data_ptr(), d_act.data_ptr(), d_st.data_ptr(),
                            d_sst.data_ptr(), d_q.data_ptr(), None, None)
        e.synchronize()
        ref2 = R.send_queues_loop(want[1], want[0], None, None, sh, nq, MY)
        np.testing.assert_array_equal(d_st.cpu().numpy(), want[0])
        np.testing.assert_array_equal(d_silo.cpu().numpy().view(np.uint32), want[1])
        np.testing.assert_array_equal(d_sst.cpu().numpy(), ref2[0])
        np.testing.assert_array_equal(d_q.cpu().numpy().view(np.uint32), ref2[1])


def test_properties_at_4m(gd):
    """4,194,304 messages over 8 silos and 16 queues through the device form: perm is a permutation,
    bucket ids do not decrease along it, indices increase inside each bucket, offsets is the bincount
    prefix; a 100k-message sample of status and bucket id against the literal restatement."""
    import torch
    rng = np.random.default_rng(4)
    n, n_silos, nq = 1 << 22, 8, 16
    B = nq + 4
    sh = R.hashes_with_edges(rng, n_silos)
    silo, rs, cat, ttl = R.mixed_batch(rng, n, n_silos, MY)
    dev = torch.device("cuda:0")
    up = lambda a, t: torch.from_numpy(a.view(t)).to(dev)
    d_silo, d_rs, d_cat, d_ttl = up(silo, np.int32), up(rs, np.uint8), up(cat, np.uint8), up(ttl, np.int64)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_q = torch.empty(n, dtype=torch.int32, device=dev)
    d_perm = torch.empty(n, dtype=torch.int32, device=dev)
    d_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    with _engine(gd, sh, nq) as e:
        e.send_queues_device(d_silo.data_ptr(), d_rs.data_ptr(), d_cat.data_ptr(), d_ttl.data_ptr(), n,
                             d_st.data_ptr(), d_q.data_ptr(), d_perm.data_ptr(), d_off.data_ptr())
        e.synchronize()
    st, q = d_st.cpu().numpy(), d_q.cpu().numpy().view(np.uint32)
    perm, off = d_perm.cpu().numpy().view(np.uint32), d_off.cpu().numpy().view(np.uint32)
    seen = np.zeros(n, bool)
    seen[perm] = True
    assert seen.all()                                               # a permutation of 0 .. n - 1
    qp = q[perm].astype(np.int64)
    assert (np.diff(qp) >= 0).all()
    same = np.diff(qp) == 0
    assert (np.diff(perm.astype(np.int64))[same] > 0).all()         # batch order inside every bucket
    want_off = np.zeros(B + 1, np.uint32)
    want_off[1:] = np.cumsum(np.bincount(q, minlength=B))
    np.testing.assert_array_equal(off, want_off)
    assert q.max() == B - 1 and set(np.unique(st).tolist()) == set(range(7))
    pick = np.sort(rng.choice(n, size=100000, replace=False))
    ref = R.send_queues_loop(silo[pick], rs[pick], cat[pick], ttl[pick], sh, nq, MY)
    np.testing.assert_array_equal(st[pick], ref[0])
    np.testing.assert_array_equal(q[pick], ref[1])
