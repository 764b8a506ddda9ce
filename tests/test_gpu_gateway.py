"""GPU parity for the gateway stage: gd_gateway_* and their device forms through the C ABI against
the literal restatement of Gateway.cs / GatewayAcceptor.cs (_gateway_ref.Gateway), every output bit for bit, dtype
included, and every state word through gd_gateway_lookup and gd_gateway_count after every call."""
import numpy as np
import pytest

import _chain_keys as CK
import _gateway_ref as R
import _sendq_ref as S

pytestmark = pytest.mark.gpu

BLOCK, TILE = 256, 4096                                   # a workgroup; the partition's tile (gd_sendq.h SQ_TILE)
SHAPES = [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, TILE - 1, TILE + 1, 3 * TILE + 17, 70001]
PAD = 64


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


@pytest.fixture()
def eng(gd):
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        yield e


def _eq(got, want, names):
    assert len(got) == len(want) == len(names)
    for name, a, b in zip(names, got, want):
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a, b, err_msg=name)


class Mirror:
    """The engine's tables and the literal ones, driven together."""

    def __init__(self, e, n_senders=3, drop_timeout=500, route_expiry=1900, hint=0):
        self.e, self.t = e, R.Gateway(n_senders, drop_timeout, route_expiry)
        e.gateway_configure(n_senders, drop_timeout, route_expiry, hint)
        self.seen = np.zeros((0, 3), np.uint64)

    def see(self, *ks):
        self.seen = np.unique(np.concatenate([self.seen] + [R.keys(k) for k in ks if k is not None]), axis=0)

    def verify(self):
        _eq(self.e.gateway_lookup(self.seen), self.t.lookup(self.seen), R.LOOKUP_NAMES)
        c = self.e.gateway_count()
        assert c[:2] == self.t.count()
        return c[2:]

    def open(self, ids, handles):
        self.see(ids)
        _eq(self.e.gateway_open(ids, handles), self.t.open(ids, handles), ("handle", "sender", "new", "pending"))
        return self.verify()

    def close(self, ids, now, pending_left=None):
        self.see(ids)
        _eq((self.e.gateway_close(ids, now, pending_left),), (self.t.close(ids, now, pending_left),), ("found",))
        self.verify()

    def drop(self, now, cap=None):
        want = self.t.drop(now, cap)
        if cap is not None and want[3] > cap:
            with pytest.raises(Exception):
                self.e.gateway_drop(now, cap)
        else:
            got = self.e.gateway_drop(now, want[3] if cap is None else cap)
            o = np.lexsort((got[0][:, 2], got[0][:, 1], got[0][:, 0]))   # no order: compared sorted by id
            _eq(tuple(a[o] for a in got), want[:3], ("id", "handle", "pending"))
        self.verify()
        return want[3]

    def routes_expire(self, now):
        want = self.t.routes_expire(now)
        assert self.e.gateway_routes_expire(now) == want
        self.verify()
        return want

    def deliver(self, target, sending, ssilo, now, ttl=None):
        self.see(target, sending)
        want = self.t.deliver(target, sending, ssilo, now, ttl)
        _eq(self.e.gateway_deliver(target, sending, ssilo, now, ttl), want, ("status", "handle", "sender", "perm", "offsets"))
        self.verify()
        return want

    def ingress(self, target, sending, direction, ttl, overloaded, my_silo=0):
        want = self.t.ingress(target, sending, direction, ttl, overloaded, my_silo)
        _eq(self.e.gateway_ingress(target, sending, direction, ttl, overloaded), want, ("status", "silo", "route_idx", "route_keys"))
        self.verify()
        return want


def batch(rng, n, ids, n_grain=64):
    """n messages over the clients `ids` and others, every deliver status possible."""
    grains = R.keys(np.c_[np.zeros(n_grain, np.uint64), np.arange(1, n_grain + 1, dtype=np.uint64),
                          np.full(n_grain, (3 << 56) | 77, np.uint64)])
    absent = R.client_keys(np.arange(8) + (1 << 40))
    pool = np.concatenate([ids, ids, absent, grains, R.with_cat(ids[:4], R.CAT_GEO_CLIENT),
                           R.with_cat(grains[:4], R.CAT_SYSTEM_TARGET)])
    target = pool[rng.integers(0, len(pool), n)]
    spool = np.concatenate([ids[:12], absent[:4], grains[:16], R.with_cat(absent[:2], R.CAT_GEO_CLIENT)])
    sending = spool[rng.integers(0, len(spool), n)]
    ssilo = rng.integers(0, 8, n).astype(np.uint32)
    ssilo[rng.random(n) < 0.2] = R.NO_SILO
    ttl = rng.integers(1, 1 << 40, n).astype(np.int64)
    ttl[rng.random(n) < 0.3] = R.TTL_NONE
    ttl[rng.random(n) < 0.05] = 0
    ttl[rng.random(n) < 0.05] = -5
    return target, sending, ssilo, ttl


def opened(e, n_clients, n_senders=3, seed=0, hint=0, close_some=True):
    rng = np.random.default_rng(seed)
    m = Mirror(e, n_senders, hint=hint)
    ids = R.client_keys(rng.choice(1 << 24, n_clients, replace=False) + 1)
    m.open(ids, np.arange(n_clients, dtype=np.uint32) + 7)
    if close_some and n_clients > 1:
        m.close(ids[::3], 1000, rng.integers(0, 9, len(ids[::3])).astype(np.uint32))
    return m, ids, rng


# ---- lifecycle, shapes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1])
def test_lifecycle_matches_the_loop(gd, seed):
    with gd.GrainDispatch(device=0, table_capacity=1024, my_silo=5) as e:     # lifecycle's ingress calls say silo 5
        m = Mirror(e, 3, *R.LIFECYCLE_TIMEOUTS)
        for call, args in R.lifecycle(np.random.default_rng(seed)):
            getattr(m, call)(*args)


@pytest.mark.parametrize("n", SHAPES)
def test_deliver_shapes(eng, n):
    m, ids, rng = opened(eng, 5, seed=n)
    t, s, ss, ttl = batch(rng, n, ids)
    want = m.deliver(t, s, ss, 2000, ttl)
    if n >= BLOCK - 1:
        assert set(want[0]) == {R.GW_NOT_PROXIED, R.GW_SEND, R.GW_PENDING, R.GW_EXPIRED, R.GW_GEO_CLIENT}
    m.deliver(t, None, None, 2100, None)                   # no sender array: nothing recorded, nothing expires


@pytest.mark.parametrize("n_clients,n_senders", [(1, 1), (5, 3), (4097, 64), (4097, 1024)])
def test_clients_and_senders(eng, n_clients, n_senders):
    m, ids, rng = opened(eng, n_clients, n_senders, seed=n_clients + n_senders)
    t, s, ss, ttl = batch(rng, 3 * TILE + 17, ids)
    m.deliver(t, s, ss, 2000, ttl)
    # all messages to one client (one hot sender bucket); no message to any client
    one = np.repeat(ids[:1], 5000, axis=0)
    m.deliver(one, s[:5000], ss[:5000], 2200)
    m.deliver(R.with_cat(t, 3), s, ss, 2300)


def test_every_status_in_one_wave_and_last_sender_wins(eng):
    m, ids, rng = opened(eng, 5, seed=3)
    gone = R.client_keys([1 << 41])
    t = np.concatenate([ids[:1], ids[1:2], gone, R.with_cat(ids[:1], R.CAT_GEO_CLIENT), ids[2:3]] * 300)[:1400]
    ttl = np.full(len(t), R.TTL_NONE, np.int64)
    ttl[4::5] = 0
    s = np.repeat(ids[4:5], len(t), axis=0)                # the same sending client in a wave, across waves, workgroups
    s[7::11] = ids[2]
    ss = np.arange(len(t), dtype=np.uint32)
    want = m.deliver(t, s, ss, 5000, ttl)
    assert set(want[0][:64]) == {0, 1, 2, 3, 4}
    lk = dict(zip(R.LOOKUP_NAMES, eng.gateway_lookup(ids[4:5])))
    last = max(i for i in range(len(t)) if want[0][i] in (R.GW_SEND, R.GW_PENDING) and not (i % 11 == 7))
    assert lk["route_silo"][0] == last and lk["route_time"][0] == 5000


def test_open_duplicates_first_wins_ranks_dense(eng):
    m = Mirror(eng, 7)
    n = 2000
    ids = R.client_keys(np.arange(n) + 10)
    for a, b in [(3, 4), (10, 200), (20, 700), (255, 256), (63, 64), (5, 1999)]:
        ids[b] = ids[a]
    ids[320:384] = ids[77]
    ids[900] = R.with_cat(ids[900:901], R.CAT_GEO_CLIENT)[0]
    m.open(ids, np.arange(n, dtype=np.uint32))
    m.open(ids[:100], np.zeros(100, np.uint32))            # all reconnects; the round robin does not move
    m.open(R.client_keys(np.arange(20) + (1 << 30)), np.arange(20, dtype=np.uint32))    # ... and goes on across batches


def test_close_drop_expire_edges(eng):
    m, ids, rng = opened(eng, 300, seed=9, close_some=False)
    assert m.drop(1 << 40) == 0                            # 0 due
    m.close(ids[:100], 1000)
    m.close(ids[50:150], 1200, np.arange(100, dtype=np.uint32))   # half already disconnected: untouched
    assert m.drop(1499) == 0
    assert m.drop(1500) == 100                             # exactly at the timeout: the first close's, not the second's
    assert m.drop(1 << 40, cap=49) == 50                   # one short: nothing changes
    assert m.drop(1 << 40, cap=50) == 50                   # all due
    t, s, ss, ttl = batch(rng, 5000, ids[150:])
    m.deliver(t, s, ss, 7000, ttl)
    assert m.routes_expire(7000 + 1899) == 0
    n_routes = m.t.count()[1]
    assert n_routes > 0 and m.routes_expire(7000 + 1900) == n_routes


def test_tombstone_rebuild_then_growth(eng):
    """200 open / close / drop cycles at constant capacity, then growth."""
    m = Mirror(eng, 3, 10, 10, hint=64)
    rng = np.random.default_rng(5)
    for c in range(200):
        ids = R.client_keys(rng.choice(1 << 30, 20, replace=False) + 1)
        m.e.gateway_open(ids, np.arange(20, dtype=np.uint32)); m.t.open(ids, np.arange(20, dtype=np.uint32))
        m.e.gateway_close(ids, c); m.t.close(ids, c)
        got = m.e.gateway_drop(c + 10, 64); want = m.t.drop(c + 10)
        assert len(got[1]) == want[3] == 20
    assert m.verify() == (64, 64)
    ids = R.client_keys(np.arange(1000) + 1)
    assert m.open(ids, np.arange(1000, dtype=np.uint32))[0] >= 2048
    m.see(ids)
    m.verify()


def test_wrapped_chains_at_load(eng):
    """Client keys sharing the table's last home: chains that wrap, in a table at load 0.75."""
    cap = 64
    m = Mirror(eng, 3, hint=cap)
    cand = R.client_keys(np.arange(1, 200000))
    homes = CK.home_slot_np(cand, cap)
    chain = cand[homes == np.uint64(cap - 8)][:20]          # 20 keys from the last home: 12 wrap
    other = cand[homes != np.uint64(cap - 8)][:28]
    assert len(chain) == 20
    m.open(np.concatenate([chain, other]), np.arange(48, dtype=np.uint32))
    assert eng.gateway_count()[2] == cap
    m.close(chain[::2], 50)
    assert m.drop(1 << 40) == 10                           # tombstones inside the wrapped chain
    rng = np.random.default_rng(1)
    m.deliver(chain[rng.integers(0, 20, 700)], chain[rng.integers(0, 20, 700)], np.arange(700, dtype=np.uint32), 60)
    m.open(chain, np.arange(20, dtype=np.uint32) + 500)    # reuses the tombstones


def test_route_table_wrapped_chains_at_load(eng):
    """The route upsert on a 64-slot table filled to 0.75 by batches that fit the host's bound (one new route a
    message): 20 senders sharing the table's last home, so their chain wraps; tombstones; a rebuild in place."""
    cap = 64
    m = Mirror(eng, 3, 500, 30, hint=cap)
    cand = R.client_keys(np.arange(1, 200000))
    homes = CK.home_slot_np(cand, cap)
    chain = cand[homes == np.uint64(cap - 8)][:20]
    other = cand[homes != np.uint64(cap - 8)][:28]
    me = R.client_keys([1 << 33])
    m.open(me, [1])
    tgt = lambda k: np.repeat(me, k, axis=0)
    a = np.concatenate([chain[:10], other[:14]])
    b = np.concatenate([chain[10:], other[14:]])
    m.deliver(tgt(24), a, np.arange(24, dtype=np.uint32), 10)             # twins of one home claimed in one batch
    m.deliver(tgt(24), b, np.arange(24, dtype=np.uint32) + 100, 20)       # ... and joined behind the first ten
    assert eng.gateway_count() == (1, 48, cap, cap)                       # load 0.75, nothing grew
    st, silo, idx, _ = m.ingress(np.concatenate([chain, other]), tgt(48), np.ones(48, np.uint8), None, False)
    assert (st == R.GWIN_DIRECT).all() and len(idx) == 0
    assert m.routes_expire(40) == 24                                      # tombstones inside the wrapped chain
    dup = np.concatenate([chain[:10], chain[:10], other[:4]])             # reuse, each sender twice: the last stands
    m.deliver(tgt(24), dup, np.arange(24, dtype=np.uint32) + 200, 50)     # past the bound: rebuilt at 64 slots
    assert eng.gateway_count() == (1, 38, cap, cap)
    m.deliver(tgt(10), chain[10:], np.arange(10, dtype=np.uint32) + 300, 60)   # overwrites along the wrapped chain
    assert eng.gateway_count()[3] == cap


# ---- ingress, the fused send stage -------------------------------------------------------------------------

def _routed_engine(gd, eng, n_grains=2000):
    """A small directory in ring mode D on the engine: (registered keys, silo hashes, rng, oracle route of keys)."""
    import oracle as o
    rng = np.random.default_rng(11)
    silos = o.bench_silos(8)
    spec = o.ring_spec(silos, "D")
    keys = o.grain_keys(77, np.arange(1, n_grains + 1))
    acts, host = np.arange(n_grains, dtype=np.uint32), rng.integers(0, 8, n_grains).astype(np.uint32)
    eng.ring_set_silos("D", [(s.ip, s.port, s.gen) for s in silos])
    eng.upsert(keys, acts, host)
    hashes = np.array([s.consistent_hash() for s in silos], np.int32)
    eng.send_configure(hashes, 4)
    oracle = lambda k: o.route_batch_np(R.keys(k), spec, o.DirectoryArrays(keys, acts, host), my_silo=0,
                                        seed_silo=0xFFFFFFFF)
    return keys, hashes, rng, oracle


@pytest.mark.parametrize("n", [0, 1, 65, TILE + 1, 20001])
def test_ingress_shapes_and_route_chain(gd, eng, n):
    import torch
    keys, hashes, rng, oracle = _routed_engine(gd, eng)
    m, ids, _ = opened(eng, 40, seed=n)
    t, s, ss, ttl = batch(rng, 3000, ids)
    m.deliver(t, s, ss, 100, ttl)                          # records routes, some with no gateway
    pool = np.concatenate([ids[:12], keys[:200], R.with_cat(ids[:3], R.CAT_GEO_CLIENT), R.with_cat(keys[:5], 1)])
    target = pool[rng.integers(0, len(pool), n)]
    sending = np.concatenate([ids, keys[:40], R.with_cat(ids[:3], R.CAT_GEO_CLIENT)])[rng.integers(0, 83, n)]
    d = rng.choice(np.array([0, 1, 1, 1, 2, 0xFF], np.uint8), n)
    ttl = batch(rng, n, ids)[3]
    want = m.t.ingress(target, sending, d, ttl[:n], False, 0)
    _eq(eng.gateway_ingress(target, sending, d, ttl[:n]), want, ("status", "silo", "route_idx", "route_keys"))
    if n >= 20001:
        assert set(want[0]) == {0, 1, 2, 3, 5}
    _eq(eng.gateway_ingress(target, sending, d, ttl[:n], overloaded=True),
        m.t.ingress(target, sending, d, ttl[:n], True, 0), ("status", "silo", "route_idx", "route_keys"))
    if n == 0:
        return
    # the device form chained into gd_route_device on d_route_keys, against the route of the same keys
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    z = lambda b: torch.full((b + PAD,), 0xAB, dtype=torch.uint8, device=dev)
    d_t, d_s, d_d, d_ttl = up(target), up(sending), up(d), up(ttl[:n])
    d_st, d_silo, d_idx, d_n, d_keys = z(n), z(4 * n), z(4 * n), z(4), z(24 * n)
    r_silo, r_act, r_st = z(4 * n), z(4 * n), z(n)
    torch.cuda.synchronize()
    eng.gateway_ingress_device(d_t.data_ptr(), d_s.data_ptr(), d_d.data_ptr(), d_ttl.data_ptr(), n, 0,
                            d_st.data_ptr(), d_silo.data_ptr(), d_idx.data_ptr(), d_n.data_ptr(), d_keys.data_ptr())
    k = len(want[2])
    eng.route_device(d_keys.data_ptr(), k, r_silo.data_ptr(), r_act.data_ptr(), r_st.data_ptr())
    eng.synchronize()
    host = lambda x, dt, c: x.cpu().numpy()[: c * np.dtype(dt).itemsize].view(dt)
    assert host(d_n, np.uint32, 1)[0] == k
    _eq((host(d_st, np.uint8, n), host(d_silo, np.uint32, n), host(d_idx, np.uint32, k),
         host(d_keys, np.uint64, 3 * k).reshape(-1, 3)), want, ("status", "silo", "route_idx", "route_keys"))
    for x, used in ((d_st, n), (d_silo, 4 * n), (d_idx, 4 * k), (d_keys, 24 * k)):
        assert (x.cpu().numpy()[used:used + PAD] == 0xAB).all()        # nothing past the end
    ow = oracle(want[3])
    for got, w in zip((host(r_st, np.uint8, k), host(r_silo, np.uint32, k), host(r_act, np.uint32, k)), ow):
        np.testing.assert_array_equal(got, w)


@pytest.mark.parametrize("n,n_senders,n_queues", [(0, 3, 4), (65, 3, 4), (3 * TILE + 17, 64, 4), (TILE + 1, 64, 1024), (20001, 1016, 1024),
                                                  (20001, 1024, 1024)])   # 1,092 / 2,044 buckets: the small partition's last
def test_send_queues_after_route_is_the_composition(gd, eng, n, n_senders, n_queues):
    import torch
    keys, hashes, rng, oracle = _routed_engine(gd, eng)
    eng.send_configure(hashes, n_queues)
    m, ids, _ = opened(eng, 40, n_senders, seed=n)
    # the clients are in the directory at this silo (ClientObserverRegistrar): without the proxy check they loop back
    eng.upsert(ids, np.arange(40, dtype=np.uint32) + 5000, np.zeros(40, np.uint32))
    pool = np.concatenate([ids, keys[:400], R.client_keys([1 << 41, 1 << 42]), R.with_cat(ids[:3], R.CAT_GEO_CLIENT)])
    target = pool[rng.integers(0, len(pool), n)]
    sending = np.concatenate([ids[:10], keys[:30]])[rng.integers(0, 40, n)]
    ssilo = rng.integers(0, 8, n).astype(np.uint32)
    _, _, cat, ttl = S.mixed_batch(rng, n, 8, 0)
    rst, rsilo, _ = eng.route(target) if n else (np.zeros(0, np.uint8), np.zeros(0, np.uint32), None)
    # the fused form == gd_gateway_deliver on the messages the send rule does not hold or expire, then
    # gd_send_queues on the not-proxied rest (the literal loop is that composition)
    want = m.t.send_queues(target, sending, ssilo, rsilo, 300, rst, cat, ttl, hashes, n_queues, 0)
    if n >= 20001:
        assert set(want[0]) == {S.SEND_QUEUED, S.SEND_LOOPBACK, S.SEND_EXPIRED, S.SEND_HELD, R.SEND_PROXIED}
    m.see(target, sending)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    z = lambda b: torch.full((b + PAD,), 0xAB, dtype=torch.uint8, device=dev)
    B = n_queues + n_senders + 4
    d_keys, d_s, d_ss, d_cat, d_ttl = up(target), up(sending), up(ssilo), up(cat), up(ttl)
    d_silo, d_act, d_rst = z(4 * n), z(4 * n), z(n)
    d_st, d_q, d_h, d_perm, d_off = z(n), z(4 * n), z(4 * n), z(4 * n), z(4 * (B + 1))
    torch.cuda.synchronize()
    if n:
        eng.route_device(d_keys.data_ptr(), n, d_silo.data_ptr(), d_act.data_ptr(), d_rst.data_ptr())
    # the same device arrays through gd_send_queues_device before and after: unchanged in every output
    plain = [[z(n), z(4 * n), z(4 * n), z(4 * (n_queues + 5))] for _ in range(2)]
    send_plain = lambda o: eng.send_queues_device(d_silo.data_ptr(), d_rst.data_ptr(), d_cat.data_ptr(), d_ttl.data_ptr(), n,
                                                  *[x.data_ptr() for x in o])
    send_plain(plain[0])
    eng.gateway_send_queues_device(d_keys.data_ptr(), d_s.data_ptr(), d_ss.data_ptr(), d_silo.data_ptr(),
                            d_rst.data_ptr(), d_cat.data_ptr(), d_ttl.data_ptr(), n, 300, d_st.data_ptr(), d_q.data_ptr(),
                            d_h.data_ptr(), d_perm.data_ptr(), d_off.data_ptr())
    eng.synchronize()
    host = lambda x, dt, c: x.cpu().numpy()[: c * np.dtype(dt).itemsize].view(dt)
    _eq((host(d_st, np.uint8, n), host(d_q, np.uint32, n), host(d_h, np.uint32, n), host(d_perm, np.uint32, n),
         host(d_off, np.uint32, B + 1)), want, ("send_status", "queue", "handle", "perm", "offsets"))
    for x, used in ((d_st, n), (d_q, 4 * n), (d_h, 4 * n), (d_perm, 4 * n), (d_off, 4 * (B + 1))):
        assert (x.cpu().numpy()[used:used + PAD] == 0xAB).all()
    m.verify()
    # the host form on a second mirror state gives the same; gd_send_queues itself is unchanged by all this
    want2 = m.t.send_queues(target, sending, ssilo, rsilo, 400, rst, cat, ttl, hashes, n_queues, 0)
    _eq(eng.gateway_send_queues(target, sending, ssilo, rsilo, 400, rst, cat, ttl), want2,
        ("send_status", "queue", "handle", "perm", "offsets"))
    m.verify()
    send_plain(plain[1])
    eng.synchronize()
    ref = S.send_queues_np(rsilo, rst, cat, ttl, hashes, n_queues, 0)
    for o in plain:
        _eq((host(o[0], np.uint8, n), host(o[1], np.uint32, n), host(o[2], np.uint32, n),
             host(o[3], np.uint32, n_queues + 5)), ref, ("send_status", "queue", "perm", "offsets"))
        assert all((x.cpu().numpy()[-PAD:] == 0xAB).all() for x in o)


# ---- device forms, prefilled outputs, errors ---------------------------------------------------------------

def test_device_forms_write_everything_and_nothing_more(gd, eng):
    import torch
    m = Mirror(eng, 5, hint=8192)
    rng = np.random.default_rng(21)
    n = TILE + 1
    ids = R.client_keys(rng.choice(1 << 24, 700, replace=False) + 1)
    opn = np.concatenate([ids, ids[:300], R.with_cat(ids[:5], 3)])[rng.permutation(1005)]
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    z = lambda b: torch.full((b + PAD,), 0xAB, dtype=torch.uint8, device=dev)
    host = lambda x, dt, c: x.cpu().numpy()[: c * np.dtype(dt).itemsize].view(dt)

    def tail_ok(pairs):
        for x, used in pairs:
            assert (x.cpu().numpy()[used:used + PAD] == 0xAB).all()

    k = len(opn)
    hd = np.arange(k, dtype=np.uint32)
    d_ids, d_hd = up(opn), up(hd)
    o = [z(4 * k), z(4 * k), z(k), z(4 * k)]
    torch.cuda.synchronize()
    eng.gateway_open_device(d_ids.data_ptr(), d_hd.data_ptr(), k, *[x.data_ptr() for x in o])
    eng.synchronize()
    _eq((host(o[0], np.uint32, k), host(o[1], np.uint32, k), host(o[2], np.uint8, k), host(o[3], np.uint32, k)),
        m.t.open(opn, hd), ("handle", "sender", "new", "pending"))
    tail_ok(zip(o, (4 * k, 4 * k, k, 4 * k)))
    m.see(opn)
    m.verify()
    cl = ids[::2]
    d_cl, d_pl, d_f = up(cl), up(np.arange(len(cl), dtype=np.uint32)), z(len(cl))
    torch.cuda.synchronize()
    eng.gateway_close_device(d_cl.data_ptr(), d_pl.data_ptr(), len(cl), 1000, d_f.data_ptr())
    eng.synchronize()
    _eq((host(d_f, np.uint8, len(cl)),), (m.t.close(cl, 1000, np.arange(len(cl), dtype=np.uint32)),), ("found",))
    tail_ok([(d_f, len(cl))])
    m.verify()
    t, s, ss, ttl = batch(rng, n, ids)
    d = [up(t), up(s), up(ss), up(ttl)]
    o = [z(n), z(4 * n), z(4 * n), z(4 * n), z(4 * 7)]
    torch.cuda.synchronize()
    eng.gateway_deliver_device(*[x.data_ptr() for x in d], n, 1500, *[x.data_ptr() for x in o])
    eng.synchronize()
    m.see(t, s)
    _eq((host(o[0], np.uint8, n), host(o[1], np.uint32, n), host(o[2], np.uint32, n), host(o[3], np.uint32, n),
         host(o[4], np.uint32, 7)), m.t.deliver(t, s, ss, 1500, ttl), ("status", "handle", "sender", "perm", "offsets"))
    tail_ok(zip(o, (n, 4 * n, 4 * n, 4 * n, 28)))
    m.verify()
    # lookup, drop (cap one short, then enough), routes_expire
    L = [z(4 * k), z(4 * k), z(k), z(8 * k), z(4 * k), z(k), z(4 * k), z(8 * k), z(k)]
    d_n, d_id, d_h, d_p = z(4), z(24 * 400), z(4 * 400), z(4 * 400)
    torch.cuda.synchronize()
    eng.gateway_lookup_device(d_ids.data_ptr(), k, *[x.data_ptr() for x in L])
    eng.gateway_drop_device(1 << 40, 349, d_id.data_ptr(), d_h.data_ptr(), d_p.data_ptr(), d_n.data_ptr())
    eng.synchronize()
    dts = (np.uint32, np.uint32, np.uint8, np.int64, np.uint32, np.uint8, np.uint32, np.int64, np.uint8)
    _eq(tuple(host(x, dt, k) for x, dt in zip(L, dts)), m.t.lookup(opn), R.LOOKUP_NAMES)
    tail_ok((x, k * np.dtype(dt).itemsize) for x, dt in zip(L, dts))
    assert host(d_n, np.uint32, 1)[0] == 350 and (d_id.cpu().numpy() == 0xAB).all()
    m.verify()
    eng.gateway_drop_device(1 << 40, 350, d_id.data_ptr(), d_h.data_ptr(), d_p.data_ptr(), d_n.data_ptr())
    eng.gateway_routes_expire_device(1 << 40, d_n.data_ptr() + 0)
    eng.synchronize()
    want = m.t.drop(1 << 40)
    got = (host(d_id, np.uint64, 3 * 350).reshape(-1, 3), host(d_h, np.uint32, 350), host(d_p, np.uint32, 350))
    srt = np.lexsort((got[0][:, 2], got[0][:, 1], got[0][:, 0]))
    _eq(tuple(a[srt] for a in got), want[:3], ("id", "handle", "pending"))
    tail_ok([(d_id, 24 * 350), (d_h, 4 * 350), (d_p, 4 * 350)])
    assert host(d_n, np.uint32, 1)[0] == m.t.routes_expire(1 << 40) > 0
    m.verify()


def test_errors_before_configure_and_inside_capture(gd, eng):
    import torch
    ids = R.client_keys([1, 2, 3])
    hd = np.zeros(3, np.uint32)
    calls = [lambda: eng.gateway_clear(), lambda: eng.gateway_count(), lambda: eng.gateway_open(ids, hd),
             lambda: eng.gateway_close(ids, 0), lambda: eng.gateway_drop(0, 4), lambda: eng.gateway_routes_expire(0),
             lambda: eng.gateway_lookup(ids), lambda: eng.gateway_deliver(ids, ids, hd, 0, bucket=False),
             lambda: eng.gateway_ingress(ids, ids),
             lambda: eng.gateway_send_queues(ids, ids, hd, hd, 0, bucket=False)]
    dev = torch.device("cuda:0")
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    p = buf.data_ptr()
    dcalls = [("open", p, p, 3, p, p, p, p), ("close", p, None, 3, 0, p), ("drop", 0, 3, p, p, p, p),
              ("routes_expire", 0, p), ("lookup", p, 3, p, None, None, None, None, None, None, None, None),
              ("deliver", p, p, p, None, 3, 0, p, p, p, None, None),
              ("send_queues", p, p, p, p, None, None, None, 3, 0, p, p, p, None, None),
              ("ingress", p, p, None, None, 3, 0, p, p, None, None, None)]
    dcall = lambda a: getattr(eng, "gateway_%s_device" % a[0])(*a[1:])
    for c in calls + [lambda a=a: dcall(a) for a in dcalls]:
        with pytest.raises(gd.GrainDispatchError) as ei:
            c()
        assert ei.value.code == gd.GD_ESTATE
    for bad in [(0, 1, 1, 0), (1025, 1, 1, 0), (3, -1, 1, 0), (3, 1, -1, 0)]:
        with pytest.raises(gd.GrainDispatchError) as ei:
            eng.gateway_configure(*bad)
        assert ei.value.code == gd.GD_EINVAL
    m = Mirror(eng, 3, hint=1024)
    with pytest.raises(gd.GrainDispatchError) as ei:       # the send stage is not configured
        dcall(dcalls[6])
    assert ei.value.code == gd.GD_ESTATE
    m.open(ids, hd)
    with pytest.raises(gd.GrainDispatchError) as ei:       # n_senders changes while clients are present
        eng.gateway_configure(4, 1, 1, 0)
    assert ei.value.code == gd.GD_EINVAL
    eng.gateway_configure(3, 500, 1900, 4096)              # the options may change, the tables grow
    assert m.verify() == (4096, 4096)
    # one of perm / offsets, route_idx / n_route without the other
    for a in [("deliver", p, p, p, None, 3, 0, p, p, p, p, None), ("ingress", p, p, None, None, 3, 0, p, p, p, None, None),
              ("ingress", p, p, None, None, 3, 0, p, p, None, None, p)]:
        with pytest.raises(gd.GrainDispatchError) as ei:
            dcall(a)
        assert ei.value.code == gd.GD_EINVAL
    # inside a stream capture: every host form is refused; the device forms enqueue (their room is known from the
    # host's bound here) and the replayed graph applies them
    d_ids, d_hd = torch.from_numpy(R.client_keys([7, 8, 9]).view(np.int64).reshape(-1).copy()).to(dev), buf[:12]
    outs = [torch.zeros(64, dtype=torch.uint8, device=dev) for _ in range(12)]
    eng.gateway_open_device(d_ids.data_ptr(), d_hd.data_ptr(), 0, p, p, p, p)
    eng.gateway_deliver_device(d_ids.data_ptr(), d_ids.data_ptr(), None, None, 3, 5, outs[4].data_ptr(),
                            outs[5].data_ptr(), outs[6].data_ptr(), outs[7].data_ptr(), outs[8].data_ptr())   # warms the scratch
    eng.gateway_open_device(d_ids.data_ptr(), d_hd.data_ptr(), 3, *[x.data_ptr() for x in outs[:4]])
    eng.synchronize()
    m.t.deliver(R.client_keys([7, 8, 9]), R.client_keys([7, 8, 9]), None, 5)
    m.t.open(R.client_keys([7, 8, 9]), np.zeros(3, np.uint32))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.set_stream(s.cuda_stream)
    g = torch.cuda.CUDAGraph()
    codes = []
    with torch.cuda.graph(g, stream=s):
        outs[11].add_(1)
        for c in calls:
            with pytest.raises(gd.GrainDispatchError) as ei:
                c()
            codes.append(ei.value.code)
        eng.gateway_close_device(d_ids.data_ptr(), None, 3, 77, outs[9].data_ptr())
        eng.gateway_deliver_device(d_ids.data_ptr(), d_ids.data_ptr(), None, None, 3, 88, outs[4].data_ptr(),
                                outs[5].data_ptr(), outs[6].data_ptr(), None, None)
        eng.gateway_ingress_device(d_ids.data_ptr(), d_ids.data_ptr(), None, None, 3, 0, outs[10].data_ptr(),
                                None, None, None, None)
        eng.gateway_lookup_device(d_ids.data_ptr(), 3, None, None, None, None, outs[3].data_ptr(), None, None,
                                None, None)
    eng.set_stream(None)
    assert codes == [gd.GD_ESTATE] * len(calls)
    g.replay()
    torch.cuda.synchronize()
    m.t.close(R.client_keys([7, 8, 9]), 77)
    want = m.t.deliver(R.client_keys([7, 8, 9]), R.client_keys([7, 8, 9]), None, 88)
    assert list(outs[4].cpu().numpy()[:3]) == list(want[0]) == [R.GW_PENDING] * 3
    assert list(outs[3].cpu().numpy()[:12].view(np.uint32)) == [1, 1, 1]
    m.see(R.client_keys([7, 8, 9]))
    m.verify()


def test_every_device_form_inside_a_capture(gd, eng):
    """Every device form captured into one graph -- with perm / offsets, route_idx / n_route / route_keys and the
    scans of open, drop and ingress -- and the replay compared with the loop; an open or a deliver whose room the
    host's bound cannot tell is GD_ESTATE inside the capture (the replay then shows only the captured calls)."""
    import torch
    rng = np.random.default_rng(77)
    hashes = (np.arange(8, dtype=np.int32) * 7919 + 1).astype(np.int32)
    eng.send_configure(hashes, 4)
    m = Mirror(eng, 3, 500, 1900, hint=4096)
    K = R.client_keys
    m.open(K([1, 2, 3, 4, 5, 6]), np.arange(6, dtype=np.uint32) + 10)
    m.close(K([1, 2]), 10, [4, 5])
    n = 300
    grains = R.keys(np.c_[np.zeros(10, np.uint64), np.arange(1, 11, dtype=np.uint64), np.full(10, (3 << 56) | 77, np.uint64)])
    pool = np.concatenate([K([1, 2, 3, 4, 5, 6, 20, 21, 99]), grains, R.with_cat(K([1]), R.CAT_GEO_CLIENT),
                           R.with_cat(grains[:1], R.CAT_SYSTEM_TARGET)])
    target, target2 = pool[rng.integers(0, len(pool), n)], pool[rng.integers(0, len(pool), n)]
    spool = np.concatenate([K([1, 2, 3, 4, 5, 6, 50, 51]), grains[:4]])
    sending = spool[rng.integers(0, len(spool), n)]
    ssilo, silo = rng.integers(0, 8, n).astype(np.uint32), rng.integers(0, 8, n).astype(np.uint32)
    _, _, cat, ttl = S.mixed_batch(rng, n, 8, 0)
    direction = rng.choice(np.array([0, 1, 1, 1], np.uint8), n)
    o_ids, o_hd = np.concatenate([K([3, 4, 20, 21, 20]), grains[:1]]), np.arange(6, dtype=np.uint32) + 70
    c_ids, c_pl = K([3, 20]), np.array([7, 8], np.uint32)
    every = np.unique(np.concatenate([pool, spool, o_ids]), axis=0)
    m.see(every)
    L = len(every)

    def loop(t):
        return {"open": t.open(o_ids, o_hd), "close": (t.close(c_ids, 900, c_pl),),
                "deliver": t.deliver(target, sending, ssilo, 950, ttl),
                "send": t.send_queues(target, sending, ssilo, silo, 960, None, cat, ttl, hashes, 4, 0),
                "ingress": t.ingress(target2, sending, direction, ttl, False, 0), "drop": t.drop(1000),
                "expire": t.routes_expire(2855), "lookup": t.lookup(every)}

    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    z = lambda b: torch.full((b + PAD,), 0xAB, dtype=torch.uint8, device=dev)
    P = lambda xs: [x.data_ptr() for x in xs]
    d = {k: up(v) for k, v in dict(t=target, t2=target2, s=sending, ss=ssilo, silo=silo, cat=cat, ttl=ttl, dir=direction,
                                   oi=o_ids, oh=o_hd, ci=c_ids, cp=c_pl, ev=every).items()}
    out = {"open": [z(24), z(24), z(6), z(24)], "close": [z(2)],
           "deliver": [z(n), z(4 * n), z(4 * n), z(4 * n), z(4 * 5)],
           "send": [z(n), z(4 * n), z(4 * n), z(4 * n), z(4 * 12)],
           "ingress": [z(n), z(4 * n), z(4 * n), z(4), z(24 * n)],
           "drop": [z(24 * 16), z(4 * 16), z(4 * 16), z(4)], "expire": [z(4)],
           "lookup": [z(4 * L), z(4 * L), z(L), z(8 * L), z(4 * L), z(L), z(4 * L), z(8 * L), z(L)]}
    big = torch.zeros(3200 * 24, dtype=torch.uint8, device=dev)

    def enqueue():
        eng.gateway_open_device(d["oi"].data_ptr(), d["oh"].data_ptr(), 6, *P(out["open"]))
        eng.gateway_close_device(d["ci"].data_ptr(), d["cp"].data_ptr(), 2, 900, *P(out["close"]))
        eng.gateway_deliver_device(d["t"].data_ptr(), d["s"].data_ptr(), d["ss"].data_ptr(), d["ttl"].data_ptr(), n, 950,
                                   *P(out["deliver"]))
        eng.gateway_send_queues_device(d["t"].data_ptr(), d["s"].data_ptr(), d["ss"].data_ptr(), d["silo"].data_ptr(), None,
                                       d["cat"].data_ptr(), d["ttl"].data_ptr(), n, 960, *P(out["send"]))
        eng.gateway_ingress_device(d["t2"].data_ptr(), d["s"].data_ptr(), d["dir"].data_ptr(), d["ttl"].data_ptr(), n, False,
                                   *P(out["ingress"]))
        eng.gateway_drop_device(1000, 16, *P(out["drop"]))
        eng.gateway_routes_expire_device(2855, out["expire"][0].data_ptr())
        eng.gateway_lookup_device(d["ev"].data_ptr(), L, *P(out["lookup"]))

    host = lambda x, dt, c: x.cpu().numpy()[: c * np.dtype(dt).itemsize].view(dt)

    def check(want):
        u8, u32, i64 = np.uint8, np.uint32, np.int64
        o = out["open"]
        _eq((host(o[0], u32, 6), host(o[1], u32, 6), host(o[2], u8, 6), host(o[3], u32, 6)), want["open"], "hsnp")
        _eq((host(out["close"][0], u8, 2),), want["close"], "f")
        o = out["deliver"]
        _eq((host(o[0], u8, n), host(o[1], u32, n), host(o[2], u32, n), host(o[3], u32, n), host(o[4], u32, 5)),
            want["deliver"], ("status", "handle", "sender", "perm", "offsets"))
        o = out["send"]
        _eq((host(o[0], u8, n), host(o[1], u32, n), host(o[2], u32, n), host(o[3], u32, n), host(o[4], u32, 12)),
            want["send"], ("send_status", "queue", "handle", "perm", "offsets"))
        o, k = out["ingress"], len(want["ingress"][2])
        assert host(o[3], u32, 1)[0] == k
        _eq((host(o[0], u8, n), host(o[1], u32, n), host(o[2], u32, k), host(o[4], np.uint64, 3 * k).reshape(-1, 3)),
            want["ingress"], ("status", "silo", "route_idx", "route_keys"))
        o, k = out["drop"], want["drop"][3]
        assert host(o[3], u32, 1)[0] == k
        got = (host(o[0], np.uint64, 3 * k).reshape(-1, 3), host(o[1], u32, k), host(o[2], u32, k))
        srt = np.lexsort((got[0][:, 2], got[0][:, 1], got[0][:, 0]))
        _eq(tuple(a[srt] for a in got), want["drop"][:3], ("id", "handle", "pending"))
        assert host(out["expire"][0], u32, 1)[0] == want["expire"]
        dts = (u32, u32, u8, i64, u32, u8, u32, i64, u8)
        _eq(tuple(host(x, dt, L) for x, dt in zip(out["lookup"], dts)), want["lookup"], R.LOOKUP_NAMES)
        assert all((x.cpu().numpy()[-PAD:] == 0xAB).all() for xs in out.values() for x in xs)
        return k

    torch.cuda.synchronize()
    enqueue()                                              # eagerly once: the scratch has its sizes, the loop follows
    eng.synchronize()
    assert check(loop(m.t)) == 2                           # clients 1 and 2 were due
    m.verify()
    m.close(K([5]), 100)                                   # so the replay's drop has a client due as well
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.set_stream(s.cuda_stream)
    g = torch.cuda.CUDAGraph()
    codes = []
    with torch.cuda.graph(g, stream=s):
        big.add_(0)                                        # the capture holds one node of the test's own
        for call in (lambda: eng.gateway_open_device(big.data_ptr(), big.data_ptr(), 3200),
                     lambda: eng.gateway_deliver_device(big.data_ptr(), big.data_ptr(), None, None, 3200, 1,
                                                        out["deliver"][0].data_ptr(), None, big.data_ptr())):
            with pytest.raises(gd.GrainDispatchError) as ei:   # 3,200 > 0.75 * 4,096: the counters would be read
                call()
            codes.append(ei.value.code)
        enqueue()
    eng.set_stream(None)
    assert codes == [gd.GD_ESTATE] * 2
    for xs in out.values():
        for x in xs:
            x.fill_(0xAB)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert check(loop(m.t)) == 1                           # client 5
    m.verify()
