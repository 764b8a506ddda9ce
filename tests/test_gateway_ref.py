"""The gateway reference against itself: the literal loop (_gateway_ref.Gateway) == the numpy form
(GatewayNp) bit for bit over mixed lifecycles, one hand-written case a rule, and the fused send form == _sendq_ref
composed with the gateway loop.  No GPU."""
import numpy as np
import pytest

import _gateway_ref as R
import _sendq_ref as S

K = R.client_keys
GRAIN = R.keys([[0, 5, (3 << 56) | 77]])
LK = lambda g, ids: dict(zip(R.LOOKUP_NAMES, g.lookup(ids)))


def _same(a, b, what):
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype, what
        np.testing.assert_array_equal(x, y, err_msg=what)


@pytest.mark.parametrize("seed", range(12))
def test_loop_equals_numpy_over_lifecycles(seed):
    loop, vec = R.Gateway(3, *R.LIFECYCLE_TIMEOUTS), R.GatewayNp(3, *R.LIFECYCLE_TIMEOUTS)
    seen = {"deliver": set(), "ingress": set(), "new": set()}
    dropped = expired = 0
    every = np.zeros((0, 3), np.uint64)
    for call, args in R.lifecycle(np.random.default_rng(seed)):
        a, b = getattr(loop, call)(*args), getattr(vec, call)(*args)
        _same(a, b, call)
        assert loop.count() == vec.count()
        if call in ("deliver", "ingress"):
            seen[call] |= set(a[0].tolist())
            every = np.unique(np.concatenate([every, R.keys(args[0]), R.keys(args[1])]), axis=0)
        if call == "open":
            seen["new"] |= set(a[2].tolist())
            every = np.unique(np.concatenate([every, R.keys(args[0])]), axis=0)
        dropped += a[3] if call == "drop" and (args[1] is None or a[3] <= args[1]) else 0
        expired += a if call == "routes_expire" else 0
        _same(loop.lookup(every), vec.lookup(every), "state after " + call)
    # the generator covers what it claims: no test passes on an empty class of messages
    assert seen["deliver"] == {R.GW_NOT_PROXIED, R.GW_SEND, R.GW_PENDING, R.GW_EXPIRED, R.GW_GEO_CLIENT}
    assert seen["ingress"] == {R.GWIN_REROUTE, R.GWIN_DIRECT, R.GWIN_SYSTEM_TARGET, R.GWIN_EXPIRED, R.GWIN_TOO_BUSY,
                               R.GWIN_GEO_CLIENT}
    assert seen["new"] == {0, 1, R.GW_NOT_CLIENT}
    assert dropped > 0 and expired > 0


@pytest.mark.parametrize("seed", range(10))
def test_fused_send_is_sendq_composed_with_the_gateway_loop(seed):
    rng = np.random.default_rng(seed)
    n, n_silos, nq, my = 3000, 9, 5, 2
    sh = S.hashes_with_edges(rng, n_silos)
    ids = K(rng.choice(1 << 20, 30, replace=False) + 1)
    fused, vec, comp = R.Gateway(4, 10, 10), R.GatewayNp(4, 10, 10), R.Gateway(4, 10, 10)
    for g in (fused, vec, comp):
        g.open(ids, np.arange(30, dtype=np.uint32))
        g.close(ids[::2], 5)
    silo, rs, cat, ttl = S.mixed_batch(rng, n, n_silos, my, sh)
    pool = np.concatenate([ids, K([1 << 30, 1 << 31]), np.repeat(GRAIN, 30, axis=0), R.with_cat(ids[:3], R.CAT_GEO_CLIENT)])
    target = pool[rng.integers(0, len(pool), n)]
    sending = np.concatenate([ids[:8], GRAIN])[rng.integers(0, 9, n)]
    ssilo = rng.integers(0, n_silos, n).astype(np.uint32)
    got = fused.send_queues(target, sending, ssilo, silo, 50, rs, cat, ttl, sh, nq, my)
    _same(got, vec.send_queues(target, sending, ssilo, silo, 50, rs, cat, ttl, sh, nq, my), "fused loop == numpy")
    # the composition: the send rule alone, deliver on what it neither holds nor expires, the rest keeps its bucket
    st, q, _, _ = S.send_queues_loop(silo, rs, cat, ttl, sh, nq, my)
    cons = ~np.isin(st, (S.SEND_HELD, S.SEND_EXPIRED))
    g_st, g_h, g_sd, _, _ = comp.deliver(target[cons], sending[cons], ssilo[cons], 50, None)
    prox = np.isin(g_st, (R.GW_SEND, R.GW_PENDING))
    ci = np.flatnonzero(cons)[prox]
    hd = np.full(n, R.NO_HANDLE, np.uint32)
    st[ci], q[ci], hd[ci] = R.SEND_PROXIED, nq + 4 + g_sd[prox], g_h[prox]
    perm, off = R._partition(q, nq + 4 + 4)
    _same(got, (st, q, hd, perm, off), "fused == composition")
    every = np.unique(np.concatenate([target, sending]), axis=0)
    _same(fused.lookup(every), comp.lookup(every), "state")
    _same(fused.lookup(every), vec.lookup(every), "state")
    assert set(st.tolist()) == set(range(8))
    # the not-proxied rest is gd_send_queues' own answer, bucket for bucket
    rest = st != R.SEND_PROXIED
    r_st, r_q, _, _ = S.send_queues_np(silo, rs, cat, ttl, sh, nq, my)
    np.testing.assert_array_equal(st[rest], r_st[rest])
    np.testing.assert_array_equal(q[rest], r_q[rest])


@pytest.fixture(params=[R.Gateway, R.GatewayNp])
def G(request):
    return request.param


def test_expiry_runs_before_the_proxy_check(G):
    g = G(2, 10, 10)
    g.open(K([1]), [9])
    g.close(K([1]), 0)
    st, hd, sd, perm, off = g.deliver(K([1, 1]), K([2, 2]), [3, 3], 7, np.array([0, R.TTL_NONE]))
    assert list(st) == [R.GW_EXPIRED, R.GW_PENDING] and list(hd) == [R.NO_HANDLE, 9] and list(sd) == [2, 0]
    assert LK(g, K([1]))["pending"][0] == 1                  # the expired message was not enqueued
    assert list(perm) == [1, 0] and list(off) == [0, 1, 1, 2]


def test_route_recorded_only_when_the_target_was_found(G):
    g = G(2, 10, 10)
    g.open(K([1]), [9])
    g.deliver(np.concatenate([K([5]), GRAIN, K([1]), K([1]), K([1])]),
              np.concatenate([K([20]), K([21]), K([22]), GRAIN, R.with_cat(K([23]), R.CAT_GEO_CLIENT)]),
              [1, 2, 3, 4, 5], 7)
    lk = LK(g, np.concatenate([K([20, 21, 22, 23]), GRAIN]))
    assert list(lk["route_found"]) == [0, 0, 1, 0, 0] and lk["route_silo"][2] == 3 and lk["route_time"][2] == 7
    # AddOrUpdate: the last message of a grain in the batch stands
    g.deliver(K([1, 1, 1]), K([22, 22, 22]), [4, 5, 6], 8)
    lk = LK(g, K([22]))
    assert lk["route_silo"][0] == 6 and lk["route_time"][0] == 8 and g.count() == (1, 1)


def test_a_route_with_no_silo_reroutes(G):
    g = G(2, 10, 10)
    g.open(K([1]), [9])
    g.deliver(K([1, 1]), K([30, 31]), [R.NO_SILO, 4], 1)
    target = np.concatenate([K([30, 31, 32]), R.with_cat(K([31]), R.CAT_GEO_CLIENT), R.with_cat(GRAIN, 1), K([31, 31])])
    sending = np.concatenate([K([1] * 5), GRAIN, K([1])])
    st, silo, idx, rk = g.ingress(target, sending, np.array([1, 1, 1, 1, 1, 1, 0], np.uint8), None, False, 6)
    assert list(st) == [R.GWIN_REROUTE, R.GWIN_DIRECT, R.GWIN_REROUTE, R.GWIN_GEO_CLIENT, R.GWIN_SYSTEM_TARGET,
                        R.GWIN_REROUTE, R.GWIN_REROUTE]
    assert list(silo) == [R.NO_SILO, 4, R.NO_SILO, R.NO_SILO, 6, R.NO_SILO, R.NO_SILO]
    assert list(idx) == [0, 2, 5, 6] and (rk == target[[0, 2, 5, 6]]).all()
    st, silo, idx, _ = g.ingress(target, sending, np.ones(7, np.uint8), np.array([1, 0, 1, 1, 1, 1, 1]), True, 6)
    assert list(st) == [R.GWIN_TOO_BUSY, R.GWIN_EXPIRED] + [R.GWIN_TOO_BUSY] * 5 and len(idx) == 0
    assert (silo == R.NO_SILO).all()


def test_duplicate_id_in_one_open_batch_and_round_robin_across_batches(G):
    g = G(3, 10, 10)
    ids = np.concatenate([K([1, 2, 1, 3]), GRAIN, K([2])])
    oh, sd, nw, pd = g.open(ids, [10, 20, 30, 40, 50, 60])
    assert list(nw) == [1, 1, 0, 1, R.GW_NOT_CLIENT, 0] and list(oh) == [10, 20, 10, 40, R.NO_HANDLE, 20]
    assert list(sd) == [0, 1, 0, 2, 3, 1] and list(pd) == [0] * 6
    oh, sd, nw, pd = g.open(K([4, 1, 5]), [70, 80, 90])       # next_round_robin went on by 3, not by 6
    assert list(sd) == [0, 0, 1] and list(nw) == [1, 0, 1] and list(oh) == [70, 10, 90]


def test_reconnect_drains_once_and_close_of_a_disconnected_client(G):
    g = G(2, 10, 10)
    g.open(K([1]), [9])
    assert list(g.close(K([1, 1, 7]), 5, [3, 4, 5])) == [1, 1, 0]   # the second finds Socket == null: untouched
    lk = LK(g, K([1]))
    assert (lk["connected"][0], lk["since"][0], lk["pending"][0]) == (0, 5, 3)
    assert list(g.close(K([1]), 9, [8])) == [1]
    lk = LK(g, K([1]))
    assert (lk["since"][0], lk["pending"][0]) == (5, 3)
    g.deliver(K([1, 1]), None, None, 6)
    oh, sd, nw, pd = g.open(K([1, 1]), [0, 0])
    assert list(pd) == [5, 0] and list(nw) == [0, 0] and list(oh) == [9, 9]
    lk = LK(g, K([1]))
    assert (lk["connected"][0], lk["since"][0], lk["pending"][0]) == (1, R.I64_MAX, 0)


def test_drop_at_exactly_the_timeout_and_cap_one_short(G):
    g = G(2, 100, 10)
    g.open(K([1, 2, 3]), [7, 8, 9])
    g.close(K([1, 2]), 1000, [4, 5])
    assert g.drop(1099)[3] == 0 and g.count()[0] == 3
    ids, hd, pd, k = g.drop(1100, cap=1)                      # n_out > cap: nothing changed or listed
    assert k == 2 and len(ids) == 0 and g.count()[0] == 3
    ids, hd, pd, k = g.drop(1100, cap=2)
    assert k == 2 and list(hd) == [7, 8] and list(pd) == [4, 5] and g.count()[0] == 1
    assert list(LK(g, K([1, 2, 3]))["found"]) == [0, 0, 1]    # the connected client is never due


def test_routes_expire_at_exactly_the_expiry(G):
    g = G(2, 10, 50)
    g.open(K([1]), [9])
    g.deliver(K([1]), K([2]), [3], 100)
    g.deliver(K([1]), K([4]), [3], 120)
    assert g.routes_expire(149) == 0 and g.routes_expire(150) == 1 and g.count() == (1, 1)
    assert list(LK(g, K([2, 4]))["route_found"]) == [0, 1]
