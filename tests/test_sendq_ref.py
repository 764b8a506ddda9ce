"""CPU tests of the sender-queue stage: the two restatements of
OutboundMessageQueue.SendMessage's queue rule (_sendq_ref.py) against each other and against one
hand-written message per rule, and the argument checks of the gd_send_* / gd_route_send* entry points
that are made before any kernel is launched."""
import ctypes as C

import numpy as np
import pytest

import _sendq_ref as R
from orleans_amd import graindispatch as g


def _same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
        assert x.dtype == y.dtype


@pytest.mark.parametrize("n_queues", [1, 2, 7, 64])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_loop_and_numpy_restatements_agree(seed, n_queues):
    rng = np.random.default_rng(seed)
    n_silos, my_silo = 40, 3
    sh = R.hashes_with_edges(rng, n_silos)
    silo, rs, cat, ttl = R.mixed_batch(rng, 3000, n_silos, my_silo)
    a = R.send_queues_loop(silo, rs, cat, ttl, sh, n_queues, my_silo)
    b = R.send_queues_np(silo, rs, cat, ttl, sh, n_queues, my_silo)
    _same(a, b)
    assert set(np.unique(a[0]).tolist()) == set(range(7))          # every status present
    st, q, perm, off = a
    assert sorted(perm.tolist()) == list(range(len(silo))) and off[-1] == len(silo)
    assert np.all(np.diff(q[perm].astype(np.int64)) >= 0)
    # optional arrays absent: nothing held, no TTL, every message Application
    _same(R.send_queues_loop(silo, None, None, None, sh, n_queues, my_silo),
          R.send_queues_np(silo, None, None, None, sh, n_queues, my_silo))


# One message per row of the rule table.  Silo table: hash[0] = 10, [1] = INT32_MIN, [2] = -7, [3] = 0,
# [4] = INT32_MAX; my silo = 0; 4 queues, so the trailing bucket is 7.
HASH = np.array([10, R.INT32_MIN, -7, 0, (1 << 31) - 1], np.int32)
NQ, MY, TRAIL = 4, 0, 7
ROWS = [
    # (silo, route status, category, ttl) -> (status, bucket)
    ((2, 1, 2, R.TTL_NONE), (R.SEND_HELD, TRAIL)),                # 1: a directory miss is not addressed
    ((2, 4, 2, R.TTL_NONE), (R.SEND_HELD, TRAIL)),                #    KeyExt
    ((2, 7, 2, R.TTL_NONE), (R.SEND_HELD, TRAIL)),                #    multi-activation
    ((2, 6, 0, -5), (R.SEND_HELD, TRAIL)),                        #    undecoded wins over expiry
    ((2, 0, 2, 0), (R.SEND_EXPIRED, TRAIL)),                      # 2: ttl 0
    ((2, 0, 2, -1), (R.SEND_EXPIRED, TRAIL)),                     #    ttl -1
    ((0, 0, 0, -1), (R.SEND_EXPIRED, TRAIL)),                     #    an expired Ping to my silo
    ((R.NO_SILO, 0, 2, 0), (R.SEND_EXPIRED, TRAIL)),              #    expiry before the null-silo check
    ((R.NO_SILO, 0, 2, 5), (R.SEND_NO_SILO, TRAIL)),              # 3
    ((5, 0, 2, 5), (R.SEND_UNKNOWN_SILO, TRAIL)),                 # 4: silo == n_silos
    ((0xFFFFFFFE, 0, 0, 5), (R.SEND_UNKNOWN_SILO, TRAIL)),
    ((0, 0, 2, R.TTL_NONE), (R.SEND_LOOPBACK, 0)),                # 5: ttl GD_TTL_NONE never expires
    ((0, 2, 1, 1), (R.SEND_LOOPBACK, 0)),                         #    a system target on my silo, ttl 1 tick
    ((2, 0, 0, 5), (R.SEND_QUEUED, 1)),                           # 6: Ping
    ((1, 0, 0, 5), (R.SEND_QUEUED, 1)),                           #    Ping to the INT32_MIN silo: no Math.Abs
    ((2, 3, 1, 5), (R.SEND_QUEUED, 2)),                           # 7: System (the membership table grain)
    ((1, 0, 1, 5), (R.SEND_QUEUED, 2)),
    ((1, 0, 2, 5), (R.SEND_THROWS, TRAIL)),                       # 8: Math.Abs(int.MinValue)
    ((1, 0, 7, 5), (R.SEND_THROWS, TRAIL)),                       #    category 7 takes the default: branch
    ((2, 0, 2, 5), (R.SEND_QUEUED, 3 + 7 % 4)),                   # 9: abs(-7) % 4 = 3
    ((2, 0, 7, 5), (R.SEND_QUEUED, 3 + 3)),                       #    category 7
    ((3, 0, 2, 5), (R.SEND_QUEUED, 3)),                           #    hash 0
    ((4, 0, 255, R.TTL_NONE), (R.SEND_QUEUED, 3 + ((1 << 31) - 1) % 4)),
]


def test_one_message_per_rule():
    for args, want in ROWS:
        assert R.send_one(*args, HASH, NQ, MY) == want, args
    silo, rs, cat, ttl = (np.array([r[0][k] for r in ROWS], dt)
                          for k, dt in enumerate((np.uint32, np.uint8, np.uint8, np.int64)))
    for form in (R.send_queues_loop, R.send_queues_np):
        st, q, perm, off = form(silo, rs, cat, ttl, HASH, NQ, MY)
        assert st.tolist() == [w[0] for _, w in ROWS], form.__name__
        assert q.tolist() == [w[1] for _, w in ROWS], form.__name__
        assert off.tolist() == np.concatenate([[0], np.cumsum(np.bincount(q, minlength=NQ + 4))]).tolist()
        for b in range(NQ + 4):                                    # every queue in batch order
            assert perm[off[b]:off[b + 1]].tolist() == [i for i in range(len(q)) if q[i] == b]


def test_math_abs_overflows_only_at_int32_min():
    with pytest.raises(R.MathAbsOverflow):
        R.math_abs(R.INT32_MIN)
    assert R.math_abs(R.INT32_MIN + 1) == (1 << 31) - 1 and R.math_abs(-1) == 1 and R.math_abs(0) == 0
    # numpy's int32 abs wraps silently: the vectorised form must not rely on it
    with np.errstate(over="ignore"):
        assert np.abs(np.array([R.INT32_MIN], np.int32))[0] == R.INT32_MIN
    st, q, _, _ = R.send_queues_np(np.array([0], np.uint32), None, None, None,
                                   np.array([R.INT32_MIN], np.int32), 3, 9)
    assert (int(st[0]), int(q[0])) == (R.SEND_THROWS, 6)


# ---- the C ABI's argument checks (no kernel is launched, no GPU needed) ----------------------------
def _err():
    return g.lib.gd_last_error(None)


def _bufs(n=4):
    return (np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32),
            np.zeros(16, np.uint32))


def test_binding_mirrors_the_header_constants():
    assert (g.SEND_QUEUED, g.SEND_LOOPBACK, g.SEND_EXPIRED, g.SEND_NO_SILO, g.SEND_UNKNOWN_SILO, g.SEND_THROWS,
            g.SEND_HELD) == tuple(range(7)) == (R.SEND_QUEUED, R.SEND_LOOPBACK, R.SEND_EXPIRED, R.SEND_NO_SILO,
                                                R.SEND_UNKNOWN_SILO, R.SEND_THROWS, R.SEND_HELD)
    assert g.TTL_NONE == R.TTL_NONE == np.iinfo(np.int64).max


def test_send_queues_before_configure_is_estate():
    silo, st, q, perm, off = _bufs()
    p = lambda a: a.ctypes.data
    assert g.lib.gd_send_queues(None, p(silo), None, None, None, 4, p(st), p(q), p(perm), p(off)) == g.GD_ESTATE
    assert _err()
    assert g.lib.gd_send_queues_device(None, p(silo), None, None, None, 4, p(st), p(q), None, None) == g.GD_ESTATE
    assert _err()
    keys = np.zeros((4, 3), np.uint64)
    assert g.lib.gd_route_send(None, p(keys), 4, None, None, p(silo), p(q), p(st), p(st), p(q), p(perm),
                               p(off)) == g.GD_ESTATE
    assert _err()


@pytest.mark.parametrize("n_silos,n_queues", [(4, 0), (4, 1025), (0, 4), (65537, 4)])
def test_send_configure_limits_are_einval(n_silos, n_queues):
    sh = np.zeros(max(n_silos, 1), np.int32)
    assert g.lib.gd_send_configure(None, sh.ctypes.data, n_silos, n_queues) == g.GD_EINVAL
    assert _err() and (b"n_queues" in _err() or b"n_silos" in _err())


def test_perm_without_offsets_is_einval():
    silo, st, q, perm, off = _bufs()
    p = lambda a: a.ctypes.data
    for pp, oo in ((p(perm), None), (None, p(off))):
        assert g.lib.gd_send_queues(None, p(silo), None, None, None, 4, p(st), p(q), pp, oo) == g.GD_EINVAL
        assert b"perm and offsets" in _err()
        assert g.lib.gd_send_queues_device(None, p(silo), None, None, None, 4, p(st), p(q), pp, oo) == g.GD_EINVAL
        assert b"perm and offsets" in _err()
        keys = np.zeros((4, 3), np.uint64)
        assert g.lib.gd_route_send_device(None, p(keys), 4, None, None, p(silo), p(q), p(st), p(st), p(q), pp,
                                          oo) == g.GD_EINVAL
        assert b"perm and offsets" in _err()
