"""The turn-admission restatement (_turns_ref.py): the vectorised closed form the kernels follow equals the
literal per-message loop, bit for bit, and the loop gives each rule line of Dispatcher.ReceiveRequest its
outcome on hand-written cases."""
import numpy as np
import pytest

import _turns_ref as R

NAMES = ("turn", "num_running_out", "running_idx", "start_idx", "wait_perm", "wait_offsets")


def _same(a, b):
    for name, x, y in zip(NAMES, a, b):
        assert x.dtype == y.dtype, name
        np.testing.assert_array_equal(x, y, err_msg=name)


def _both(b):
    want = R.turns_loop(b)
    _same(R.turns_np(b), want)
    _same(R.turns_np(b.explicit()), want)
    return want


def _one(flags, msgs, num_running=0, request_count=0, **kw):
    """One context; msgs = [(direction, msg_flags, ttl, forward_count, same_activation)]."""
    n = len(msgs)
    ta = np.arange(3 * n, dtype=np.uint64).reshape(n, 3) + 10
    sa = ta + 1
    for i, m in enumerate(msgs):
        if m[4]:
            sa[i] = ta[i]
    b = R.Batch(np.zeros(n, np.uint32), 1, [flags], [num_running], [request_count], None, [m[0] for m in msgs],
                [m[2] for m in msgs], [m[3] for m in msgs], [m[1] for m in msgs], ta, sa, **kw)
    return _both(b)


def M(direction=R.DIR_REQUEST, flags=0, ttl=R.TTL_NONE, fwd=0, same=False):
    return (direction, flags, ttl, fwd, same)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("n,n_ctx", [(0, 1), (1, 1), (300, 1), (300, 7), (2000, 50), (5000, 700), (3000, 4000)])
@pytest.mark.parametrize("targets", ["uniform", "zipf"])
def test_closed_form_equals_loop(seed, n, n_ctx, targets):
    rng = np.random.default_rng(seed * 1000 + n + n_ctx)
    _both(R.mixed_batch(rng, n, n_ctx, targets, limits=seed % 3 != 0, chain=seed % 2 == 0))


def test_mixed_batch_covers_every_outcome_and_state():
    b = R.mixed_batch(np.random.default_rng(5), 5000, 300)
    turn = _both(b)[0]
    assert set(np.unique(turn).tolist()) == set(range(R.N_TURNS))
    assert set(np.unique(b.ctx_flags & R.CTX_STATE_MASK).tolist()) == {0, 1, 2}


def test_idle_activation_first_starts_second_waits():
    turn, nr, run, start, perm, off = _one(R.CTX_VALID, [M(), M()])
    assert turn.tolist() == [R.TURN_START, R.TURN_WAIT]
    assert nr.tolist() == [1] and run.tolist() == [0] and start.tolist() == [0]
    assert perm.tolist() == [1, 0] and off.tolist() == [0, 1, 2]


def test_read_only_interleaves_with_read_only_write_waits():
    ro = R.MSG_READ_ONLY
    turn, nr, run, *_ = _one(R.CTX_VALID, [M(flags=ro), M(flags=ro), M(), M(flags=ro)])
    assert turn.tolist() == [R.TURN_START, R.TURN_START, R.TURN_WAIT, R.TURN_START]
    assert nr.tolist() == [3] and run.tolist() == [0]
    # a write first: read-only requests after it wait
    turn, *_ = _one(R.CTX_VALID, [M(), M(flags=ro)])
    assert turn.tolist() == [R.TURN_START, R.TURN_WAIT]
    # Running from before the batch, read-only: the context's flag decides
    f = R.CTX_VALID | R.CTX_HAS_RUNNING | R.CTX_RUNNING_READ_ONLY
    turn, nr, run, *_ = _one(f, [M(flags=ro), M()], num_running=1)
    assert turn.tolist() == [R.TURN_START, R.TURN_WAIT] and nr.tolist() == [2] and run.tolist() == [R.NONE32]
    turn, *_ = _one(R.CTX_VALID | R.CTX_HAS_RUNNING, [M(flags=ro)], num_running=1)
    assert turn.tolist() == [R.TURN_WAIT]


def test_call_chain_match_option_on_and_off():
    f = R.CTX_VALID | R.CTX_HAS_RUNNING
    msgs = [M(same=True), M(same=False)]
    assert _one(f, msgs, num_running=1, chain=True)[0].tolist() == [R.TURN_START, R.TURN_WAIT]
    assert _one(f, msgs, num_running=1, chain=False)[0].tolist() == [R.TURN_WAIT, R.TURN_WAIT]


def test_reentrant_class_and_interleave_flags():
    f = R.CTX_VALID | R.CTX_HAS_RUNNING
    assert _one(f | R.CTX_REENTRANT, [M(), M(), M()], num_running=2)[0].tolist() == [R.TURN_START] * 3
    turn = _one(f, [M(flags=R.MSG_ALWAYS_INTERLEAVE), M(flags=R.MSG_MAY_INTERLEAVE), M()], num_running=1)[0]
    assert turn.tolist() == [R.TURN_START, R.TURN_START, R.TURN_WAIT]


def test_num_running_without_running():
    """numRunning > 0 with Running == null: CanInterleave's `Running == null` accepts, and the message
    becomes Running."""
    turn, nr, run, *_ = _one(R.CTX_VALID, [M(), M()], num_running=2)
    assert turn.tolist() == [R.TURN_START, R.TURN_WAIT] and nr.tolist() == [3] and run.tolist() == [0]
    # Running set but numRunning 0: the first request is accepted outright, Running stays
    turn, nr, run, *_ = _one(R.CTX_VALID | R.CTX_HAS_RUNNING, [M(), M()], num_running=0)
    assert turn.tolist() == [R.TURN_START, R.TURN_WAIT] and nr.tolist() == [1] and run.tolist() == [R.NONE32]


def test_expired_first_does_not_become_running():
    ro = R.MSG_READ_ONLY
    turn, nr, run, start, *_ = _one(R.CTX_VALID, [M(flags=ro, ttl=0), M(), M(flags=ro)])
    assert turn.tolist() == [R.TURN_EXPIRED, R.TURN_START, R.TURN_WAIT]
    assert run.tolist() == [1] and start.tolist() == [1] and nr.tolist() == [1]
    assert _one(R.CTX_VALID, [M(ttl=-7), M(ttl=1)])[0].tolist() == [R.TURN_EXPIRED, R.TURN_START]


def test_invalid_activation_forward_counts():
    turn, nr, run, start, *_ = _one(R.CTX_INVALID, [M(fwd=0), M(fwd=1), M(fwd=2), M(R.DIR_ONE_WAY, fwd=3),
                                                    M(R.DIR_RESPONSE)], max_forward_count=2)
    assert turn.tolist() == [R.TURN_FORWARD, R.TURN_FORWARD, R.TURN_REJECT_TRANSIENT, R.TURN_REJECT_TRANSIENT,
                             R.TURN_RESPONSE_DROPPED]
    assert nr.tolist() == [0] and run.tolist() == [R.NONE32] and len(start) == 0


def test_not_ready_waits():
    turn, nr, run, _, perm, off = _one(R.CTX_NOT_READY | R.CTX_REENTRANT, [M(), M(flags=R.MSG_ALWAYS_INTERLEAVE)])
    assert turn.tolist() == [R.TURN_WAIT, R.TURN_WAIT] and nr.tolist() == [0] and run.tolist() == [R.NONE32]
    assert perm.tolist() == [0, 1] and off.tolist() == [0, 2, 2]


def test_stuck():
    f = R.CTX_VALID | R.CTX_HAS_RUNNING | R.CTX_STUCK
    assert _one(f, [M(), M(flags=R.MSG_ALWAYS_INTERLEAVE)], num_running=1)[0].tolist() == [R.TURN_STUCK, R.TURN_START]
    # the overload check comes first
    assert _one(f, [M(), M()], num_running=1, request_count=4, hard_limit=3)[0].tolist() == \
        [R.TURN_REJECT_OVERLOADED, R.TURN_STUCK]


def test_response_between_requests():
    turn, nr, *_ = _one(R.CTX_VALID, [M(), M(R.DIR_RESPONSE), M(), M(R.DIR_ABSENT)])
    assert turn.tolist() == [R.TURN_START, R.TURN_RESPONSE, R.TURN_WAIT, R.TURN_WAIT] and nr.tolist() == [1]


def test_non_participating_messages_touch_nothing():
    b = R.Batch([0, 1, R.NONE32, 0], 1, [R.CTX_VALID], [0], [0], recv_status=[1, 0, 0, 0])
    turn, nr, run, *_ = _both(b)
    assert turn.tolist() == [R.TURN_NONE, R.TURN_NONE, R.TURN_NONE, R.TURN_START] and run.tolist() == [3]


@pytest.mark.parametrize("stateless", [False, True])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_overload_boundary(stateless, delta):
    """request_count - j == limit + delta for the first would-wait message (rank j = 1 behind a START)."""
    limit = 4
    f = R.CTX_VALID | (R.CTX_STATELESS_WORKER if stateless else 0)
    kw = dict(hard_limit_sw=limit, hard_limit=100) if stateless else dict(hard_limit=limit, hard_limit_sw=100)
    rc = limit + delta + 1
    turn = _one(f, [M()] * 4, request_count=rc, **kw)[0].tolist()
    # count before message j is rc - j while nothing has waited; the first wait freezes it at or under the limit
    want = [R.TURN_START] + [R.TURN_REJECT_OVERLOADED if rc - j > limit else R.TURN_WAIT for j in (1, 2, 3)]
    assert turn == want
    assert (R.TURN_REJECT_OVERLOADED in turn) == (delta == 1)


def test_rejected_prefix_then_waits():
    f = R.CTX_VALID | R.CTX_HAS_RUNNING
    turn, _, _, _, perm, off = _one(f, [M()] * 6, num_running=1, request_count=7, hard_limit=4)
    assert turn.tolist() == [R.TURN_REJECT_OVERLOADED] * 3 + [R.TURN_WAIT] * 3
    assert perm.tolist() == [3, 4, 5, 0, 1, 2] and off.tolist() == [0, 3, 6]
    # responses and expired messages between them still count down
    msgs = [M(), M(R.DIR_RESPONSE), M(ttl=0), M(), M()]
    assert _one(f, msgs, num_running=1, request_count=7, hard_limit=4)[0].tolist() == \
        [R.TURN_REJECT_OVERLOADED, R.TURN_RESPONSE, R.TURN_EXPIRED, R.TURN_WAIT, R.TURN_WAIT]


def test_request_count_after_receive():
    off = np.array([0, 2, 2, 5, 6, 7], np.uint32)           # n_ctx = 3, null bucket, not enqueued
    assert R.request_count_after_receive([1, 0, 4], off, 3).tolist() == [3, 0, 7]
