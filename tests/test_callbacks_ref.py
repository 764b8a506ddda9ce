"""The callback table's literal loop (_callbacks_ref.Table) against the closed form of respond (respond_np), one
hand-written case per rule line, and a request's lifecycle.  CPU only."""
import copy

import numpy as np
import pytest

import _callbacks_ref as R
from _callbacks_ref import (CB_FIRE, CB_GATEWAY_BACK, CB_NO_CALLBACK, CB_NONE, CB_RESEND, CB_SILO_FAILED, CB_TIMEOUT,
                            NO_HANDLE, NO_SILO, Options, Table)

I64 = lambda *a: np.array(a, np.int64)
U8 = lambda *a: np.array(a, np.uint8)
U32 = lambda *a: np.array(a, np.uint32)


def filled(opt, n=40, resend=None):
    t = Table(opt)
    t.add(np.arange(100, 100 + n, dtype=np.int64), np.arange(n, dtype=np.uint32) + 7, np.full(n, 1000, np.int64))
    if resend is not None:
        for k, e in t.d.items():
            e[2] = int(resend[(k - 100) % len(resend)])
    return t


@pytest.mark.parametrize("max_resend", [0, 1, 3])
@pytest.mark.parametrize("seed", range(12))
def test_loop_equals_closed_form(seed, max_resend):
    rng = np.random.default_rng(seed * 7 + max_resend)
    a = filled(Options(max_resend), n=400, resend=[0, 0, 1, 2, 3, 4])
    b = copy.deepcopy(a)
    for step in range(4):
        ids, res, rej, fl = R.mixed_batch(rng, a, 300)
        turn = None if step % 2 == 0 else rng.choice(np.array([1, 8, 9], np.uint8), len(ids), p=[0.2, 0.7, 0.1])
        want = a.respond(ids, res, rej, fl, turn)
        got = R.respond_np(b, ids, res, rej, fl, turn)
        for w, g, name in zip(want, got, ("outcome", "flags", "handle", "fire_idx")):
            assert w.dtype == g.dtype, name
            np.testing.assert_array_equal(g, w, err_msg=f"{name} step {step}")
        assert a.d == b.d
        # the first batch (the table still full) contained what it should
        assert step or len(set(want[0])) >= 3 and np.any(np.bincount(np.unique(ids, return_inverse=True)[1]) >= 2)


def test_closed_form_null_arrays_all_success():
    a, b = filled(Options(2)), filled(Options(2))
    ids = I64(100, 101, 100, 5)
    want, got = a.respond(ids), R.respond_np(b, ids)
    np.testing.assert_array_equal(want[0], U8(CB_FIRE, CB_FIRE, CB_NO_CALLBACK, CB_NO_CALLBACK))
    for w, g in zip(want, got):
        np.testing.assert_array_equal(g, w)
    assert a.d == b.d


# ---- one case per rule line ---------------------------------------------------------------------

def test_rule1_gateway_back_touches_nothing():
    t = filled(Options(3))
    o, f, h, fire = t.respond(I64(100), U8(R.REJECTION), U8(R.TRANSIENT), U8(R.RESP_TARGET_NOT_ME))
    assert (o[0], f[0], h[0], len(fire)) == (CB_GATEWAY_BACK, 0, NO_HANDLE, 0)
    assert t.d[100] == [7, 1000, 0, NO_SILO]
    # only a rejection is gatewayed back: a Success with the flag fires
    o, _, _, _ = t.respond(I64(100), U8(R.SUCCESS), None, U8(R.RESP_TARGET_NOT_ME))
    assert o[0] == CB_FIRE


@pytest.mark.parametrize("rej,hdr,want", [(R.TRANSIENT, 0, 1), (R.UNRECOVERABLE, 0, 1), (R.TRANSIENT, 2, 0),
                                          (R.UNRECOVERABLE, 2, 0), (R.OVERLOADED, 0, 0), (R.DUPLICATE, 0, 0),
                                          (R.GATEWAY_TOO_BUSY, 0, 0)])
def test_rule2_cache_invalidation_bit(rej, hdr, want):
    t = filled(Options(0))
    # the bit does not depend on the id being there
    _, f, _, _ = t.respond(I64(100, 1), U8(R.REJECTION, R.REJECTION), U8(rej, rej), U8(hdr, hdr))
    assert list(f) == [want, want]
    _, f, _, _ = t.respond(I64(101), U8(R.ERROR), U8(rej), U8(hdr))
    assert f[0] == 0


def test_rule3_no_callback():
    t = filled(Options(0))
    o, _, h, fire = t.respond(I64(5))
    assert (o[0], h[0], len(fire)) == (CB_NO_CALLBACK, NO_HANDLE, 0) and t.count() == 40


def test_rule4_transient_resend_keeps_the_entry_and_clears_the_target():
    t = filled(Options(2))
    t.set_target(I64(100), U32(3))
    o, _, h, fire = t.respond(I64(100), U8(R.REJECTION), U8(R.TRANSIENT))
    assert (o[0], h[0], len(fire)) == (CB_RESEND, 7, 0) and t.d[100] == [7, 1000, 1, NO_SILO]
    o, _, _, _ = t.respond(I64(100), U8(R.REJECTION), U8(R.TRANSIENT))
    assert o[0] == CB_RESEND and t.d[100][2] == 2
    o, _, h, fire = t.respond(I64(100), U8(R.REJECTION), U8(R.TRANSIENT))       # MayResend is false now
    assert (o[0], h[0], list(fire)) == (CB_FIRE, 7, [0]) and 100 not in t.d
    # a rejection that is not transient is never resent
    o, _, _, _ = t.respond(I64(101), U8(R.REJECTION), U8(R.OVERLOADED))
    assert o[0] == CB_FIRE


def test_rule5_fire_removes_and_later_responses_find_nothing():
    t = filled(Options(1))
    o, _, h, fire = t.respond(I64(100, 101, 100, 100), U8(2, 0, 0, 2), U8(0, 0, 0, 0))
    assert list(o) == [CB_RESEND, CB_FIRE, CB_FIRE, CB_NO_CALLBACK]
    assert list(h) == [7, 8, 7, NO_HANDLE] and list(fire) == [1, 2] and t.count() == 38


def test_turn_mask():
    t = filled(Options(0))
    o, f, h, fire = t.respond(I64(100, 101, 102), U8(2, 0, 0), U8(0, 0, 0), None, U8(1, 8, 9))
    assert list(o) == [CB_NONE, CB_FIRE, CB_NONE] and list(f) == [0, 0, 0] and list(fire) == [1]
    assert list(h) == [NO_HANDLE, 8, NO_HANDLE] and t.count() == 39


@pytest.mark.parametrize("resend_on_timeout", [False, True])
def test_expire(resend_on_timeout):
    t = Table(Options(1, resend_on_timeout, 50))
    t.add(I64(1, 2, 3), U32(10, 20, 30), I64(99, 100, 101))
    t.set_target(I64(1), U32(4))
    ids, hs, kinds = t.expire(100)
    assert list(ids) == [1, 2] and list(hs) == [10, 20]
    if resend_on_timeout:
        assert list(kinds) == [CB_RESEND, CB_RESEND]
        assert t.d[1] == [10, 149, 1, NO_SILO] and t.d[2] == [20, 150, 1, NO_SILO]
        assert len(t.expire(100)[0]) == 0                                        # one tick a call; not due yet
        ids, _, kinds = t.expire(150)
        assert list(ids) == [1, 2, 3] and list(kinds) == [CB_TIMEOUT, CB_TIMEOUT, CB_RESEND]
        assert t.d == {3: [30, 151, 1, NO_SILO]}
    else:
        assert list(kinds) == [CB_TIMEOUT, CB_TIMEOUT] and sorted(t.d) == [3]


@pytest.mark.parametrize("resend_on_timeout", [False, True])
def test_break_silo(resend_on_timeout):
    t = Table(Options(1, resend_on_timeout, 50))
    t.add(I64(1, 2, 3), U32(10, 20, 30), I64(100, 100, 100))
    t.set_target(I64(1, 2, 3, 3), U32(4, 5, 5, 4))                               # the last one stands
    assert len(t.break_silo(5)[0]) == 1 and len(t.break_silo(9)[0]) == 0
    ids, hs, kinds = t.break_silo(4)
    assert list(ids) == [1, 3] and list(hs) == [10, 30]
    if resend_on_timeout:
        assert list(kinds) == [CB_RESEND, CB_RESEND] and t.d[1] == [10, 100, 1, NO_SILO]   # the deadline stands
        assert len(t.break_silo(4)[0]) == 0                                      # the target was cleared
    else:
        assert list(kinds) == [CB_SILO_FAILED, CB_SILO_FAILED] and t.count() == 0


def test_add_first_wins_and_set_target_absent():
    t = Table()
    assert list(t.add(I64(9, 9, 8), U32(1, 2, 3), I64(5, 6, 7))) == [1, 0, 1] and t.d[9] == [1, 5, 0, NO_SILO]
    assert list(t.add(I64(9), U32(4), I64(1))) == [0]
    assert list(t.set_target(I64(9, 7), U32(2, 2))) == [1, 0]
    h, r, s, f = t.lookup(I64(9, 7))
    assert (list(h), list(r), list(s), list(f)) == ([1, NO_HANDLE], [0, 0], [2, NO_SILO], [1, 0])


def test_lifecycle():
    """add -> set_target -> respond (transient, resent) -> respond (fires) -> respond again (no callback) ->
    expire (nothing left)."""
    t = Table(Options(1, True, 10))
    assert list(t.add(I64(42), U32(5), I64(100))) == [1]
    assert list(t.set_target(I64(42), U32(2))) == [1]
    o, f, h, _ = t.respond(I64(42), U8(R.REJECTION), U8(R.TRANSIENT))
    assert (o[0], f[0], h[0]) == (CB_RESEND, 1, 5) and t.d[42] == [5, 100, 1, NO_SILO]
    o, _, h, fire = t.respond(I64(42))
    assert (o[0], h[0], list(fire)) == (CB_FIRE, 5, [0])
    o, _, h, _ = t.respond(I64(42))
    assert (o[0], h[0]) == (CB_NO_CALLBACK, NO_HANDLE)
    assert len(t.expire(1 << 40)[0]) == 0 and t.count() == 0
