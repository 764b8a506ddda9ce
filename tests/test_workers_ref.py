"""CPU tests of the stateless-worker reference (tests/_workers_ref.py): the literal per-message simulation of
StatelessWorkerDirector.SelectActivationCore and the closed form the kernels follow agree on randomized worlds --
that agreement is the proof that the closed form is the sequential model -- and hand-written cases at the edges."""
import numpy as np
import pytest

import _workers_ref as W

TCD = (W.CAT_GRAIN << 56) | (77 << 32)
CLIENT = 4 << 56


def key(i, tcd=TCD):
    return [0, i, tcd]


def both(w, *a, **kw):
    """select_loop and select_closed on clones of w: equal outputs and equal tables; returns (ctx, pick, new_idx, table)."""
    wl, wc = w.clone(), w.clone()
    got_l = W.select_loop(wl, *a, **kw)
    got_c = W.select_closed(wc, *a, **kw)
    for x, y, name in zip(got_l, got_c, ("ctx", "pick", "new_idx")):
        np.testing.assert_array_equal(x, y, err_msg=name)
    assert wl.sets == wc.sets
    return got_l + (wl,)


@pytest.mark.parametrize("seed", range(12))
def test_loop_equals_closed_form_on_random_worlds(seed):
    rng = np.random.default_rng(seed)
    sc = int(rng.choice([1, 2, 5, 16, 64]))
    n_ctx = 200
    w, keys, fl, nr, wo = W.random_world(rng, 9, sc, n_ctx, TCD)
    n = int(rng.integers(0, 400))
    pool = np.concatenate([keys, np.array([key(10 ** 6 + j) for j in range(4)], np.uint64),
                           np.array([[0, 5, CLIENT]], np.uint64)])
    p = rng.random(len(pool)) ** 3
    batch = pool[rng.choice(len(pool), size=n, p=p / p.sum())]
    ml = rng.integers(-1, sc + 2, n).astype(np.int32)
    draw = rng.integers(0, 1 << 31, n).astype(np.uint32)
    draw[rng.random(n) < 0.05] = 0x7FFFFFFF
    ctx, pick, new_idx, after = both(w, batch, 5000, fl, nr, wo if seed % 3 else None, ml if seed % 2 else None,
                                     draw if seed % 4 else None)
    assert np.array_equal(ctx[new_idx], 5000 + np.arange(len(new_idx)))          # dense, in batch order
    assert np.array_equal(np.flatnonzero(pick == W.WK_NEW), new_idx)
    for s in after.sets.values():
        assert 0 < len(s[1]) <= sc and len(set(s[1])) == len(s[1])


def world(c, m, idle, sc=1024, n_ctx=64):
    """One set of c workers (contexts 0..c-1) with MaxLocal m, the first `idle` of them idle and the rest running."""
    w = W.Workers(sc, 1)
    if c:
        w.sets[tuple(key(1))] = [m, list(range(c))]
    fl = np.zeros(n_ctx, np.uint8)
    nr = np.ones(n_ctx, np.uint32)
    nr[:idle] = 0
    return w, fl, nr


@pytest.mark.parametrize("m", [1, 4])
@pytest.mark.parametrize("c_rel", ["0", "m-1", "m", "m+2"])
@pytest.mark.parametrize("a_rel", ["0", "1", "c"])
def test_counts_at_the_edges(m, c_rel, a_rel):
    c = {"0": 0, "m-1": m - 1, "m": m, "m+2": m + 2}[c_rel]
    a = {"0": 0, "1": min(1, c), "c": c}[a_rel]
    w, fl, nr = world(c, m, a)
    n = a + max(0, m - c) + 3
    draw = np.arange(n, dtype=np.uint32) * np.uint32(300000007) & np.uint32(0x7FFFFFFE)
    ctx, pick, new_idx, after = both(w, [key(1)] * n, 100, fl, nr, None, np.full(n, m, np.int32), draw)
    room = max(0, m - c)
    assert list(pick[:a]) == [W.WK_IDLE] * a and list(ctx[:a]) == list(range(a))
    assert list(pick[a:a + room]) == [W.WK_NEW] * room and list(ctx[a:a + room]) == list(range(100, 100 + room))
    assert all(p == W.WK_RANDOM for p in pick[a + room:])
    final = list(range(c)) + list(range(100, 100 + room))
    assert after.sets[tuple(key(1))] == [m, final]
    for i in range(a + room, n):
        r = 0 if len(final) == 1 else W.random_index(int(draw[i]), len(final))
        assert ctx[i] == final[r]


def test_max_local_one_ignores_a_garbage_draw():
    w, fl, nr = world(1, 1, 0)
    draw = np.array([0xFFFFFFFF, 0x7FFFFFFF, 12345], np.uint32)
    ctx, pick, new_idx, _ = both(w, [key(1)] * 3, 9, fl, nr, None, None, draw)
    assert list(pick) == [W.WK_RANDOM] * 3 and list(ctx) == [0, 0, 0] and len(new_idx) == 0
    ctx, pick, _, _ = both(w, [key(1)] * 2, 9, fl, nr, None, None, None)          # no draws at all
    assert list(pick) == [W.WK_RANDOM] * 2


@pytest.mark.parametrize("C", [2, 3, 1024])
def test_draw_extremes(C):
    assert W.random_index(0, C) == 0
    assert W.random_index(0x7FFFFFFE, C) == C - 1
    w, fl, nr = world(C, C, 0)
    draw = np.array([0, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000], np.uint32)
    ctx, pick, _, _ = both(w, [key(1)] * 4, 5000, fl, nr, None, np.full(4, C, np.int32), draw)
    assert list(pick) == [W.WK_RANDOM, W.WK_RANDOM, W.WK_HELD, W.WK_HELD]
    assert list(ctx) == [0, C - 1, W.NONE32, W.NONE32]


def test_held_consumes_its_rank_and_null_draws_hold():
    w, fl, nr = world(2, 3, 1)
    ctx, pick, new_idx, after = both(w, [key(1)] * 5, 50, fl, nr, None, np.full(5, 3, np.int32), None)
    assert list(pick) == [W.WK_IDLE, W.WK_NEW, W.WK_HELD, W.WK_HELD, W.WK_HELD]
    assert list(new_idx) == [1] and after.sets[tuple(key(1))] == [3, [0, 1, 50]]


def test_random_lands_on_this_batchs_own_workers():
    w = W.Workers(8, 3)
    draw = np.array([0, 0, 0, 0x7FFFFFFE, 0x40000000], np.uint32)
    ctx, pick, new_idx, after = both(w, [key(9)] * 5, 700, np.zeros(0, np.uint8), np.zeros(0, np.uint32), None, None, draw)
    assert list(pick) == [W.WK_NEW] * 3 + [W.WK_RANDOM] * 2
    assert list(ctx) == [700, 701, 702, 702, 701] and after.sets[tuple(key(9))] == [3, [700, 701, 702]]


def test_client_is_none_and_oversized_max_local_is_held():
    w = W.Workers(4, 2)
    keys = [[0, 5, CLIENT], key(1), key(1)]
    ctx, pick, new_idx, after = both(w, keys, 10, np.zeros(0, np.uint8), np.zeros(0, np.uint32), None,
                                     np.array([1, 5, 4], np.int32), None)
    assert list(pick) == [W.WK_NONE, W.WK_HELD, W.WK_NEW] and after.sets[tuple(key(1))] == [4, [10]]


def test_idle_needs_all_four_checks():
    w = W.Workers(8, 8)
    w.sets[tuple(key(1))] = [8, [0, 1, 2, 3, 4, 70]]
    fl = np.array([0, 1, 2, 0, 0], np.uint8)                       # 1 NOT_READY, 2 INVALID
    nr = np.array([0, 0, 0, 1, 0xFFFFFFFF], np.uint32)             # 3 running, 4 at -1 (inactive)
    wo = np.array([0, 1, 1, 1, 1, 1], np.uint32)                   # 0 has a waiting message
    ctx, pick, _, _ = both(w, [key(1)] * 2, 100, fl, nr, wo, None, None)
    assert list(pick) == [W.WK_IDLE, W.WK_NEW] and ctx[0] == 4     # 70 >= n_ctx: counted, never idle
    ctx, pick, _, _ = both(w, [key(1)], 100, fl, nr, None, None, None)
    assert ctx[0] == 0                                             # no waiting lists: context 0 is idle


def test_add_and_remove_loops():
    w = W.Workers(3, 2)
    st = w.add_loop([key(1), key(1), key(2), key(1), key(1), [0, 5, CLIENT], key(3)], [10, 11, 20, 12, 13, 1, 30],
                    np.array([0, 0, 0, 0, 0, 0, 4], np.int32))
    assert list(st) == [W.WK_ADDED, W.WK_ADDED, W.WK_ADDED, W.WK_ADDED, W.WK_FULL, W.WK_NOT_GRAIN, W.WK_FULL]
    assert w.sets[tuple(key(1))] == [2, [10, 11, 12]] and tuple(key(3)) not in w.sets
    out = w.remove_loop([key(1), key(1), key(1), key(2), key(7)], [11, 11, 10, 20, 1])
    assert list(out) == [1, 0, 1, 1, 0]
    assert w.sets[tuple(key(1))] == [2, [12]] and tuple(key(2)) not in w.sets
    cnt, ml, lst = w.lookup([key(1), key(2)])
    assert list(cnt) == [1, 0] and list(ml) == [2, 0] and list(lst[0]) == [12, W.NONE32, W.NONE32]
