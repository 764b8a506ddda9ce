"""CPU tests of the micro-batch sorter's reference (_mbsort_ref.py): its two restatements against each
other, its checker against answers that are wrong in one way each, and the case table of
test_gpu_mbsort.py against the driver's documented choice of instantiation and grid."""
import types

import numpy as np
import pytest

import _mbsort_ref as R


def _same(a, b):
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
        assert x.dtype == y.dtype == np.uint32
    assert a[3] == b[3]


N_ACT_EDGES = [1, 2, 15, 16, 255, 2047, 2048, 1 << 20, (1 << 22) - 1, 1 << 22, 1 << 31, 0xFFFFFFFD, 0xFFFFFFFE]


@pytest.mark.parametrize("n_act", N_ACT_EDGES)
def test_literal_and_fast_restatements_agree(n_act):
    rng = np.random.default_rng(n_act & 0xFFFF)
    M = 0xFFFFFFFF
    hi = min(n_act + 40, M)
    batches = [
        np.zeros(0, np.uint32),                                                    # n = 0
        np.array([0], np.uint32), np.array([M], np.uint32),                        # n = 1
        np.full(300, min(7, n_act - 1), np.uint32),                                # all equal, below n_act
        np.full(300, M, np.uint32),                                                # all 0xFFFFFFFF
        rng.integers(n_act, M + 1, size=500, dtype=np.uint64).astype(np.uint32),   # all >= n_act
        rng.integers(0, hi + 1, size=2000, dtype=np.uint64).astype(np.uint32),     # uniform, some clamped
        rng.integers(max(0, n_act - 5), hi + 1, size=700, dtype=np.uint64).astype(np.uint32),   # around n_act
        np.where(rng.random(1500) < 0.5, M, rng.integers(0, 12, size=1500)).astype(np.uint32),  # few, long runs
        np.arange(600, dtype=np.uint32)[::-1].copy(),                              # descending
    ]
    for acts in batches:
        a, b = R.literal_runs(acts, n_act), R.fast_runs(acts, n_act)
        _same(a, b)
        perm, run_act, run_start, r = a
        n = len(acts)
        assert sorted(perm.tolist()) == list(range(n)) and run_start[r] == n and len(run_act) == r
        assert np.all(np.diff(run_act.astype(np.int64)) > 0) and (r == 0 or run_act[-1] <= n_act)
        assert (r == 0) == (n == 0)
        for q in range(r):                                   # each run: one activation, arrival order
            run = perm[run_start[q]:run_start[q + 1]].astype(np.int64)
            assert len(run) > 0 and np.all(np.diff(run) > 0)
            assert np.all(np.minimum(acts[run].astype(np.int64), n_act) == run_act[q])


def test_restatements_on_hand_written_batch():
    #        0  1   2  3           4  5  6
    acts = [5, 2, 9, 0xFFFFFFFF, 2, 5, 7]
    for f in (R.literal_runs, R.fast_runs):
        perm, run_act, run_start, r = f(np.asarray(acts, dtype=np.uint32), 7)
        assert perm.tolist() == [1, 4, 0, 5, 2, 3, 6]          # 9, the miss and 7 share the trailing bucket 7
        assert run_act.tolist() == [2, 5, 7] and run_start.tolist() == [0, 2, 4, 7] and r == 3


# ----------------------------------------------------------------------------- check() rejects wrong answers
def _stand_in(acts, n_act, capacity=64):
    perm, run_act, run_start, r = R.fast_runs(acts, n_act)
    s = types.SimpleNamespace(perm=np.full(capacity, 0xAAAAAAAA, np.uint32), n_runs=r,
                              run_act=np.full(capacity, 0xAAAAAAAA, np.uint32),
                              run_start=np.full(capacity + 1, 0xAAAAAAAA, np.uint32))
    s.perm[:len(perm)], s.run_act[:r], s.run_start[:r + 1] = perm, run_act, run_start
    return s


_ACTS = np.array([4, 9, 4, 1, 9, 9, 30, 1, 4, 77, 2, 30], dtype=np.uint32)     # n_act 40: runs 1 2 4 9 30 40
_N_ACT = 40


def _swap_in_run(s):            # the two first entries of the run of 4: arrival order lost
    a = int(s.run_start[2])
    s.perm[[a, a + 1]] = s.perm[[a + 1, a]]


def _swap_runs(s):              # the runs of 4 (3 messages) and 9 (3 messages) change places
    a, b, c = (int(x) for x in s.run_start[2:5])
    s.perm[a:c] = np.concatenate([s.perm[b:c], s.perm[a:b]])
    s.run_act[[2, 3]] = s.run_act[[3, 2]]


def _one_run_less(s):
    s.n_runs -= 1


def _one_run_more(s):
    s.n_runs += 1
    s.run_start[s.n_runs] = len(_ACTS)


def _open_end(s):               # run_start[r] is not n
    s.run_start[s.n_runs] = len(_ACTS) - 1


def _duplicate(s):              # one entry twice, another lost
    s.perm[5] = s.perm[4]


def _wrong_run_act(s):
    s.run_act[1] += 1


def _wrong_run_start(s):
    s.run_start[3] += 1


def test_check_accepts_the_reference():
    R.check(_stand_in(_ACTS, _N_ACT), len(_ACTS), _ACTS, _N_ACT)
    R.check(_stand_in(_ACTS[:0], _N_ACT), 0, _ACTS, _N_ACT)
    s = _stand_in(_ACTS[:5], _N_ACT)                            # n below len(acts): only acts[:n] count
    R.check(s, 5, _ACTS, _N_ACT)


@pytest.mark.parametrize("perturb", [_swap_in_run, _swap_runs, _one_run_less, _one_run_more, _open_end,
                                     _duplicate, _wrong_run_act, _wrong_run_start], ids=lambda f: f.__name__)
def test_check_rejects(perturb):
    s = _stand_in(_ACTS, _N_ACT)
    perturb(s)
    with pytest.raises(AssertionError):
        R.check(s, len(_ACTS), _ACTS, _N_ACT)


def test_check_rejects_a_stale_empty_batch():
    s = _stand_in(_ACTS[:0], _N_ACT)
    s.n_runs = 1
    with pytest.raises(AssertionError):
        R.check(s, 0, _ACTS, _N_ACT)
    s = _stand_in(_ACTS[:0], _N_ACT)
    s.run_start[0] = 3
    with pytest.raises(AssertionError):
        R.check(s, 0, _ACTS, _N_ACT)


# ----------------------------------------------------------------------------- the case table
def test_plan_restates_the_documented_choice():
    assert R.plan(10, 8192) == (4, 1, 8, 8)
    assert R.plan(50000, 4096) == (8, 2, 4, 8)
    assert R.plan(12000, 2048) == (7, 2, 4, 8)
    assert R.plan(1 << 20, 4096) == (11, 2, 4, 8)
    assert R.plan((1 << 22) - 1, 4097) == (11, 2, 8, 8)
    assert R.plan(1 << 22, 255, 64) == (8, 3, 4, 1)
    assert R.plan(0xFFFFFFFE, 8192, 64) == (11, 3, 8, 32)
    assert R.plan(1, 0) == (4, 1, 4, 1)


def test_case_table_covers_every_instantiation():
    pairs = [(b, 1) for b in range(4, 12)] + [(b, 2) for b in range(6, 12)] + [(b, 3) for b in range(8, 12)]
    # what the driver's rule can reach at all: every bit length of n_act
    reachable = {R.plan((1 << kb) - 1, 1)[:2] for kb in range(1, 33)}
    assert reachable == set(pairs) and len(pairs) == 18
    table = R.table()
    plans = {R.plan(na, n, s) for na, n, s in table}
    assert {p[:3] for p in plans} == {(b, p, it) for b, p in pairs for it in (4, 8)}
    assert {p[:2] for p in {R.plan(na, 1) for na in R.N_ACTS}} == set(pairs) and len(R.N_ACTS) == 21
    assert (1 << 20, 4096, 8) in table and R.plan(1 << 20, 4096)[:3] == (11, 2, 4)      # bench.py's cfg 5
    assert {s for _, _, s in table} == set(R.SPLITS) == {1, 2, 3, 7, 8, 31, 32, 64}
    assert {1, 2, 3, 7, 8, 31, 32} <= {p[3] for p in plans}
    for na in R.ANCHORS:                                       # each anchor: every split, every grid
        assert {1, 2, 3, 7, 8, 31, 32} <= {R.plan(a, n, s)[3] for a, n, s in table if a == na}
        assert {R.plan(na, n)[2] for n in R.SPLIT_NS} == {4, 8}
    assert set(R.ANCHORS) <= set(R.N_ACTS)
    assert all(0 <= n <= R.MB_MAX for _, n, _ in table) and all(1 <= na <= 0xFFFFFFFE for na, _, _ in table)
    for na in R.N_ACTS:
        assert set(R.patterns_of(na)) >= {"uniform", "one"} and set(R.patterns_of(na)) <= set(R.ANCHOR_PATTERNS)
        assert any(f in R.patterns_of(na) for f in R.FAMILIES)


def test_activation_numbers():
    acts, fam = R.activation_numbers()
    assert acts.dtype == np.uint32 and len(acts) == 8192 and len(np.unique(acts)) == 8192
    assert acts.max() == R.ACT_MAX == 0xFFFFFFFD and acts.min() == 0
    lengths = np.array([int(a).bit_length() for a in acts])
    assert set(lengths.tolist()) == set(range(33))
    assert min(np.count_nonzero(lengths == b) for b in range(11, 33)) >= 256
    assert sorted(acts[fam["j"]].tolist()) == list(range(1024))
    assert sorted(acts[fam["j<<11"]].tolist()) == [j << 11 for j in range(1, 1024)]
    assert sorted(acts[fam["j<<22"]].tolist()) == [j << 22 for j in range(1, 512)]
    for na in R.N_ACTS:                                         # activations on both sides of every n_act
        assert (acts < na).any() and (na == 0xFFFFFFFE or (acts > na).any())
    again, _ = R.activation_numbers()
    assert np.array_equal(acts, again)
