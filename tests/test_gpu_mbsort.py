"""The micro-batch sorter (k_mb_sort_runs, gd_mbsort.h) at every digit width, pass count, rows-per-wave
and store split the driver can choose, against _mbsort_ref.py, bit for bit.

mb_enqueue (eng_abi.hip) picks k_mb_sort_runs<bits, IT> and the pass count from n_act and n; the 21
n_act values of _mbsort_ref.N_ACTS reach all 18 (bits, passes) pairs, each with IT = 4 and IT = 8
(test_mbsort_ref.py proves that of the table), bench.py's cfg 5 shape (n_act = 2^20, n = 4096: two 11-bit
passes, IT = 4) among them.  Every case runs through gd_microbatch_run eagerly and as a graph replay, on
a handle with the default ranks and on one with every rank by ballots (no_lane_order); the outputs are
overwritten before each run, so a run that stores nothing fails.  The 8,192 registered grains carry
chosen activation numbers (_mbsort_ref.activation_numbers): every bit length up to 32, and three
families whose low or high digits coincide.  Status, silo and act are checked against the oracle's
route, perm and the runs against _mbsort_ref.check over the routed activations.

Registered activation numbers stop at 0xFFFFFFFD: gd_dir_register takes 0xFFFFFFFE, but as
GD_ACT_MULTI (a grain with several activations, routed with act 0xFFFFFFFF), not as an activation.

Not covered here: the LocalLookup (cache_max) route's act_copy stores under a non-default split (that
route runs with the default split in test_gpu_cache.py), and GD_OPT_MB_TRACE (the timestamp stores of
mb_mark)."""
import numpy as np
import pytest

import _mbsort_ref as R
import oracle as o

pytestmark = pytest.mark.gpu

TC = o.grain_type_code(o.PING_GRAIN_CLASS)
G = 8192                   # registered grains: ids 0..G-1; ids G..2G-1 are unregistered
CAP = R.MB_MAX
MODES = ("lane_order", "ballots")


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


class World:
    """Two handles (one per rank mode) over the same ring and directory, and the oracle's route of
    every grain id, computed once."""

    def __init__(self, gd):
        self.gd = gd
        silos = o.bench_silos(8)
        spec = o.ring_spec(silos, "D")
        self.acts, self.fam = R.activation_numbers()
        self.pool = o.grain_keys(TC, np.arange(2 * G))
        reg = self.pool[:G]
        owner = o.ring_owner_np(spec, o.jenkins_u64x3_np(reg[:, 2], reg[:, 0], reg[:, 1])).astype(np.uint32)
        st, silo, act = o.route_batch_np(self.pool, spec, o.DirectoryArrays(reg, self.acts, owner))[:3]
        assert np.array_equal(act[:G], self.acts) and np.all(act[G:] == o.M32) and np.all(st[G:] == o.ST_MISS)
        self.want = (st, silo, act)
        self.by_act = np.argsort(self.acts, kind="stable")        # grain ids by ascending activation
        self.handles = {}
        for mode in MODES:
            e = gd.GrainDispatch(device=0, table_capacity=1 << 15, no_lane_order=(mode == "ballots"))
            e.ring_set_silos("D", [(s.ip, s.port, s.gen) for s in silos])
            got_act, got_silo, ins = e.register(reg, self.acts, owner)
            assert ins.all() and np.array_equal(got_act, self.acts) and np.array_equal(got_silo, owner)
            self.handles[mode] = e

    def close(self):
        for e in self.handles.values():
            e.close()

    def below(self, n_act):
        """Grain ids with an activation below n_act, by ascending activation."""
        return self.by_act[:int(np.searchsorted(self.acts[self.by_act], n_act, side="left"))]

    def ids(self, pattern, n, n_act, seed, grid=1):
        """The grain ids of a batch of n messages."""
        rng = np.random.default_rng([n_act & 0xFFFFFFFF, n, seed])
        i = np.arange(n)
        below = self.below(n_act)
        a, b = int(below[-1]), int(below[len(below) // 2])        # the largest activation in range, the median
        if pattern == "uniform":
            return rng.integers(0, G, size=n)
        if pattern == "one":                                      # the hot digit in every lane, every pass
            return np.full(n, a)
        if pattern == "alt_lane":
            return np.where(i & 1, a, b)
        if pattern == "alt_row":
            return np.where((i // 64) & 1, a, b)
        if pattern == "descending":
            some = rng.choice(G, size=n, replace=False)
            return some[np.argsort(self.acts[some], kind="stable")[::-1]]
        if pattern == "unregistered":                             # every key in the trailing bucket n_act
            return G + rng.integers(0, G, size=n)
        if pattern == "half_unregistered":
            return np.where(rng.random(n) < 0.5, G + rng.integers(0, G, size=n), rng.integers(0, G, size=n))
        if pattern in self.fam:
            return rng.choice(self.fam[pattern], size=n)
        if pattern in ("edge", "edge+1"):
            # two runs; the second starts on the edge of a sorter's share [n b / g, n (b + 1) / g), or one past
            assert len(below) >= 2 and n >= 2
            edge = n * ((grid + 1) // 2) // grid if grid > 1 else n // 2
            first = edge + (1 if pattern == "edge+1" else 0)
            assert 0 < first < n
            out = np.full(n, a)
            out[rng.permutation(n)[:first]] = b
            return out
        raise KeyError(pattern)


@pytest.fixture(scope="module")
def world(gd):
    w = World(gd)
    yield w
    w.close()


def _poison(mb):
    for v in (mb.silo, mb.act, mb.perm, mb.run_start, mb.run_act, mb._n_runs):
        v[:] = 0xEEEEEEEE
    mb.status[:] = 0xEE


def _run_and_check(w, mb, n, ids, n_act, what):
    st, silo, act = (x[ids] for x in w.want)
    mb.keys[:n] = w.pool[ids]
    for use_graph in (False, True):
        _poison(mb)
        mb.run(n, use_graph)
        where = f"{what} n={n} {'graph' if use_graph else 'eager'}"
        assert np.array_equal(mb.status[:n], st) and np.array_equal(mb.silo[:n], silo), where
        assert np.array_equal(mb.act[:n], act), where
        try:
            R.check(mb, n, act, n_act)
        except AssertionError as err:
            raise AssertionError(f"{where}: {err}") from None


class _Batches:
    """One MicroBatch per rank mode, with handle options set for their creation only."""

    def __init__(self, w, n_act, **options):
        self.w, self.options, self.mbs = w, options, {}
        self.n_act = n_act

    def __enter__(self):
        for mode, e in self.w.handles.items():
            saved = {k: e.get_option(k) for k in self.options}
            try:
                for k, v in self.options.items():
                    e.set_option(k, v)                            # read at gd_microbatch_create
                    assert e.get_option(k) == v
                self.mbs[mode] = self.w.gd.MicroBatch(e, CAP, self.n_act)
            finally:
                for k, v in saved.items():
                    e.set_option(k, v)
        return self.mbs

    def __exit__(self, *exc):
        for mb in self.mbs.values():
            mb.close()


@pytest.mark.parametrize("n_act", R.N_ACTS)
def test_every_digit_width_and_pass_count(world, n_act):
    with _Batches(world, n_act) as mbs:
        for n in R.ns_of(n_act):
            for k, pattern in enumerate(R.patterns_of(n_act)):
                ids = world.ids(pattern, n, n_act, k)
                for mode, mb in mbs.items():
                    _run_and_check(world, mb, n, ids, n_act, f"n_act={n_act} {pattern} {mode}")


@pytest.mark.parametrize("split", R.SPLITS)
@pytest.mark.parametrize("n_act", R.ANCHORS)
def test_split_stores(world, n_act, split):
    """min(split, n / 256) sorters, each storing its share: one grain (every share cuts the run), and two
    runs whose boundary is a share's edge or one past it."""
    with _Batches(world, n_act, mb_split=split) as mbs:
        for n in R.SPLIT_NS:
            grid = R.plan(n_act, n, split)[3]
            for k, pattern in enumerate(R.SPLIT_PATTERNS):
                ids = world.ids(pattern, n, n_act, k, grid)
                for mode, mb in mbs.items():
                    _run_and_check(world, mb, n, ids, n_act, f"n_act={n_act} split={split} {pattern} {mode}")


@pytest.mark.parametrize("n_act", R.ANCHORS)
def test_staged_copies(world, n_act):
    """mb_zerocopy = 0: H2D keys, one sorter, one D2H of the output block."""
    with _Batches(world, n_act, mb_zerocopy=0) as mbs:
        for n in R.STAGED_NS:
            for k, pattern in enumerate(("uniform", "one")):
                ids = world.ids(pattern, n, n_act, k)
                for mode, mb in mbs.items():
                    _run_and_check(world, mb, n, ids, n_act, f"n_act={n_act} staged {pattern} {mode}")


@pytest.mark.parametrize("n_act", R.ANCHORS)
def test_state_reuse(world, n_act):
    """One MicroBatch, n going 8192 -> 1 -> 4097 -> 0 -> 4096 three times over with new keys, eager and
    graph interleaved, nothing cleared in between: outputs past n are stale, each n has its cached graph,
    and n = 0 gives no runs."""
    with _Batches(world, n_act) as mbs:
        for mode, mb in mbs.items():
            for rnd in range(3):
                for i, n in enumerate(R.REUSE_NS):
                    use_graph = (i + rnd) % 2 == 1
                    ids = world.ids(("uniform", "half_unregistered", "j<<11")[rnd], n, n_act, 10 + rnd)
                    st, silo, act = (x[ids] for x in world.want)
                    mb.keys[:n] = world.pool[ids]
                    mb.run(n, use_graph)
                    where = f"n_act={n_act} {mode} round {rnd} n={n} {'graph' if use_graph else 'eager'}"
                    assert np.array_equal(mb.status[:n], st) and np.array_equal(mb.silo[:n], silo), where
                    assert np.array_equal(mb.act[:n], act), where
                    try:
                        R.check(mb, n, act, n_act)
                    except AssertionError as err:
                        raise AssertionError(f"{where}: {err}") from None
                    if n == 0:
                        assert mb.n_runs == 0 and mb.run_start[0] == 0, where
