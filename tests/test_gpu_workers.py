"""GPU parity for the stateless-worker stage: gd_workers_select / add / remove / lookup through the C ABI against the
literal restatement of StatelessWorkerDirector.SelectActivationCore and the ActivationDirectory's worker lists
(_workers_ref.py), bit for bit: ctx, pick, new_idx, n_new, and afterwards gd_workers_lookup of every grain seen."""
import numpy as np
import pytest

import _chain_keys as CK
import _turns_ref as TR
import _workers_ref as W
import oracle as o

pytestmark = pytest.mark.gpu

WK_TILE = 256                     # k_wk_find / k_wk_claim / k_wk_classify / k_wk_finish: messages a workgroup (BLOCK)
WK_SET_NT = 64                    # k_wk_sets / k_wk_remove_sets: list entries a step (one wave a set, gd_workers.h)
TC = o.grain_type_code(o.PING_GRAIN_CLASS)
CLIENT = np.uint64(4 << 56)
GUARD = 0xA5


def sizes(t):
    return [t - 1, t, t + 1, 3 * t + 5]


def grains(ids):
    return o.grain_keys(TC, np.asarray(ids))


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


class World:
    """An engine and the reference table beside it."""

    def __init__(self, gd, sc=16, default_ml=3, capacity=48, configure=True):
        self.gd = gd
        self.e = gd.GrainDispatch(device=0, table_capacity=1024)
        if configure:
            self.e.workers_configure(capacity, sc, default_ml)
        self.w = W.Workers(sc, default_ml)
        self.seen = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()

    def see(self, keys):
        for k in np.asarray(keys, dtype=np.uint64).reshape(-1, 3):
            self.seen[tuple(int(x) for x in k)] = True

    def verify(self):
        keys = np.array(list(self.seen), np.uint64).reshape(-1, 3)
        if len(keys):
            for got, want, name in zip(self.e.workers_lookup(keys), self.w.lookup(keys), ("count", "max_local", "list")):
                np.testing.assert_array_equal(got, want, err_msg="lookup " + name)
        sets, cap = self.e.workers_count()
        assert sets == len(self.w.sets)
        return cap

    def add(self, keys, ctx, ml=None):
        self.see(keys)
        want = self.w.add_loop(keys, ctx, ml)
        np.testing.assert_array_equal(self.e.workers_add(keys, ctx, ml), want)
        self.verify()
        return want

    def remove(self, keys, ctx):
        self.see(keys)
        want = self.w.remove_loop(keys, ctx)
        np.testing.assert_array_equal(self.e.workers_remove(keys, ctx), want)
        self.verify()
        return want

    def select(self, keys, ctx_base, fl, nr, wo=None, ml=None, draw=None):
        self.see(keys)
        want = W.select_loop(self.w, keys, ctx_base, fl, nr, wo, ml, draw)
        got = self.e.workers_select(keys, ctx_base, fl, nr, wo, ml, draw)
        for g, x, name in zip(got, want, ("ctx", "pick", "new_idx")):
            np.testing.assert_array_equal(g, x, err_msg=name)
        self.verify()
        return want


def mixed(rng, world, n, n_ctx=300):
    """A random table in `world` (through gd_workers_add) and a batch of n messages over it, new grains and a client."""
    ref, keys, fl, nr, wo = W.random_world(rng, 9, world.w.sc, n_ctx, int(grains([0])[0, 2]))
    for t, (m, lst) in ref.sets.items():
        world.add(np.array([t] * len(lst), np.uint64), lst, np.full(len(lst), m, np.int32))
    pool = np.concatenate([keys, grains(10 ** 6 + np.arange(4)), np.array([[0, 5, CLIENT]], np.uint64)])
    p = rng.random(len(pool)) ** 3
    batch = pool[rng.choice(len(pool), size=n, p=p / p.sum())]
    ml = rng.integers(-1, world.w.sc + 2, n).astype(np.int32)
    draw = rng.integers(0, 1 << 31, n).astype(np.uint32)
    draw[rng.random(n) < 0.05] = 0x7FFFFFFF
    return batch, fl, nr, wo, ml, draw


@pytest.mark.parametrize("n", sorted(set([0, 1, 63, 64, 65] + sizes(WK_TILE) + sizes(WK_SET_NT))))
def test_select_sizes(gd, n):
    rng = np.random.default_rng(n)
    with World(gd) as x:
        batch, fl, nr, wo, ml, draw = mixed(rng, x, n)
        x.select(batch, 7000, fl, nr, wo, ml, draw)
        x.select(batch, 9000, fl, nr, None, None, None)            # no draws: HELD exactly where one is needed


def busy(n_ctx, idle=0):
    fl, nr = np.zeros(n_ctx, np.uint8), np.ones(n_ctx, np.uint32)
    nr[:idle] = 0
    return fl, nr


def test_null_draws_hold_only_where_a_draw_is_read(gd):
    with World(gd) as x:
        x.add(grains([1, 1, 2]), [0, 1, 2], np.array([2, 2, 1], np.int32))
        fl, nr = busy(8)
        _, pick, _ = x.select(grains([1, 2, 1, 2]), 100, fl, nr)
        assert list(pick) == [W.WK_HELD, W.WK_RANDOM, W.WK_HELD, W.WK_RANDOM]        # set 2 has one entry: index 0


def test_client_key_is_none_and_changes_nothing(gd):
    with World(gd) as x:
        x.add(grains([1]), [0])
        keys = np.array([[0, 5, CLIENT], [7, 7, np.uint64(1 << 56)]], np.uint64)
        fl, nr = busy(4)
        ctx, pick, new_idx = x.select(keys, 100, fl, nr)
        assert list(pick) == [W.WK_NONE] * 2 and list(ctx) == [W.NONE32] * 2 and len(new_idx) == 0
        assert x.e.workers_count()[0] == 1


def test_entry_past_n_ctx_is_counted_but_never_idle(gd):
    with World(gd) as x:
        x.add(grains([1, 1]), [1000, 2], np.array([3, 3], np.int32))
        fl, nr = busy(8, idle=8)
        ctx, pick, _ = x.select(grains([1, 1, 1]), 100, fl, nr, draw=np.zeros(3, np.uint32))
        assert list(pick) == [W.WK_IDLE, W.WK_NEW, W.WK_RANDOM] and list(ctx) == [2, 100, 1000]


def hot_world(gd):
    """One set of 100 workers, 70 idle, MaxLocal 170, slot_capacity 256: a = 70, room = 70."""
    x = World(gd, sc=256, default_ml=170)
    ctx = np.arange(100, dtype=np.uint32)
    x.add(grains([1] * 100), ctx, np.full(100, 170, np.int32))
    fl, nr = busy(128)
    nr[np.arange(0, 100)[np.arange(100) % 10 < 7]] = 0             # 70 idle, spread through the list
    return x, fl, nr


def test_one_set_takes_the_whole_batch(gd):
    n = 3 * WK_TILE + 5
    x, fl, nr = hot_world(gd)
    with x:
        draw = np.random.default_rng(3).integers(0, 0x7FFFFFFF, n).astype(np.uint32)
        _, pick, new_idx = x.select(grains([1] * n), 4000, fl, nr, draw=draw)
        assert list(np.bincount(pick, minlength=5)) == [0, 70, 70, n - 140, 0] and len(new_idx) == 70


def test_hot_set_with_every_seventh_message_elsewhere(gd):
    n = 3 * WK_TILE + 5
    x, fl, nr = hot_world(gd)
    with x:
        ids = np.ones(n, np.int64)
        ids[::7] = 50 + np.arange(len(ids[::7])) % 11
        draw = np.random.default_rng(4).integers(0, 0x7FFFFFFF, n).astype(np.uint32)
        x.select(grains(ids), 4000, fl, nr, draw=draw)


def test_every_pick_status_inside_one_wave(gd):
    with World(gd, sc=4, default_ml=2) as x:
        x.add(grains([1, 1]), [0, 1])
        fl, nr = busy(8, idle=1)
        keys = np.concatenate([grains([1, 1, 1, 2]), np.array([[0, 5, CLIENT]], np.uint64), grains([3, 1])])
        ml = np.array([0, 0, 0, 0, 0, 5, 0], np.int32)
        draw = np.array([0, 0x7FFFFFFE, 0x7FFFFFFF, 0, 0, 0, 1], np.uint32)
        _, pick, _ = x.select(keys, 100, fl, nr, None, ml, draw)
        assert list(pick) == [W.WK_IDLE, W.WK_RANDOM, W.WK_HELD, W.WK_NEW, W.WK_NONE, W.WK_HELD, W.WK_RANDOM]


def test_all_new_grains_with_max_local_one(gd):
    n = 300
    with World(gd, sc=2, default_ml=1) as x:
        ctx, pick, new_idx = x.select(grains(1000 + np.arange(n)), 50, np.zeros(0, np.uint8), np.zeros(0, np.uint32))
        assert list(pick) == [W.WK_NEW] * n and list(ctx) == list(range(50, 50 + n)) and list(new_idx) == list(range(n))
        assert x.verify() >= 512                                   # 300 sets: the table grew from 64 slots


def test_new_grain_hit_five_times(gd):
    with World(gd, sc=8, default_ml=3) as x:
        draw = np.array([0, 0, 0, 0x7FFFFFFE, 0x40000000], np.uint32)
        ctx, pick, _ = x.select(grains([9] * 5), 700, np.zeros(0, np.uint8), np.zeros(0, np.uint32), draw=draw)
        assert list(pick) == [W.WK_NEW] * 3 + [W.WK_RANDOM] * 2 and list(ctx) == [700, 701, 702, 702, 701]


def test_max_local_at_and_past_slot_capacity(gd):
    with World(gd, sc=4, default_ml=2) as x:
        ml = np.array([4] * 5 + [5], np.int32)
        ctx, pick, _ = x.select(grains([1] * 5 + [2]), 10, np.zeros(0, np.uint8), np.zeros(0, np.uint32), None, ml,
                                np.zeros(6, np.uint32))
        assert list(pick) == [W.WK_NEW] * 4 + [W.WK_RANDOM, W.WK_HELD]
        assert x.e.workers_count()[0] == 1                         # grain 2 was not created


def test_add_to_full_and_order(gd):
    with World(gd, sc=3, default_ml=2) as x:
        st = x.add(grains([5, 5, 5]), [30, 10, 20])                # three workers of one new grain: order kept
        assert list(st) == [W.WK_ADDED] * 3
        st = x.add(np.concatenate([grains([5, 6, 6, 6, 6, 7]), np.array([[0, 5, CLIENT]], np.uint64)]),
                   [1, 2, 3, 4, 5, 6, 7], np.array([0, 0, 0, 0, 0, 4, 0], np.int32))
        assert list(st) == [W.WK_FULL] + [W.WK_ADDED] * 3 + [W.WK_FULL, W.WK_FULL, W.WK_NOT_GRAIN]


def test_remove(gd):
    with World(gd, sc=8, default_ml=8) as x:
        x.add(grains([1] * 5 + [2]), [10, 11, 12, 13, 14, 20])
        out = x.remove(grains([1, 1, 1]), [13, 10, 11])            # three of five in one batch
        assert list(out) == [1, 1, 1] and x.w.sets[tuple(int(v) for v in grains([1])[0])][1] == [12, 14]
        out = x.remove(grains([1, 1, 2, 3]), [12, 12, 20, 1])      # a duplicate pair; set 2's last worker
        assert list(out) == [1, 0, 1, 0]
        assert x.e.workers_count()[0] == 1
        _, pick, _ = x.select(grains([2]), 500, np.zeros(0, np.uint8), np.zeros(0, np.uint32))
        assert list(pick) == [W.WK_NEW]                            # the set is created again


def test_wrapped_chains_at_load_three_quarters(gd):
    cap = 64
    with World(gd, sc=4, default_ml=2, capacity=48) as x:
        keys = np.concatenate([CK.keys_with_home(TC, cap, 56, 20), CK.keys_with_home(TC, cap, 8, 14),
                               CK.keys_with_home(TC, cap, 32, 14)])
        x.add(keys, np.arange(48, dtype=np.uint32))                # 48 sets in 64 slots; the first chain wraps
        assert x.verify() == cap
        fl, nr = busy(64, idle=30)
        rng = np.random.default_rng(5)
        batch = keys[rng.integers(0, 48, 200)]
        x.select(batch, 1000, fl, nr, draw=rng.integers(0, 0x7FFFFFFF, 200).astype(np.uint32))
        assert x.verify() == cap


def test_tombstone_reuse_then_growth(gd):
    cap = 64
    with World(gd, sc=4, default_ml=2, capacity=48) as x:
        keys = CK.keys_with_home(TC, cap, 56, 24)
        x.add(np.repeat(keys, 2, axis=0), np.arange(48, dtype=np.uint32))
        x.remove(np.repeat(keys[4:16], 2, axis=0), np.arange(8, 32, dtype=np.uint32))      # 12 tombstones in the chain
        more = CK.keys_with_home(TC, cap, 56, 12, start=int(keys[-1, 1]) + 1)
        x.add(more, 100 + np.arange(12, dtype=np.uint32))          # reuses them
        assert x.verify() == cap
        x.add(grains(5000 + np.arange(200)), 1000 + np.arange(200, dtype=np.uint32))
        assert x.verify() > cap                                    # grew; every list intact after the rehash


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def guarded(nbytes):
    import torch
    return torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")


def host(t, dtype, count):
    a = t.cpu().numpy()
    nb = count * np.dtype(dtype).itemsize
    assert (a[nb:] == GUARD).all(), "wrote past its output"
    return a[:nb].view(dtype).copy()


def test_composition_with_turns_and_device_forms(gd):
    import torch
    rng = np.random.default_rng(11)
    n, n_ctx, base = 3 * WK_TILE + 5, 800, 500                    # at most 13 sets x 16 new workers: base + 208 < n_ctx
    with World(gd, sc=16, default_ml=6) as x:
        batch, fl, nr, wo, ml, draw = mixed(rng, x, n, n_ctx=300)
        fl = np.concatenate([fl & 3, np.full(n_ctx - 300, TR.CTX_INVALID, np.uint8)]).astype(np.uint8)
        nr = np.concatenate([nr.view(np.int32).clip(0, 2).astype(np.uint32), np.zeros(n_ctx - 300, np.uint32)])
        wo = np.concatenate([wo, np.full(n_ctx - 300, wo[-1], np.uint32)])
        x.see(batch)
        want = W.select_loop(x.w, batch, base, fl, nr, wo, ml, draw)
        d_k, d_ml, d_draw = dev(batch), dev(ml), dev(draw)
        d_fl, d_nr, d_wo = dev(fl), dev(nr), dev(wo)
        d_ctx, d_pick, d_new, d_nn = guarded(4 * n), guarded(n), guarded(4 * n), guarded(4)
        x.e.workers_select_device(d_k.data_ptr(), n, d_ml.data_ptr(), d_draw.data_ptr(), base, n_ctx, d_fl.data_ptr(),
                                  d_nr.data_ptr(), d_wo.data_ptr(), d_ctx.data_ptr(), d_pick.data_ptr(),
                                  d_new.data_ptr(), d_nn.data_ptr())
        x.e.synchronize()
        n_new = int(host(d_nn, np.uint32, 1)[0])
        assert n_new == len(want[2]) > 0
        np.testing.assert_array_equal(host(d_ctx, np.uint32, n), want[0])
        np.testing.assert_array_equal(host(d_pick, np.uint8, n), want[1])
        np.testing.assert_array_equal(host(d_new, np.uint32, n)[:n_new], want[2])
        x.verify()
        # the host creates the new ActivationData: NOT_READY | STATELESS_WORKER in the flag array before gd_turns
        fl2 = fl.copy()
        fl2[base:base + n_new] = TR.CTX_NOT_READY | TR.CTX_STATELESS_WORKER
        d_fl2 = dev(fl2)
        d_turn, d_nro, d_run = guarded(n), guarded(4 * n_ctx), guarded(4 * n_ctx)
        state = x.e.turn_state_device(d_fl2.data_ptr(), d_nr.data_ptr())
        x.e.turns_device(d_ctx.data_ptr(), None, None, None, None, None, None, None, n, n_ctx, state, d_turn.data_ptr(),
                         d_nro.data_ptr(), d_run.data_ptr())
        x.e.synchronize()
        turn = host(d_turn, np.uint8, n)
        ref = TR.turns_np(TR.Batch(want[0], n_ctx, fl2, nr, np.zeros(n_ctx, np.uint32)))
        np.testing.assert_array_equal(turn, ref[0])
        np.testing.assert_array_equal(host(d_nro, np.uint32, n_ctx), ref[1])
        np.testing.assert_array_equal(host(d_run, np.uint32, n_ctx), ref[2])
        assert (turn[want[1] == W.WK_IDLE] == TR.TURN_START).all() and (want[1] == W.WK_IDLE).any()
        assert (turn[want[1] == W.WK_NEW] == TR.TURN_WAIT).all()
        # add / remove / lookup on device arrays, every output guarded
        keys = grains([900, 900, 901])
        d_k2, d_c2 = dev(keys), dev(np.array([1, 2, 3], np.uint32))
        d_st, d_rm = guarded(3), guarded(3)
        x.e.workers_add_device(d_k2.data_ptr(), d_c2.data_ptr(), None, 3, d_st.data_ptr())
        x.e.workers_remove_device(d_k2.data_ptr(), d_c2.data_ptr(), 2, d_rm.data_ptr())
        d_cnt, d_m, d_lst = guarded(12), guarded(12), guarded(3 * 16 * 4)
        x.e.workers_lookup_device(d_k2.data_ptr(), 3, d_cnt.data_ptr(), d_m.data_ptr(), d_lst.data_ptr())
        x.e.synchronize()
        assert list(host(d_st, np.uint8, 3)) == [W.WK_ADDED] * 3 and list(host(d_rm, np.uint8, 2)) == [1, 1]
        x.see(keys)
        x.w.add_loop(keys, [1, 2, 3])
        x.w.remove_loop(keys[:2], [1, 2])
        assert list(host(d_cnt, np.uint32, 3)) == [0, 0, 1] and list(host(d_m, np.uint32, 3)) == [0, 0, 6]
        lst = host(d_lst, np.uint32, 48).reshape(3, 16)
        assert lst[2, 0] == 3 and (lst.reshape(-1)[np.arange(48) != 32] == W.NONE32).all()
        x.verify()


def test_errors(gd):
    import torch
    k = grains([1, 2, 3])
    z8, z32 = np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    with World(gd, configure=False) as x:
        calls = [lambda: x.e.workers_clear(), lambda: x.e.workers_count(), lambda: x.e.workers_add(k, [1, 2, 3]),
                 lambda: x.e.workers_remove(k, [1, 2, 3]), lambda: x.e.workers_select(k, 0, z8, z32)]
        x.e.workers_slot_capacity = 4
        calls.append(lambda: x.e.workers_lookup(k))
        for c in calls:
            with pytest.raises(gd.GrainDispatchError) as ei:
                c()
            assert ei.value.code == gd.GD_ESTATE
        for sc in (0, 1025):
            with pytest.raises(gd.GrainDispatchError) as ei:
                x.e.workers_configure(16, sc, 1)
            assert ei.value.code == gd.GD_EINVAL
        x.e.workers_configure(16, 4, 2)
        with pytest.raises(gd.GrainDispatchError) as ei:
            x.e.workers_select(k, 0xFFFFFFFD, z8, z32)             # ctx_base overflow
        assert ei.value.code == gd.GD_EINVAL
        d_k, out = dev(k), guarded(64)
        p = out.data_ptr()
        for new_idx, n_new in ((p, None), (None, p)):
            with pytest.raises(gd.GrainDispatchError) as ei:
                x.e.workers_select_device(d_k.data_ptr(), 3, None, None, 0, 0, None, None, None, p, p, new_idx, n_new)
            assert ei.value.code == gd.GD_EINVAL
        assert x.e.workers_count()[0] == 0
        # inside a capture: every batch call is refused and nothing is launched
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        x.e.set_stream(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        codes = []
        with torch.cuda.graph(g, stream=s):
            out.add_(0)
            for c in (lambda: x.e.workers_select_device(d_k.data_ptr(), 3, None, None, 0, 0, None, None, None, p, p),
                      lambda: x.e.workers_add_device(d_k.data_ptr(), p, None, 3, p),
                      lambda: x.e.workers_remove_device(d_k.data_ptr(), p, 3, p), lambda: x.e.workers_select(k, 0, z8, z32)):
                with pytest.raises(gd.GrainDispatchError) as ei:
                    c()
                codes.append(ei.value.code)
        x.e.set_stream(None)
        g.replay()
        torch.cuda.synchronize()
        assert codes == [gd.GD_ESTATE] * 4
        assert x.e.workers_count()[0] == 0 and (host(out, np.uint8, 0) == GUARD).all()
