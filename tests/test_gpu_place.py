"""GPU parity for the batched placement of unregistered grains: gd_route_place / gd_route_place_bucket through
the C ABI against the literal restatement of the reference's slow path (_place_ref.py place_loop), bit for
bit: status, silo, act, place status, new_idx, n_new, n_proposed, and perm / offsets for the bucket forms.
After each call the directory (gd_dir_lookup of every key of the batch) equals the reference directory and a
plain gd_route of the same keys gives the reference's routes, so the probe indexes were re-projected."""
import numpy as np
import pytest

import _place_ref as P
import oracle as o
from dirstate import DirectoryState

pytestmark = pytest.mark.gpu

T = 4096                          # k_place_mark's messages per workgroup (orleans_amd/csrc/gd_place.h PL_TILE)
CAP = 4096
MY, SEED = 2, 6
TC = o.grain_type_code(o.PING_GRAIN_CLASS)
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


class World:
    """An engine, the reference directory beside it and the placement configuration of both."""

    def __init__(self, gd, silos=None, compatible=None, local_active=True, cap=CAP, n_reg=300, multi=True,
                 configure=True, **kw):
        self.silos = silos or o.bench_silos(8)
        self.spec = o.ring_spec(self.silos, "D")
        self.tuples = [(s.ip, s.port, s.gen) for s in self.silos]
        self.e = gd.GrainDispatch(device=0, table_capacity=cap, my_silo=MY, seed_silo=SEED, **kw)
        self.e.ring_set_silos("D", self.tuples)
        self.d = DirectoryState()
        self.configure(compatible, local_active, call=configure)
        if n_reg:
            reg = o.grain_keys(TC, np.arange(n_reg))
            acts = np.arange(n_reg, dtype=np.uint32)
            if multi:
                acts[::17] = o.ACT_MULTI
            host = (np.arange(n_reg) % len(self.silos)).astype(np.uint32)
            self.e.upsert(reg, acts, host)
            self.d.upsert(reg, acts, host)

    def configure(self, compatible=None, local_active=True, call=True):
        self.cfg = P.PlaceConfig(self.silos, compatible, local_active, my_silo=MY)
        if call:
            self.e.place_configure(self.tuples, compatible, local_active)

    def set_valid(self, valid, n):
        self.e.set_valid_silos(valid, n)
        self.d.set_valid(valid, n)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()

    def check_directory(self, keys):
        """gd_dir_lookup of every key of the batch, and a plain route of the batch, against the reference."""
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
        if not len(keys):
            return
        plain = keys[(keys[:, 2] >> np.uint64(56)) == o.CAT_GRAIN]
        if len(plain):
            act, silo, found = self.e.lookup(plain)
            want = self.d.lookup_tagged(plain)
            ok = np.array([w[3] != 2 for w in want])       # 2: an entry on an invalid silo (no new entry is)
            np.testing.assert_array_equal((found != 0)[ok], np.array([w[3] == 1 for w in want])[ok])
            np.testing.assert_array_equal(act[ok], np.array([w[0] for w in want], np.uint32)[ok])
            np.testing.assert_array_equal(silo[ok], np.array([w[1] for w in want], np.uint32)[ok])
        for got, want, name in zip(self.e.route(keys), P.route_of(keys, self.spec, self.d, MY, SEED),
                                   ("status", "silo", "act")):
            np.testing.assert_array_equal(got, want, err_msg="route after: " + name)

    def run(self, keys, strategy=P.PLACE_HASH, given=None, act_base=1000, n_act=None):
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
        route = P.route_of(keys, self.spec, self.d, MY, SEED)
        want = P.place_loop(keys, route, strategy, given, act_base, self.cfg, self.d)
        if n_act is None:
            got = self.e.route_place(keys, act_base, strategy, given)
        else:
            got = self.e.route_place_bucket(keys, n_act, act_base, strategy, given)
            want = want + o.bucket_stable(want[2], n_act)
        for name, a, b in zip(("status", "silo", "act", "placed", "new_idx", "n_proposed", "perm", "offsets"), got, want):
            if name == "n_proposed":
                assert a == b, name
                continue
            assert a.dtype == b.dtype, name
            np.testing.assert_array_equal(a, b, err_msg=name)
        self.check_directory(keys)
        return got


def _new_keys(ids):
    return o.grain_keys(TC, 100000 + np.asarray(ids))


def _batch(rng, n, share):
    """n messages to registered grains; share 'none' / 'one' / 'all' of them to new grains (with repeats)."""
    ids = rng.integers(0, 300, size=n)
    keys = o.grain_keys(TC, ids)
    if share == "one" and n:
        keys[n // 2] = _new_keys([7])[0]
    if share == "all" and n:
        keys = _new_keys(rng.integers(0, max(1, n // 3), size=n))
    return keys


@pytest.mark.parametrize("share", ["none", "one", "all"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_shapes(gd, n, share):
    rng = np.random.default_rng(n * 7 + len(share))
    cap = CAP if share != "all" or n < T else 4 * CAP
    with World(gd, cap=cap) as w:
        st, silo, act, placed, new_idx, n_prop = w.run(_batch(rng, n, share))
        if share == "none" or n == 0:
            assert n_prop == 0 and len(new_idx) == 0
        elif share == "one":
            assert n_prop == 1 and new_idx.tolist() == [n // 2]
        else:
            assert n_prop == n and 0 < len(new_idx) <= n


@pytest.mark.parametrize("probe", [0, 2, 4])
def test_duplicates_one_grain_every_message(gd, probe):
    n = 3 * T + 17
    with World(gd, options={"probe": probe}) as w:
        live = w.e.stats()["table_live"]
        st, silo, act, placed, new_idx, n_prop = w.run(np.repeat(_new_keys([5]), n, axis=0))
        assert new_idx.tolist() == [0] and n_prop == n
        assert (placed[1:] == P.PLACED_JOINED).all() and (act == 1000).all()
        assert w.e.stats()["table_live"] == live + 1


@pytest.mark.parametrize("no_lane_order", [False, True])
def test_duplicates_across_waves_and_tiles(gd, no_lane_order):
    """One new grain's messages in different lanes, waves and tiles, between other new grains; the first message
    of another new grain skipped (strategy NONE) and a later one placing."""
    rng = np.random.default_rng(3)
    n = 3 * T + 17
    keys = _batch(rng, n, "none")
    strat = np.full(n, P.PLACE_HASH, np.uint8)
    a, b = _new_keys([1])[0], _new_keys([2])[0]
    for i in (5, 64 + 9, 1024 + 3, T - 1, T, T + 700, 3 * T + 16):
        keys[i] = a
    for i in (2, 70, 2 * T + 1):
        keys[i] = b
    strat[2] = P.PLACE_NONE
    others = rng.choice(np.setdiff1d(np.arange(100, n), [1027, T - 1, T, T + 700, 2 * T + 1, 3 * T + 16]), 200,
                        replace=False)
    keys[others] = _new_keys(10 + rng.integers(0, 80, size=200))
    with World(gd, no_lane_order=no_lane_order) as w:
        st, silo, act, placed, new_idx, n_prop = w.run(keys, strat)
        assert placed[2] == P.PLACED_SKIPPED and st[2] == o.ST_MISS and placed[70] == P.PLACED_NEW
        assert placed[5] == P.PLACED_NEW and (placed[[73, 1027, T - 1, T, T + 700, 3 * T + 16]] == P.PLACED_JOINED).all()
        assert len(set(act[[5, 73, 1027, T - 1, T, T + 700, 3 * T + 16]].tolist())) == 1


def _mixed(rng, n, n_silos=8):
    keys = P.mixed_keys(rng, n, TC, 300)
    strat = rng.integers(0, 5, size=n).astype(np.uint8)      # 4: no known value
    given = rng.integers(0, n_silos + 2, size=n).astype(np.uint32)
    given[rng.random(n) < 0.02] = P.NO_SILO
    return keys, strat, given


@pytest.mark.parametrize("probe,no_lane_order", [(0, False), (2, False), (4, False), (1, True)])
def test_mixed_strategies_per_message(gd, probe, no_lane_order):
    rng = np.random.default_rng(11 + probe)
    compatible = np.ones(8, np.uint8)
    compatible[[1, 5]] = 0
    with World(gd, compatible=compatible, options={"probe": probe}, no_lane_order=no_lane_order) as w:
        w.set_valid([0, 1, 2, 4, 6], 7)
        keys, strat, given = _mixed(rng, 2 * T + 333)
        st, silo, act, placed, new_idx, n_prop = w.run(keys, strat, given)
        assert set(np.unique(placed).tolist()) == {0, 1, 2, 3} and n_prop > len(new_idx) > 0


@pytest.mark.parametrize("strategy", [P.PLACE_NONE, P.PLACE_HASH, P.PLACE_LOCAL, P.PLACE_GIVEN])
def test_one_strategy_for_the_batch(gd, strategy):
    rng = np.random.default_rng(20 + strategy)
    with World(gd) as w:
        keys, _, given = _mixed(rng, T + 77)
        st, silo, act, placed, new_idx, n_prop = w.run(keys, strategy, given)
        assert (n_prop == 0) == (strategy == P.PLACE_NONE)
        if strategy == P.PLACE_LOCAL:
            assert (silo[placed == P.PLACED_NEW] == MY).all()


@pytest.mark.parametrize("with_given", [False, True])
def test_local_with_the_local_silo_inactive(gd, with_given):
    rng = np.random.default_rng(31)
    with World(gd, local_active=False) as w:
        keys, _, given = _mixed(rng, T + 5)
        st, silo, act, placed, new_idx, n_prop = w.run(keys, P.PLACE_LOCAL, given if with_given else None)
        assert (n_prop > 0) == with_given and (placed == P.PLACED_SKIPPED).any()
    with World(gd, compatible=[1, 1, 0, 1, 1, 1, 1, 1]) as w:    # active, but the local silo cannot host the class
        assert w.run(_new_keys(np.arange(50)), P.PLACE_LOCAL, np.full(50, 4, np.uint32))[5] == 50


@pytest.mark.parametrize("n_comp", [1, 2, 7, 300])
def test_hash_over_compatible_sets(gd, n_comp):
    """HASH over 1, 2, 7 and 300 compatible silos out of a table that holds more, in an order that is not the
    index order (addresses, ports and generations differ)."""
    n_silos = n_comp + 3
    silos = [o.Silo(f"10.{i % 3}.{(i * 7) % 200}.{250 - i % 250}", 11111 + i % 3, 1 + (i * 5) % 4) for i in range(n_silos)]
    compatible = np.ones(n_silos, np.uint8)
    compatible[[0, n_silos // 2, n_silos - 1]] = 0
    rng = np.random.default_rng(n_comp)
    with World(gd, silos=silos, compatible=compatible) as w:
        assert len(w.cfg.sorted) == n_comp
        st, silo, act, placed, new_idx, n_prop = w.run(_new_keys(rng.integers(0, 1500, size=2000)), P.PLACE_HASH)
        used = set(silo[placed == P.PLACED_NEW].tolist())
        assert used <= set(w.cfg.sorted) and len(used) >= min(n_comp, 7)


def test_skips_register_nothing(gd):
    keys = _new_keys(np.arange(40))
    client = np.array([[7, 11, o.type_code_data(o.CAT_CLIENT, 0)]] * 3, np.uint64)
    cases = [dict(given=np.full(40, 8, np.uint32)),                                   # >= n_silos
             dict(given=np.full(40, 3, np.uint32), compatible=[1, 1, 1, 0, 1, 1, 1, 1]),   # not compatible
             dict(given=np.full(40, 3, np.uint32), valid=[0, 1, 2, 4, 5, 6, 7]),      # invalid
             dict(given=np.full(40, 1, np.uint32), compatible=[0] * 8)]               # empty compatible set
    for c in cases:
        with World(gd, compatible=c.get("compatible")) as w:
            if "valid" in c:
                w.set_valid(c["valid"], 8)
            live = w.e.stats()["table_live"]
            empty = "compatible" in c and not any(c["compatible"])
            for strategy in (P.PLACE_GIVEN, P.PLACE_HASH, P.PLACE_LOCAL) if empty else (P.PLACE_GIVEN,):
                st, silo, act, placed, new_idx, n_prop = w.run(keys, strategy, c["given"])
                assert (st == o.ST_MISS).all() and (placed == P.PLACED_SKIPPED).all() and n_prop == 0
            assert w.e.stats()["table_live"] == live
    with World(gd) as w:
        live = w.e.stats()["table_live"]
        st, silo, act, placed, new_idx, n_prop = w.run(client, P.PLACE_HASH)
        assert (st == o.ST_MISS).all() and (placed == P.PLACED_NONE).all() and n_prop == 0
        assert w.e.stats()["table_live"] == live


def test_untouched_rows_equal_gd_route(gd):
    """System targets, the membership grain, KeyExt, MULTI_ACT and hits keep what gd_route gives on a second
    engine that never places."""
    rng = np.random.default_rng(41)
    keys = P.mixed_keys(rng, T + 200, TC, 300, new_share=0.2)
    with World(gd) as w, World(gd, configure=False) as plain:
        r_st, r_silo, r_act = plain.e.route(keys)
        assert {o.ST_OK, o.ST_MISS, o.ST_SYSTEM_TARGET, o.ST_MEMBERSHIP, o.ST_KEYEXT, o.ST_MULTI_ACT} <= set(r_st.tolist())
        st, silo, act, placed, new_idx, n_prop = w.run(keys, P.PLACE_HASH)
        same = placed == P.PLACED_NONE
        assert same.sum() > T // 2 and (~same).any()
        np.testing.assert_array_equal(st[same], r_st[same])
        np.testing.assert_array_equal(silo[same], r_silo[same])
        np.testing.assert_array_equal(act[same], r_act[same])
        before = w.e.stats()["routed"]
        w.run(keys, P.PLACE_HASH, act_base=5000)
        assert w.e.stats()["routed"] - before == 2 * len(keys)     # the placing call once, check_directory's route once


def test_probe_4_one_class_short_keys(gd):
    """GD_OPT_PROBE 4, one class, N1 < 2^32: the 8-B index takes the new entries (their numbers fit the 12
    activation bits the index was laid out with); wider numbers stay in the directory and route the same."""
    rng = np.random.default_rng(43)
    with World(gd, cap=1 << 14, n_reg=3000, multi=False, options={"probe": 4}) as w:
        keys = o.grain_keys(TC, rng.integers(0, 3100, size=T + 99))
        w.e.route(keys)
        st, silo, act, placed, new_idx, n_prop = w.run(keys, P.PLACE_HASH, act_base=3000)
        assert 50 < len(new_idx) <= 100 and act.max() < 4000
        stats = w.e.index_stats()
        assert stats["current"] == 1 and stats["synced_slots"] > 0 and stats["out8"] == 0
        w.run(o.grain_keys(TC, rng.integers(0, 6000, size=T + 99)), P.PLACE_LOCAL, act_base=9000)


def _cxd_builds(e):
    return e.kernel_times().get("k_cxd_build", (0, 0.0))[0]     # as tests/test_gpu_direct.py counts them


def test_direct_table_then_place_then_route(gd):
    rng = np.random.default_rng(47)
    with World(gd, cap=1 << 14, n_reg=6000, multi=False, options={"probe": 4}) as w:
        w.e.set_kernel_timing(True)
        q = o.grain_keys(TC, rng.integers(0, 6300, size=20001))
        w.e.stats()
        w.check_directory(q)
        w.check_directory(q)
        assert _cxd_builds(w.e) == 1                             # the direct table is in use
        st, silo, act, placed, new_idx, n_prop = w.run(q, P.PLACE_HASH, act_base=7000)
        assert len(new_idx) > 100
        w.check_directory(q)                                     # the routes follow the directory
        w.check_directory(q)


def test_sequence_with_unregister_in_between(gd):
    rng = np.random.default_rng(53)
    with World(gd) as w:
        base = 1000
        got = w.run(_new_keys(rng.integers(0, 400, size=T + 50)), P.PLACE_HASH, act_base=base)
        base += got[5]
        placed_keys = _new_keys(np.arange(0, 400, 3))
        acts = np.array([w.d.entries.get(tuple(int(x) for x in k), [M32])[0] for k in placed_keys], np.uint32)
        removed = w.e.unregister(placed_keys, acts)
        np.testing.assert_array_equal(removed, np.array(w.d.unregister(placed_keys, acts), np.uint8))
        assert removed.sum() > 50
        keys, strat, given = _mixed(rng, T + 9)
        keys[::4] = _new_keys(rng.integers(0, 400, size=len(keys[::4])))
        got = w.run(keys, strat, given, act_base=base)
        base += got[5]
        got = w.run(_new_keys(rng.integers(300, 700, size=900)), P.PLACE_LOCAL, act_base=base)
        assert 0 < got[5] < 900 and got[2][got[4]].min() >= base      # ids 300..399 are registered by now: hits


def test_growth_inside_the_directory_batch(gd):
    with World(gd, n_reg=1000) as w:
        assert w.e.stats()["table_capacity"] == CAP
        st, silo, act, placed, new_idx, n_prop = w.run(_new_keys(np.arange(5000) % 3500), P.PLACE_HASH)
        assert len(new_idx) == 3500 and w.e.stats()["table_capacity"] > CAP


@pytest.mark.parametrize("n_act_at", ["below", "at", "above"])
def test_bucket_form(gd, n_act_at):
    rng = np.random.default_rng(59)
    keys, strat, given = _mixed(rng, 2 * T + 100)
    act_base = 400
    with World(gd) as w0:
        acts = w0.run(keys, strat, given, act_base=act_base)[2]
        largest = int(acts[(acts != M32) & (acts >= act_base)].max())
    n_act = {"below": largest - 50, "at": largest, "above": largest + 10}[n_act_at]
    with World(gd) as w:
        got = w.run(keys, strat, given, act_base=act_base, n_act=n_act)
        off = got[7]
        assert off[-1] == len(keys) and (off[n_act + 1] - off[n_act] > 0)


def test_device_forms_agree_with_host_forms(gd):
    import torch
    rng = np.random.default_rng(61)
    keys, strat, given = _mixed(rng, 2 * T + 41)
    n, n_act, act_base = len(keys), 2000, 500
    dev = torch.device("cuda:0")
    with World(gd) as wh, World(gd) as wd:
        want = wh.run(keys, strat, given, act_base=act_base, n_act=n_act)
        d_keys = torch.from_numpy(keys.view(np.int64)).to(dev)
        d_strat = torch.from_numpy(strat).to(dev)
        d_given = torch.from_numpy(given.view(np.int32)).to(dev)
        i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)
        d_silo, d_act, d_new, d_perm, d_off = i32(n), i32(n), i32(n), i32(n), i32(n_act + 2)
        d_st = torch.empty(n, dtype=torch.uint8, device=dev)
        d_pl = torch.empty(n + 1, dtype=torch.uint8, device=dev)[1:]      # a place-status array that is not 16-B aligned
        torch.cuda.synchronize()
        n_new, n_prop = wd.e.route_place_device(d_keys.data_ptr(), n, d_strat.data_ptr(), 0, d_given.data_ptr(), act_base,
                                                d_silo.data_ptr(), d_act.data_ptr(), d_st.data_ptr(), d_pl.data_ptr(),
                                                d_new.data_ptr(), n_act, d_perm.data_ptr(), d_off.data_ptr())
        wd.e.synchronize()
        u32 = lambda t: t.cpu().numpy().view(np.uint32)
        got = (d_st.cpu().numpy(), u32(d_silo), u32(d_act), d_pl.cpu().numpy(), u32(d_new)[:n_new], n_prop, u32(d_perm),
               u32(d_off))
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        # without new_idx and without the bucketing: the same counts
        keys2 = _new_keys(rng.integers(2000, 2300, size=n))
        d_keys2 = torch.from_numpy(keys2.view(np.int64)).to(dev)
        torch.cuda.synchronize()
        n_new2, n_prop2 = wd.e.route_place_device(d_keys2.data_ptr(), n, None, P.PLACE_HASH, None, 9000, d_silo.data_ptr(),
                                                  d_act.data_ptr(), d_st.data_ptr(), d_pl.data_ptr(), None)
        want2 = wh.run(keys2, P.PLACE_HASH, None, act_base=9000)
        assert (n_new2, n_prop2) == (len(want2[4]), want2[5])
        np.testing.assert_array_equal(u32(d_act), want2[2])
        np.testing.assert_array_equal(d_pl.cpu().numpy(), want2[3])


def test_errors(gd):
    import torch
    keys = _new_keys(np.arange(10))
    with World(gd, configure=False) as w:
        with pytest.raises(gd.GrainDispatchError) as ei:
            w.e.route_place(keys, 0)
        assert ei.value.code == gd.GD_ESTATE and "gd_place_configure" in str(ei.value)
        with pytest.raises(gd.GrainDispatchError) as ei:
            w.e.place_configure([], None)
        assert ei.value.code == gd.GD_EINVAL
    with World(gd) as w:
        before = dict(w.d.entries)
        live = w.e.stats()["table_live"]
        with pytest.raises(gd.GrainDispatchError) as ei:
            w.e.route_place(keys, o.ACT_MULTI - 9)               # the tenth proposal would be GD_ACT_MULTI
        assert ei.value.code == gd.GD_EINVAL
        assert w.e.stats()["table_live"] == live and w.d.entries == before
        w.check_directory(keys)
        got = w.run(keys, act_base=o.ACT_MULTI - 10)             # ... and one lower fits
        assert got[2].max() == o.ACT_MULTI - 1
        # inside a stream capture the call is refused before anything is launched
        dev = torch.device("cuda:0")
        d_keys = torch.from_numpy(_new_keys(np.arange(50, 60)).view(np.int64)).to(dev)
        outs = [torch.zeros(16, dtype=torch.int32, device=dev) for _ in range(3)]
        d_st = torch.zeros(16, dtype=torch.uint8, device=dev)
        d_pl = torch.zeros(16, dtype=torch.uint8, device=dev)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        w.e.set_stream(s.cuda_stream)
        w.e.set_kernel_timing(True)
        w.e.kernel_times_reset()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            outs[2].add_(1)                                      # the capture holds one node of the test's own
            with pytest.raises(gd.GrainDispatchError) as ei:
                w.e.route_place_device(d_keys.data_ptr(), 10, None, P.PLACE_HASH, None, 0, outs[0].data_ptr(),
                                       outs[1].data_ptr(), d_st.data_ptr(), d_pl.data_ptr(), outs[2].data_ptr())
            code = ei.value.code
        w.e.set_stream(None)
        assert code == gd.GD_ESTATE
        assert not any(k.startswith("k_") for k in w.e.kernel_times())
        w.check_directory(_new_keys(np.arange(50, 60)))


def test_one_larger_run_against_the_numpy_form(gd):
    """1M messages over 2^18 grains, 1 % of the grains unregistered, a 2^19-slot table: every output against
    place_np, then the directory by a route of the batch."""
    rng = np.random.default_rng(67)
    G, n = 1 << 18, 1 << 20
    with World(gd, cap=1 << 19, n_reg=0) as w:
        ids = np.arange(G)
        reg_ids = ids[rng.random(G) >= 0.01]
        reg = o.grain_keys(TC, reg_ids)
        acts = np.arange(len(reg), dtype=np.uint32)
        host = (reg_ids % 8).astype(np.uint32)
        w.e.register(reg, acts, host)
        w.d.entries = {k: [int(a), int(s), 0, True] for k, a, s in
                       zip(map(tuple, reg.tolist()), acts.tolist(), host.tolist())}
        keys = o.grain_keys(TC, rng.integers(0, G, size=n))
        route = P.route_of(keys, w.spec, w.d, MY, SEED)
        want = P.place_np(keys, route, P.PLACE_HASH, None, G, w.cfg, w.d)
        got = w.e.route_place(keys, G, P.PLACE_HASH)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        assert 2000 < len(got[4]) < 3500 and got[5] > 3 * len(got[4])
        for a, b in zip(w.e.route(keys), P.route_of(keys, w.spec, w.d, MY, SEED)):
            np.testing.assert_array_equal(a, b)
