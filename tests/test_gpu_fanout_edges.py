"""The follower fan-out at its plan, tile and 32-bit boundaries (gd_fanout.h, eng_fanout.hip), bit for bit
against oracle/fanout.py over the case table of _fanout_cases.py (test_fanout_cases.py proves on the CPU
that each case reaches the path it names):

  * the staged / global search on either side of FAN_LDS_ITEMS publishers a block, in both tile forms;
  * rows and totals on, one below and one above the tile edges; the search's 64-piece rounds on either
    side of 64, 64^2 and 64^3 publishers; the three counting plans and where they switch;
  * the 2^32 - 1 rule, by the size query alone (degrees and scan, no expansion: nothing here can make a
    kernel index out of range, whatever the count comes to);
  * the fused route's own probe on OK, MULTI_ACT, invalid-silo, tombstoned, wrapped and absent chains;
  * k_frontier_count's 16-B and scalar paths.

Every output buffer holds a pattern before each run, so an output the kernel skipped shows."""
from functools import lru_cache

import numpy as np
import pytest

import fanout as fo
import oracle as o
import _fanout_cases as fc

pytestmark = pytest.mark.gpu

TC = fc.TC
PATTERN = 0xA5A5A5A5
PROBES = (0, 2, 4)                 # GD_OPT_PROBE: the directory probe, the 16-B index, the 8-B index
N_ACT = fc.N_NODES
HOST_FORM_MAX = 100_000            # cases below this many messages also run through the host-pointer form


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


# ----------------------------------------------------------------------------- references, computed once
@lru_cache(maxsize=None)
def _spec(mode):
    return o.ring_spec(o.bench_silos(8), mode)


def _owner(keys, mode):
    return o.ring_owner_np(_spec(mode), o.jenkins_u64x3_np(keys[:, 2], keys[:, 0], keys[:, 1])).astype(np.uint32)


@lru_cache(maxsize=None)
def _route_table(mode):
    """The oracle's route of GrainId(TC, t) for every follower id t the shared graph names."""
    reg_nodes = fc.registered_nodes()
    reg = o.grain_keys(TC, reg_nodes)
    d = o.DirectoryArrays(reg, reg_nodes.astype(np.uint32), _owner(reg, mode))
    st, silo, act, _, _ = o.route_batch_np(o.grain_keys(TC, np.arange(fc.N_TARGETS)), _spec(mode), d)
    assert (st == o.ST_MISS).sum() > 200 and (st == o.ST_OK).sum() > 3000
    return st, silo, act


def _want(case, mode="D"):
    (ro, dst, fr), _ = case.build()
    t, s = fo.expand(ro, dst, fr)
    st, silo, act = (x[t] for x in _route_table(mode))
    perm, off = o.bucket_stable(act, N_ACT)
    return dict(target=t, sender=s, status=st, silo=silo, act=act, perm=perm, offsets=off)


_shared_want = lru_cache(maxsize=None)(lambda label: _want(fc.BY_LABEL[label]))


# ----------------------------------------------------------------------------- the engine under test
class _Rig:
    def __init__(self, gd, probe, mode="D"):
        import torch
        from orleans_amd.fanout import DeviceFanoutEngine
        self.torch = torch
        reg_nodes = fc.registered_nodes()
        reg = o.grain_keys(TC, reg_nodes)
        self.e = gd.GrainDispatch(device=0, table_capacity=4 * fc.N_NODES, options={"probe": probe})
        self.e.ring_set_silos(mode, [(s.ip, s.port, s.gen) for s in o.bench_silos(8)])
        self.e.register(reg, reg_nodes.astype(np.uint32), _owner(reg, mode))
        self.eng = DeviceFanoutEngine(self.e, torch.device("cuda", 0), TC)

    def close(self):
        self.e.close()

    def dev(self, a):
        a = np.array(a, order="C")                       # a writable copy: the table's arrays are read-only
        return self.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(self.eng.device)

    def filled(self, n, dtype=None):
        torch = self.torch
        if dtype == torch.uint8:
            return torch.full((n,), PATTERN & 0xFF, dtype=torch.uint8, device=self.eng.device)
        return torch.full((n,), PATTERN - (1 << 32), dtype=torch.int32, device=self.eng.device)

    def graph(self, ro, dst):
        from orleans_amd.fanout import upload_graph
        return upload_graph(ro.copy(), dst.copy(), self.eng.device)      # the table's arrays are read-only


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _check_expand(rig, g, fr_t, want):
    """gd_fanout_expand_device: the size query, then k_fan_expand into patterned buffers."""
    m = want["target"].size
    assert rig.eng.count(g, fr_t) == m
    target, sender = rig.filled(m), rig.filled(m)
    got = rig.e.fanout_expand_device(g.row_off.data_ptr(), g.dst.data_ptr(), g.n_nodes, fr_t.data_ptr(),
                                     int(fr_t.shape[0]), target.data_ptr(), sender.data_ptr(), m)
    assert got == m
    np.testing.assert_array_equal(_u32(target), want["target"], err_msg="expand target")
    np.testing.assert_array_equal(_u32(sender), want["sender"], err_msg="expand sender")


def _check_fused(rig, g, fr_t, want, n_act=N_ACT):
    """gd_fanout_route_bucket_device (k_fan_route + the bucketing) into patterned buffers."""
    m = want["target"].size
    b = {k: rig.filled(m) for k in ("target", "sender", "silo", "act", "perm")}
    b["status"] = rig.filled(m, rig.torch.uint8)
    b["offsets"] = rig.filled(n_act + 2)
    got = rig.e.fanout_route_bucket_device(
        g.row_off.data_ptr(), g.dst.data_ptr(), g.n_nodes, fr_t.data_ptr(), int(fr_t.shape[0]), TC, n_act,
        b["target"].data_ptr(), b["sender"].data_ptr(), b["silo"].data_ptr(), b["act"].data_ptr(),
        b["status"].data_ptr(), b["perm"].data_ptr(), b["offsets"].data_ptr(), m)
    assert got == m
    for k in ("target", "sender", "silo", "act", "perm", "offsets"):
        np.testing.assert_array_equal(_u32(b[k]), want[k], err_msg=f"fused {k}")
    np.testing.assert_array_equal(b["status"].cpu().numpy(), want["status"], err_msg="fused status")


def _check_host_form(rig, ro, dst, fr, want, n_act=N_ACT):
    got = rig.e.fanout_route_bucket(ro, dst, fr, TC, n_act)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"host form {k}")


def _run_case(gd, case, probe, want, fused_runs=1):
    (ro, dst, fr), _ = case.build()
    rig = _Rig(gd, probe)
    with rig.eng.context():
        g = rig.graph(ro, dst)
        fr_t = rig.dev(fr)
        _check_expand(rig, g, fr_t, want)
        for _ in range(fused_runs):
            _check_fused(rig, g, fr_t, want)
        if want["target"].size < HOST_FORM_MAX:
            _check_host_form(rig, ro, dst, fr, want)
    rig.close()


# ----------------------------------------------------------------------------- expansion cases
@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("label", [c.label for c in fc.cases("staging") + fc.cases("edges")])
def test_staging_and_tile_edges(gd, label, probe):
    """The 2,048 / 2,049-publisher blocks (staged / global search) in the 512- and 2,048-output forms, at
    block 0 and inside; rows and totals at the tile edges; under each probe form."""
    _run_case(gd, fc.BY_LABEL[label], probe, _shared_want(label))


_WIDTH_CASES = fc.cases("widths")


@pytest.mark.parametrize("label,probe", [(c.label, PROBES[i % 3]) for i, c in enumerate(_WIDTH_CASES)])
def test_search_widths(gd, label, probe):
    """Frontiers of 1 .. 64^3 + 1 publishers: every round count of wave_upper_bound_u32 and both sides
    of each; all-ones frontiers make every piece boundary a search target."""
    case = fc.BY_LABEL[label]
    _run_case(gd, case, probe, _want(case))


@pytest.mark.parametrize("label,probe", [(c.label, p) for c, p in zip(fc.cases("plans"), (0, 4, 2, 0))])
def test_counting_plans(gd, label, probe):
    """2^21 (narrow), 2^21 + 1 and 2^24 (wide), 2^24 + 1 (slow: u64 atomics and the two-level scan)."""
    case = fc.BY_LABEL[label]
    _run_case(gd, case, probe, _want(case))


# ----------------------------------------------------------------------------- the 32-bit limit
@pytest.mark.parametrize("label", list(fc.LIMITS))
def test_fanout_of_2_32_messages_is_refused(gd, label):
    """gd_fanout_expand_device with null outputs (degrees + scan only).  2^32 - 1 messages are counted;
    2^32 are refused with GD_EINVAL -- also when they all fall into one degree tile, whose u32 sum is 0."""
    import torch
    from orleans_amd.fanout import DeviceFanoutEngine, upload_graph
    (ro, dst, fr), _ = fc.limit_case(label)
    accepted = fc.LIMITS[label][3]
    e = gd.GrainDispatch(device=0, table_capacity=1024)
    eng = DeviceFanoutEngine(e, torch.device("cuda", 0), TC)
    with eng.context():
        g = upload_graph(ro, dst, eng.device)
        fr_t = torch.from_numpy(fr.view(np.int32)).to(eng.device)
        if accepted:
            assert eng.count(g, fr_t) == 4_294_967_295
        else:
            with pytest.raises(gd.GrainDispatchError) as ei:
                got = eng.count(g, fr_t)
                print(f"{label}: size query returned {got} with no error")
            assert ei.value.code == gd.GD_EINVAL
        # the handle still counts an ordinary hop afterwards
        assert eng.count(g, torch.tensor([1, 5, 0], dtype=torch.int32, device=eng.device)) == 2 * fc.BIG_ROW - 1
    e.close()


# ----------------------------------------------------------------------------- probe states
@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("mode", ["D", "R", "V"])
def test_fused_route_probe_states(gd, mode, probe):
    """k_fan_route (and k_route_nodes) on a 2,048-slot directory with a chain wrapped over the table end
    and one mid-table, tombstones inside both, multi-activation grains, an invalid silo and absent ids
    of the same homes."""
    import torch
    from orleans_amd.fanout import DeviceFanoutEngine, upload_graph
    w = fc.probe_world(mode)
    want = w["want"]
    e = gd.GrainDispatch(device=0, table_capacity=fc.PROBE_CAP, options={"probe": probe})
    e.ring_set_silos(mode, [(s.ip, s.port, s.gen) for s in w["silos"]])
    _, _, ins = e.register(w["reg"], w["reg_act"], w["reg_silo"])
    assert ins.all()
    rem = e.unregister(w["gone"], w["gone_act"])
    assert np.asarray(rem).all()
    e.upsert(w["multi"], np.full(len(w["multi"]), gd.GD_ACT_MULTI, np.uint32), w["multi_silo"])
    e.set_valid_silos([s for s in range(8) if s != fc.PROBE_INVALID_SILO], 8)
    st = e.stats()
    assert st["table_capacity"] == fc.PROBE_CAP and st["table_tombstones"] == len(w["gone"])
    assert st["table_live"] == len(w["reg"]) - len(w["gone"])
    rig = _Rig.__new__(_Rig)
    rig.torch, rig.e = torch, e
    rig.eng = DeviceFanoutEngine(e, torch.device("cuda", 0), TC)
    with rig.eng.context():
        g = upload_graph(w["row_off"], w["dst"], rig.eng.device)
        fr_t = rig.dev(w["frontier"])
        _check_expand(rig, g, fr_t, want)
        for _ in range(2):                       # right after the directory batches, and settled
            _check_fused(rig, g, fr_t, want, fc.PROBE_N_ACT)
        _check_host_form(rig, w["row_off"], w["dst"], w["frontier"], want, fc.PROBE_N_ACT)
        s2, silo, act, perm, off = rig.eng.route_nodes_bucket(rig.dev(want["target"]), fc.PROBE_N_ACT)
        np.testing.assert_array_equal(s2.cpu().numpy(), want["status"])
        for got, k in ((silo, "silo"), (act, "act"), (perm, "perm"), (off, "offsets")):
            np.testing.assert_array_equal(_u32(got), want[k], err_msg=f"route_nodes {k}")
    assert e.stats()["table_capacity"] == fc.PROBE_CAP
    e.close()


# ----------------------------------------------------------------------------- next frontier
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset"])
@pytest.mark.parametrize("n_act", fc.FRONTIER_N_ACT)
def test_frontier_next_paths(gd, n_act, aligned):
    """k_frontier_count's 16-B path (16 activations left, both pointers 16-B aligned) and its scalar
    path (the tail, or offsets[1:] / visited[1:] views); guard bytes around visited stay untouched."""
    import torch
    from orleans_amd.fanout import DeviceFanoutEngine
    off, visited, _ = fc.frontier_case(n_act)
    e = gd.GrainDispatch(device=0, table_capacity=1024)
    eng = DeviceFanoutEngine(e, torch.device("cuda", 0), TC)
    lead = 0 if aligned else 1
    with eng.context():
        off_full = torch.zeros(lead + n_act + 2, dtype=torch.int32, device=eng.device)
        vis_full = torch.zeros(lead + n_act + 16, dtype=torch.uint8, device=eng.device)
        off_t, vis_t = off_full[lead:], vis_full[lead:]
        off_t.copy_(torch.from_numpy(off.view(np.int32)))
        vis_t[:n_act].copy_(torch.from_numpy(visited.astype(np.uint8)))
        assert (off_t.data_ptr() % 16 == 0) == aligned and (vis_t.data_ptr() % 16 == 0) == aligned
        fr = eng.frontier_next(off_t, n_act, vis_t)
        vis2 = visited.copy()
        want = fo.next_frontier(off, n_act, vis2)
        np.testing.assert_array_equal(_u32(fr), want)
        got_vis = vis_full.cpu().numpy()
        np.testing.assert_array_equal(got_vis[lead:lead + n_act].astype(bool), vis2)
        assert got_vis[lead:lead + n_act].max() <= 1
        assert not got_vis[:lead].any() and not got_vis[lead + n_act:].any()
        # a second call finds nothing new
        assert eng.frontier_next(off_t, n_act, vis_t).shape[0] == 0
        np.testing.assert_array_equal(vis_full.cpu().numpy(), got_vis)
    e.close()
