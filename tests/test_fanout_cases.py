"""CPU proof that the fan-out case table (_fanout_cases.py) hits what it claims: the staging counts on
either side of FAN_LDS_ITEMS in both tile forms, every listed total and frontier length, the counting
plan each long frontier lands in, the 2^32 - 1 / 2^32 sums and where they sit, the probe states of the
directory world, and the two oracle forms agreeing on every small case."""
import numpy as np
import pytest

import fanout as fo
import oracle as o
import _fanout_cases as fc


def _total(case):
    (ro, dst, fr), _ = case.build()
    return int(fc.degrees(ro, fr).sum())


def test_labels_and_graph():
    ro, dst = fc.graph()
    assert len(ro) == fc.N_NODES + 1 and ro[-1] == len(dst) and dst.max() < fc.N_TARGETS
    for u, d in fc.SPECIAL.items():
        assert int(ro[u + 1]) - int(ro[u]) == d
    for c in fc.CASES:
        (ro2, dst2, fr), label = c.build()
        assert label == c.label and fr.dtype == np.uint32 and ro2 is ro and dst2 is dst
    assert fc.SMALL_FORM_MAX == 2_095_104
    assert fc.route_tile(fc.SMALL_FORM_MAX) == 512 and fc.route_tile(fc.SMALL_FORM_MAX + 1) == 2048


@pytest.mark.parametrize("form,tile", [("small", fc.FAN_SMALL_TILE), ("large", fc.FAN_TILE)])
def test_staging_cases_sit_on_both_sides_of_the_boundary(form, tile):
    want = {fc.FAN_LDS_ITEMS - 2: fc.FAN_LDS_ITEMS, fc.FAN_LDS_ITEMS - 1: fc.FAN_LDS_ITEMS + 1}
    for z, cnt in want.items():
        case = fc.BY_LABEL[f"staging-{form}-z{z}"]
        (ro, dst, fr), _ = case.build()
        total = _total(case)
        assert fc.route_tile(total) == tile
        assert (total <= fc.SMALL_FORM_MAX) == (form == "small")
        counts = fc.block_counts(ro, fr, tile)
        assert counts[0] == cnt and counts[fc.INTERIOR_BLOCK] == cnt
        assert 0 < fc.INTERIOR_BLOCK < len(counts) - 1
        # no other block is near the boundary: the two named blocks are what the case tests
        others = np.delete(counts, [0, fc.INTERIOR_BLOCK])
        assert (others < fc.FAN_LDS_ITEMS // 2).all()
    assert want == {2046: 2048, 2047: 2049}


def test_tile_edge_cases():
    for form, tile in (("small", fc.FAN_SMALL_TILE), ("large", fc.FAN_TILE)):
        case = fc.BY_LABEL[f"edges-{form}"]
        (ro, dst, fr), _ = case.build()
        deg = fc.degrees(ro, fr)
        ends = np.cumsum(deg)
        assert fc.route_tile(int(ends[-1])) == tile
        nz = deg > 0
        assert ((ends[nz] % tile) == 0).sum() >= 2                        # rows ending on a block edge
        assert {tile - 1, tile, tile + 1} <= set(deg.tolist())
        assert {511, 512, 513, 2047, 2048, 2049} <= set(deg.tolist())     # both tile sizes, in either form
        first_block = (ends - deg) // tile
        last_block = (ends - 1) // tile
        assert (last_block[nz] - first_block[nz] >= 2).any()              # one row over three blocks
        for pos in (0, len(fr) - 1):
            assert deg[pos] == 0
        mid = np.arange(1, len(fr) - 1)
        assert (fr[mid] >= fc.N_NODES).any() and ((fr[mid] < fc.N_NODES) & (deg[mid] == 0)).any()
        assert {fc.N_NODES, fc.U32_MAX} <= set(fr.tolist())
        assert len(np.unique(fr[nz])) < nz.sum()                           # duplicated publishers
    assert {int(fr[0]) for fr in (fc.BY_LABEL["edges-small"].build()[0][2],
                                  fc.BY_LABEL["edges-large"].build()[0][2])} == {fc.N_NODES, fc.U32_MAX}


def test_every_listed_total_and_length_is_present():
    assert fc.TOTALS == (1, 511, 512, 513, 2047, 2048, 2049, 2_095_104, 2_095_105)
    for t in fc.TOTALS:
        assert _total(fc.BY_LABEL[f"total-{t}"]) == t
    assert fc.WIDTHS == (1, 2, 63, 64, 65, 4095, 4096, 4097, 262_143, 262_144, 262_145)
    for n in fc.WIDTHS:
        (ro, dst, fr), _ = fc.BY_LABEL[f"width-mixed-{n}"].build()
        assert len(fr) == n and set(fc.degrees(ro, fr).tolist()) <= {0, 1, 3}
        if n >= 63:
            assert set(fc.degrees(ro, fr).tolist()) == {0, 1, 3}
        (ro, dst, fr), _ = fc.BY_LABEL[f"width-ones-{n}"].build()
        assert len(fr) == n and (fc.degrees(ro, fr) == 1).all()


def test_counting_plan_cases_land_in_the_plan_named():
    def plan(nf):                              # eng_fanout.hip fan_count, restated
        if fc.blocks_for(nf, 1024) <= 2048:
            return "narrow"
        return "wide" if fc.blocks_for(nf, 4096) <= 4096 else "slow"

    assert fc.PLAN_LENGTHS == {1 << 21: "narrow", (1 << 21) + 1: "wide", 1 << 24: "wide", (1 << 24) + 1: "slow"}
    for nf, name in fc.PLAN_LENGTHS.items():
        assert plan(nf) == name == fc.plan_of(nf)
        (ro, dst, fr), _ = fc.BY_LABEL[f"plan-{name}-{nf}"].build()
        assert len(fr) == nf
        deg = fc.degrees(ro, fr)
        assert 100_000 < deg.sum() < 1_000_000 and set(deg.tolist()) == {0, 1, 3}
        assert (deg == 0).mean() > 0.8
        assert deg[nf - 1] > 0
        for tile in (1024, 4096):
            last = (nf - 1) // tile
            for t in (0, 1, last - 1):
                assert deg[t * tile] > 0 and deg[t * tile + tile - 1] > 0
            assert deg[last * tile] > 0
    # every other case of the table is counted by the narrow plan
    assert all(fc.plan_of(len(c.build()[0][2])) == "narrow" for c in fc.CASES if c.group != "plans")


def test_limit_cases_sum_to_the_limit_and_sit_where_named():
    ro, dst = fc.limit_graph()
    assert int(ro[1]) - int(ro[0]) == 1 << 22 and int(ro[2]) - int(ro[1]) == (1 << 22) - 1
    assert len(dst) == int(ro[2]) and not dst.any()
    for label, (nf, start, entries, accepted) in fc.LIMITS.items():
        (_, _, fr), _ = fc.limit_case(label)
        deg = fc.degrees(ro, fr).astype(np.uint64)
        total = int(deg.sum(dtype=np.uint64))
        assert total == (fc.U32_MAX if accepted else 1 << 32), label
        assert len(fr) == nf
        pos = np.nonzero(deg)[0]
        assert len(pos) == 1024 and pos[-1] - pos[0] == 1023
        tile = fc.plan_tile(nf)
        tiles = np.unique(pos // tile)
        scan_tiles = np.unique(pos // fc.SCAN_TILE)
        assert fc.plan_of(nf) == ("wide" if label.startswith("wide") else "narrow")
        if label == "two-tiles-2^32":
            assert len(tiles) == 2 and pos[0] > 0 and (fr[:pos[0]] == fc.U32_MAX).all()
            # neither tile's own sum reaches 2^32: only the host's u64 sum of the partials refuses this one
            assert all(int(deg[pos[pos // tile == t]].sum(dtype=np.uint64)) < 1 << 32 for t in tiles)
        else:
            assert len(tiles) == 1, label                              # inside one degree tile of the plan
        if label == "wide-two-scan-tiles-2^32":
            assert len(scan_tiles) == 2
        # a u32 sum of the tile (the form before the fix) wraps to 0 exactly where the case says
        if not accepted and len(tiles) == 1:
            assert int(deg[pos].sum(dtype=np.uint64)) & fc.U32_MAX == 0


def test_expand_forms_agree_on_every_small_case():
    n = 0
    for c in fc.CASES:
        if _total(c) >= 50_000:
            continue
        (ro, dst, fr), _ = c.build()
        t, s = fo.expand(ro, dst, fr)
        tl, sl = fo.expand_loop(ro, dst, fr)
        np.testing.assert_array_equal(t, tl, err_msg=c.label)
        np.testing.assert_array_equal(s, sl, err_msg=c.label)
        n += 1
    assert n >= 20


@pytest.mark.parametrize("mode", ["D", "R", "V"])
def test_probe_world_yields_every_state(mode):
    w = fc.probe_world(mode)
    st = w["want"]["status"]
    ok = st == o.ST_OK
    miss = st == o.ST_MISS
    assert ok.sum() >= 5
    assert (miss & w["removed"]).sum() >= 5                     # tombstones
    assert (miss & w["absent"]).sum() >= 5                      # never registered, same homes
    assert (st == o.ST_MULTI_ACT).sum() >= 5
    assert (miss & w["invalid"]).sum() >= 5                     # IsValidSilo
    assert not (w["invalid"] & (w["removed"] | w["absent"])).any()
    assert set(st.tolist()) == {o.ST_OK, o.ST_MISS, o.ST_MULTI_ACT}
    # the chains: 40 grains of one home each; linear probing from the table's last group of 8 slots
    # holds at most 8 of them before the table end, so the chain goes on from slot 0
    homes = w["homes"]
    assert (homes[:40] == fc.PROBE_CAP - 8).all() and (homes[40:] == fc.MID_HOME).all()
    assert fc.PROBE_CAP - int(homes[0]) < 40
    # tombstones lie inside both chains, with live grains behind them; some chain members are multi
    gone_ids = set(w["gone"][:, 1].tolist())
    for chain in (w["wrap"][:40], w["mid"][:40]):
        ids = chain[:, 1].tolist()
        assert ids[0] in gone_ids and ids[36] in gone_ids and ids[38] not in gone_ids
        assert sum(i in gone_ids for i in ids) == 14
    # the table does not grow: live + tombstones stay below 3/4 of the capacity
    assert len(w["reg"]) < fc.PROBE_CAP * 3 // 4
    assert w["want"]["act"][ok].max() < fc.PROBE_N_ACT
    # the graph names every id and the frontier has an out-of-graph publisher and a duplicate
    assert set(np.concatenate([w["reg"][:, 1], w["wrap"][45:70, 1], w["mid"][45:70, 1]]).tolist()) <= \
        set(w["want"]["target"].tolist())


def test_frontier_cases():
    assert fc.FRONTIER_N_ACT == (1, 15, 16, 17, 4095, 4096, 4097, (1 << 20) + 5)
    for n_act in fc.FRONTIER_N_ACT:
        off, visited, edges = fc.frontier_case(n_act)
        assert len(off) == n_act + 2 and len(visited) == n_act
        fresh = fo.next_frontier(off, n_act, visited.copy())
        assert {0, n_act - 1} <= set(fresh.tolist()) and set(edges.tolist()) <= set(fresh.tolist())
        if n_act > 100:
            assert abs(visited.mean() - 1 / 3) < 0.02
            assert 0 < len(fresh) < n_act
