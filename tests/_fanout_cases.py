"""Case table of the follower fan-out's hard edges (gd_fanout.h, eng_fanout.hip), for
test_fanout_cases.py (CPU: the table reaches what it claims) and test_gpu_fanout_edges.py (GPU: bit for
bit against oracle/fanout.py).  numpy and the oracle only; no GPU code is imported here.

Every builder returns ((row_off, dst, frontier), label).  The arithmetic below restates the driver's
documented choices (counting plan, tile form, items a block stages); it only proves that a case reaches
the path it names and is never an expected value for a kernel."""
from functools import lru_cache

import numpy as np

import fanout as fo
import oracle as o
from _chain_keys import home_slot_np, keys_with_home

# ----------------------------------------------------------------------------- the code's constants
BLOCK = 256                     # gd_hash.h:16      constexpr int BLOCK = 256
SCAN_TILE = BLOCK * 4           # gd_scan.h:8-9     SCAN_ITEMS = 4, SCAN_TILE = BLOCK * SCAN_ITEMS
FAN_TILE = BLOCK * 8            # gd_fanout.h:29-30 FAN_IT = 8, FAN_TILE = BLOCK * FAN_IT
FAN_LDS_ITEMS = FAN_TILE        # gd_fanout.h:31    publishers a block stages
FAN_SMALL_TILES = 1024          # eng_fanout.hip:79 below that many FAN_TILE tiles: tiles of BLOCK * 2 outputs
FAN_SMALL_TILE = BLOCK * 2      # eng_fanout.hip    fan_route_launch_cx: fan_route_launch_it<..., 2>
FR_TILE = BLOCK * 16            # gd_fanout.h:486-487 FR_ITEMS = 16, FR_TILE = BLOCK * FR_ITEMS
FR_ITEMS = 16
WAVE = 64                       # gd_hash.h:15      wave_upper_bound_u32 narrows by WAVE pieces a round
NARROW_MAX_BLOCKS = 2048        # eng_fanout.hip fan_count: nb4 <= 2048
WIDE_MAX_BLOCKS = 4096          # eng_fanout.hip fan_count: nb16 <= 4096
U32_MAX = 0xFFFFFFFF
SMALL_FORM_MAX = (FAN_SMALL_TILES - 1) * FAN_TILE        # 2,095,104: the largest total of the 512-output form

TC = o.grain_type_code(fo.CHIRPER_ACCOUNT_CLASS)


def blocks_for(n, tile):
    return (n + tile - 1) // tile


def plan_of(nf):
    """fan_count / fan_count_post's counting plan for a frontier of nf publishers."""
    if blocks_for(nf, SCAN_TILE) <= NARROW_MAX_BLOCKS:
        return "narrow"
    if blocks_for(nf, 4 * SCAN_TILE) <= WIDE_MAX_BLOCKS:
        return "wide"
    return "slow"


def plan_tile(nf):
    """Frontier entries a degree tile of the plan covers (slow: k_fan_degree has no tiles)."""
    return {"narrow": SCAN_TILE, "wide": 4 * SCAN_TILE, "slow": None}[plan_of(nf)]


def route_tile(total):
    """Outputs a block of k_fan_route owns at this total (k_fan_expand always owns FAN_TILE)."""
    return FAN_SMALL_TILE if blocks_for(total, FAN_TILE) < FAN_SMALL_TILES else FAN_TILE


def degrees(row_off, frontier):
    ro = np.asarray(row_off, dtype=np.int64)
    fr = np.asarray(frontier, dtype=np.int64)
    ok = fr < len(ro) - 1
    frc = np.where(ok, fr, 0)
    return np.where(ok, ro[frc + 1] - ro[frc], 0)


def block_counts(row_off, frontier, tile):
    """Publishers each block of `tile` outputs covers, as fan_stage finds them: from the item of its
    first output to the item of its last, both by upper_bound over the inclusive scan."""
    ends = np.cumsum(degrees(row_off, frontier))
    total = int(ends[-1]) if len(ends) else 0
    p0 = np.arange(0, total, tile, dtype=np.int64)
    p1 = np.minimum(p0 + tile, total)
    lo = np.searchsorted(ends, p0, side="right")
    hi = np.searchsorted(ends, p1 - 1, side="right")
    return hi - lo + 1


# ----------------------------------------------------------------------------- the shared graph
N_NODES = 4096
# nodes with a chosen follower count; every other node i has (0, 1, 3)[i % 3] followers
SPECIAL = {0: 0, 1: 1, 2: 2, 3: 3, 10: 511, 11: 512, 12: 513, 13: 2047, 14: 2048, 15: 2049, 16: 7000}
FIRST_PLAIN = 33                # a multiple of 3: plain node i has class i % 3
OUT_OF_GRAPH = (N_NODES, U32_MAX)
N_TARGETS = N_NODES + 64        # follower ids the lists name (the ones past N_NODES are never registered)


@lru_cache(maxsize=None)
def graph():
    deg = np.array([(0, 1, 3)[i % 3] for i in range(N_NODES)], dtype=np.int64)
    for u, d in SPECIAL.items():
        deg[u] = d
    row_off = np.zeros(N_NODES + 1, dtype=np.uint32)
    row_off[1:] = np.cumsum(deg)
    dst = np.random.default_rng(41).integers(0, N_TARGETS, size=int(row_off[-1])).astype(np.uint32)
    row_off.setflags(write=False)
    dst.setflags(write=False)
    return row_off, dst


def registered_nodes():
    """The directory of the expansion cases: every target id below N_NODES but each 19th."""
    ids = np.arange(N_NODES)
    return ids[ids % 19 != 7]


def _node_of_degree(d):
    return next(u for u, x in SPECIAL.items() if x == d)


def _plain(cls, idx):
    """Plain nodes of degree class cls (0 -> 0, 1 -> 1, 2 -> 3 followers), picked by index."""
    n = (N_NODES - FIRST_PLAIN) // 3
    return FIRST_PLAIN + 3 * (np.asarray(idx, dtype=np.int64) % n) + cls


def _case(frontier, label):
    ro, dst = graph()
    fr = np.ascontiguousarray(np.asarray(frontier, dtype=np.int64).astype(np.uint32))
    fr.setflags(write=False)
    return (ro, dst, fr), label


class Case:
    """One row of the table: `build()` is the builder (cached: references are computed once)."""

    def __init__(self, label, group, fn, *args):
        self.label, self.group = label, group
        self._fn, self._args = fn, args
        self._built = None

    def build(self):
        if self._built is None:
            got, label = self._fn(*self._args)
            assert label == self.label
            self._built = got
        return self._built, self.label


# ----------------------------------------------------------------------------- staging boundary
def _staging_pattern(tile, z, salt):
    """Exactly `tile` outputs over z + 2 publishers: one follower, z publishers without followers, then
    a row that covers the rest of the block."""
    return np.concatenate([[_node_of_degree(1)], _plain(0, salt + np.arange(z)), [_node_of_degree(tile - 1)]])


INTERIOR_BLOCK = 3


def staging(form, z):
    """The pattern at block 0 and at block INTERIOR_BLOCK of the form's tiling, whole-tile rows between
    them, ordinary publishers behind; the large form has a tail lifting the total past SMALL_FORM_MAX."""
    tile = FAN_SMALL_TILE if form == "small" else FAN_TILE
    fill = [_node_of_degree(tile)] * (INTERIOR_BLOCK - 1)
    parts = [_staging_pattern(tile, z, 0), fill, _staging_pattern(tile, z, 500), _plain(2, np.arange(40)),
             _plain(1, np.arange(25))]
    if form == "large":
        parts.append([_node_of_degree(FAN_TILE)] * 1100)
        parts.append(_plain(2, np.arange(7)))
    return _case(np.concatenate(parts), f"staging-{form}-z{z}")


# ----------------------------------------------------------------------------- tile edges
def tile_edges(form):
    """Rows ending on block edges, rows of TILE - 1 / TILE / TILE + 1 outputs for both tile sizes, one
    row over at least three blocks, publishers without followers or outside the graph at the first, a
    middle and the last position, duplicates."""
    d = _node_of_degree
    if form == "small":
        fr = [OUT_OF_GRAPH[0], d(512), d(512), d(0), d(511), d(1), d(513), d(511), OUT_OF_GRAPH[1], d(7000),
              d(3), d(3), d(2047), OUT_OF_GRAPH[0], d(0), d(2048), d(2049), d(7000), d(1), d(1), d(0)]
    else:
        fr = [OUT_OF_GRAPH[1], d(2048), d(2048), d(0), d(2047), d(1), d(2049), d(2047), d(7000), d(512), d(511),
              d(513)] + [d(2048)] * 550 + [OUT_OF_GRAPH[0], d(0), d(7000), d(7000)] + [d(2049)] * 500 + \
             [d(3), d(3), OUT_OF_GRAPH[0]]
    return _case(fr, f"edges-{form}")


TOTALS = (1, 511, 512, 513, 2047, 2048, 2049, SMALL_FORM_MAX, SMALL_FORM_MAX + 1)


def total_case(total):
    """A frontier emitting exactly `total` messages: rows of 2,048, 512, 3 and 1 followers, a publisher
    without followers after every seventh."""
    fr, left = [], total
    for deg in (2048, 512, 3, 1):
        k, left = divmod(left, deg)
        fr += [_node_of_degree(deg)] * k
    fr = np.asarray(fr, dtype=np.int64)
    fr = np.insert(fr, np.arange(7, len(fr), 7), _node_of_degree(0))
    return _case(fr, f"total-{total}")


# ----------------------------------------------------------------------------- search widths
WIDTHS = (1, 2, WAVE - 1, WAVE, WAVE + 1, WAVE ** 2 - 1, WAVE ** 2, WAVE ** 2 + 1, WAVE ** 3 - 1, WAVE ** 3,
          WAVE ** 3 + 1)


def width_mixed(nf):
    rng = np.random.default_rng(1000 + nf)
    cls = rng.integers(0, 3, size=nf)                     # followers (0, 1, 3)[cls]
    if nf == 1:
        cls[:] = 2                                        # a frontier of one publisher must emit something
    return _case(_plain(cls, rng.integers(0, 1 << 20, size=nf)), f"width-mixed-{nf}")


def width_ones(nf):
    """Every publisher has one follower: output p belongs to item p, so every piece boundary of every
    round of the search is some block's target."""
    rng = np.random.default_rng(2000 + nf)
    return _case(_plain(1, rng.integers(0, 1 << 20, size=nf)), f"width-ones-{nf}")


# ----------------------------------------------------------------------------- counting plans
PLAN_LENGTHS = {(1 << 21): "narrow", (1 << 21) + 1: "wide", (1 << 24): "wide", (1 << 24) + 1: "slow"}


def plan_case(nf):
    """nf publishers, nearly all without followers; a sparse few with 1 or 3 (so the hop stays under a
    million messages), among them the first and the last entry of degree tiles of both sizes and the last
    entry of the frontier."""
    rng = np.random.default_rng(3000 + (nf & 0xFFFF) + (nf >> 16))
    fr = _plain(0, rng.integers(0, 1 << 20, size=nf))
    stride = 8 if nf <= (1 << 21) + 1 else 64
    pos = np.arange(3, nf, stride)
    edges = []
    for tile in (SCAN_TILE, 4 * SCAN_TILE):
        last_tile = (nf - 1) // tile
        for t in (0, 1, last_tile // 2, last_tile - 1, last_tile):
            edges += [t * tile, min(t * tile + tile - 1, nf - 1)]
    pos = np.unique(np.concatenate([pos, edges, [nf - 1]]))
    fr[pos] = _plain(rng.integers(1, 3, size=len(pos)), rng.integers(0, 1 << 20, size=len(pos)))
    return _case(fr, f"plan-{PLAN_LENGTHS[nf]}-{nf}")


CASES = (
    [Case(f"staging-{form}-z{z}", "staging", staging, form, z)
     for form in ("small", "large") for z in (FAN_LDS_ITEMS - 2, FAN_LDS_ITEMS - 1)] +
    [Case(f"edges-{form}", "edges", tile_edges, form) for form in ("small", "large")] +
    [Case(f"total-{t}", "edges", total_case, t) for t in TOTALS] +
    [Case(f"width-mixed-{n}", "widths", width_mixed, n) for n in WIDTHS] +
    [Case(f"width-ones-{n}", "widths", width_ones, n) for n in WIDTHS] +
    [Case(f"plan-{PLAN_LENGTHS[n]}-{n}", "plans", plan_case, n) for n in PLAN_LENGTHS]
)
BY_LABEL = {c.label: c for c in CASES}
assert len(BY_LABEL) == len(CASES)


def cases(group):
    return [c for c in CASES if c.group == group]


# ----------------------------------------------------------------------------- the 32-bit limit
BIG_ROW = 1 << 22               # row 0; row 1 has one follower fewer


@lru_cache(maxsize=None)
def limit_graph():
    """Two publishers of 2^22 and 2^22 - 1 followers, every follower id 0 (32 MB of zeros)."""
    row_off = np.array([0, BIG_ROW, 2 * BIG_ROW - 1], dtype=np.uint32)
    return row_off, np.zeros(2 * BIG_ROW - 1, dtype=np.uint32)


def _limit_frontier(nf, start, entries):
    fr = np.full(nf, U32_MAX, dtype=np.uint32)           # outside the graph: no followers
    fr[start:start + len(entries)] = entries
    return fr


# label -> (frontier length, first entry, entries, accepted)
_ROWS0 = [0] * 1024
LIMITS = {
    "max-accepted":          (1024, 0, [0] * 1023 + [1], True),
    "one-tile-2^32":         (1024, 0, _ROWS0, False),
    "two-tiles-2^32":        (SCAN_TILE + 512 + 1024, SCAN_TILE + 512, _ROWS0, False),
    "wide-one-tile-2^32":    ((1 << 21) + 1, 5 * 4 * SCAN_TILE + 2 * SCAN_TILE, _ROWS0, False),
    "wide-two-scan-tiles-2^32": ((1 << 21) + 1, 9 * 4 * SCAN_TILE + SCAN_TILE + 512, _ROWS0, False),
    "wide-max-accepted":     ((1 << 21) + 1, 3 * 4 * SCAN_TILE + 512, [0] * 1023 + [1], True),
}


def limit_case(label):
    nf, start, entries, _ = LIMITS[label]
    ro, dst = limit_graph()
    return (ro, dst, _limit_frontier(nf, start, entries)), label


# ----------------------------------------------------------------------------- probe states
PROBE_CAP = 2048
PROBE_N_ACT = 1 << 12
PROBE_BG = 300
PROBE_INVALID_SILO = 3
MID_HOME = 1000                  # 8-aligned, mid-table


@lru_cache(maxsize=None)
def probe_world(mode):
    """A directory of PROBE_CAP slots holding two chains of 40 grains (one homed in the table's last
    group, so it wraps to slot 0; one mid-table) and background grains; every third chain member
    unregistered again (tombstones), some grains upserted to several activations, silo
    PROBE_INVALID_SILO invalid, and ids of the chains' homes that were never registered.  A follower
    graph of 64 publishers whose lists name all of them.  Returns a dict: the directory calls to make,
    the graph and frontier, and the oracle's route of every message (`want`)."""
    silos = o.bench_silos(8)
    spec = o.ring_spec(silos, mode)
    last_home = PROBE_CAP - 8
    wrap = keys_with_home(TC, PROBE_CAP, last_home, 70)
    mid = keys_with_home(TC, PROBE_CAP, MID_HOME, 70)
    base = int(max(wrap[-1, 1], mid[-1, 1])) + 1
    bg = o.grain_keys(TC, base + np.arange(PROBE_BG))
    chains = np.concatenate([wrap[:40], mid[:40]])
    never = np.concatenate([wrap[45:70], mid[45:70], o.grain_keys(TC, base + PROBE_BG + np.arange(40))])
    reg = np.concatenate([bg[:150], chains, bg[150:]])
    own = lambda k: o.ring_owner_np(spec, o.jenkins_u64x3_np(k[:, 2], k[:, 0], k[:, 1])).astype(np.uint32)  # noqa: E731
    reg_act = np.arange(1, len(reg) + 1, dtype=np.uint32)
    rng = np.random.default_rng(77)
    # registered on any silo (a grain's activation need not live on its directory owner)
    reg_silo = ((own(reg) + rng.integers(0, 3, size=len(reg))) % 8).astype(np.uint32)
    table = {tuple(int(x) for x in k): (int(a), int(s)) for k, a, s in zip(reg, reg_act, reg_silo)}
    gone = np.concatenate([wrap[:40][::3], mid[:40][::3]])
    gone_act = np.array([table[tuple(int(x) for x in k)][0] for k in gone], dtype=np.uint32)
    for k in gone:
        del table[tuple(int(x) for x in k)]
    multi = np.concatenate([wrap[:40][1::6], mid[:40][1::6], bg[5:60:5]])
    multi_silo = own(multi)
    for k, s in zip(multi, multi_silo):
        table[tuple(int(x) for x in k)] = (o.ACT_MULTI, int(s))
    keys = np.array(list(table.keys()), dtype=np.uint64).reshape(-1, 3)
    vals = np.array(list(table.values()), dtype=np.uint32).reshape(-1, 2)
    directory = o.DirectoryArrays(keys, vals[:, 0], vals[:, 1])
    # the follower graph: every id above, each several times, over 64 publishers
    ids = np.concatenate([reg[:, 1], never[:, 1]]).astype(np.uint32)
    lists = np.concatenate([ids, ids[rng.permutation(len(ids))], ids[rng.permutation(len(ids))]])
    cuts = np.sort(rng.choice(np.arange(1, len(lists)), size=63, replace=False))
    row_off = np.concatenate([[0], cuts, [len(lists)]]).astype(np.uint32)
    frontier = np.concatenate([rng.permutation(64), [64, 5, 5, U32_MAX]]).astype(np.uint32)
    target, sender = fo.expand(row_off, lists, frontier)
    st, silo, act, owner, _ = o.route_batch_np(o.grain_keys(TC, target.astype(np.int64)), spec, directory)
    # IsValidSilo: a single activation on an invalid silo is a miss at the ring owner
    bad = (st == o.ST_OK) & (silo == PROBE_INVALID_SILO)
    st, silo, act = st.copy(), silo.copy(), act.copy()
    st[bad], silo[bad], act[bad] = o.ST_MISS, owner[bad], o.M32
    perm, off = o.bucket_stable(act, PROBE_N_ACT)
    removed = np.isin(target, gone[:, 1].astype(np.uint32))
    absent = np.isin(target, never[:, 1].astype(np.uint32))
    return dict(spec=spec, silos=silos, mode=mode, last_home=last_home, wrap=wrap, mid=mid, reg=reg, reg_act=reg_act,
                reg_silo=reg_silo, gone=gone, gone_act=gone_act, multi=multi, multi_silo=multi_silo,
                row_off=row_off, dst=lists, frontier=frontier, invalid=bad, removed=removed, absent=absent,
                homes=home_slot_np(chains, PROBE_CAP),
                want=dict(target=target, sender=sender, status=st, silo=silo, act=act, perm=perm, offsets=off))


# ----------------------------------------------------------------------------- next frontier
FRONTIER_N_ACT = (1, 15, 16, 17, FR_TILE - 1, FR_TILE, FR_TILE + 1, (1 << 20) + 5)


def frontier_case(n_act):
    """(offsets u32[n_act + 2], visited bool[n_act]): activations that got 0, 1 or 2 messages, a third of
    them visited before; the first and last activation, both sides of every FR_TILE edge and of the first
    thread's 16-item edge got one and were not visited."""
    rng = np.random.default_rng(4000 + n_act % 9973)
    got = rng.integers(0, 3, size=n_act)
    visited = np.zeros(n_act, dtype=bool)
    visited[rng.permutation(n_act)[: n_act // 3]] = True
    edges = [0, n_act - 1, FR_ITEMS - 1, FR_ITEMS]
    for e in range(FR_TILE, n_act + 1, FR_TILE):
        edges += [e - 1, e]
    edges = np.array([e for e in edges if 0 <= e < n_act], dtype=np.int64)
    got[edges] = 1
    visited[edges] = False
    offsets = np.zeros(n_act + 2, dtype=np.uint32)
    offsets[1:n_act + 1] = np.cumsum(got)
    offsets[n_act + 1] = offsets[n_act] + 5                # the trailing bucket: unrouted messages
    return offsets, visited, edges
