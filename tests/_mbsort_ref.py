"""Reference of the micro-batch sorter (k_mb_sort_runs, gd_mbsort.h) and the case table of
test_gpu_mbsort.py.

The sorter's contract: the messages of a batch grouped by clamped activation min(act, n_act), groups in
ascending activation order, every group in arrival order (ActivationData.cs:566-606: a grain's messages
are enqueued in the order received); per group a run (activation, first position), run_start closed by n.
Two restatements, neither of which allocates O(n_act) memory (n_act reaches 0xFFFFFFFE) and neither of
which uses the oracle's bucket_stable: literal_runs (a dict of lists) and fast_runs (a stable argsort).

plan() restates the driver's documented choice of the sorter's template instantiation and grid
(mb_enqueue / mb_sort_grid, eng_abi.hip).  It only proves that the case table below reaches every
instantiation; it is never an expected value for the kernel."""
import numpy as np

MB_MAX = 8192            # messages a micro-batch holds
MB_MAX_BITS = 11         # widest radix digit
ACT_MAX = 0xFFFFFFFD     # largest single-activation number (0xFFFFFFFE: GD_ACT_MULTI, 0xFFFFFFFF: a miss)


# ----------------------------------------------------------------------------- the two restatements
def literal_runs(acts, n_act):
    """(perm u32[n], run_act u32[r], run_start u32[r + 1], n_runs): one FIFO per clamped activation,
    filled in arrival order, emitted by ascending activation."""
    queues = {}
    for i, a in enumerate(acts):
        queues.setdefault(min(int(a), int(n_act)), []).append(i)
    perm, run_act, run_start = [], [], []
    for a in sorted(queues):
        run_act.append(a)
        run_start.append(len(perm))
        perm.extend(queues[a])
    run_start.append(len(perm))
    return (np.asarray(perm, dtype=np.uint32), np.asarray(run_act, dtype=np.uint32),
            np.asarray(run_start, dtype=np.uint32), len(run_act))


def fast_runs(acts, n_act):
    """literal_runs from a stable argsort of the clamped activations and np.unique."""
    a = np.asarray(acts).astype(np.uint64)
    clamped = np.minimum(a, np.uint64(n_act))
    perm = np.argsort(clamped, kind="stable").astype(np.uint32)
    if len(a) == 0:
        return perm, np.zeros(0, np.uint32), np.zeros(1, np.uint32), 0
    ua, counts = np.unique(clamped, return_counts=True)
    run_start = np.zeros(len(ua) + 1, dtype=np.uint32)
    run_start[1:] = np.cumsum(counts)
    return perm, ua.astype(np.uint32), run_start, len(ua)


def check(mb, n, acts, n_act):
    """mb (a MicroBatch after run(n), or anything with its perm / n_runs / run_act / run_start) against
    fast_runs(acts[:n], n_act): bit for bit, and perm a permutation of range(n)."""
    perm, run_act, run_start, r = fast_runs(np.asarray(acts)[:n], n_act)
    got = np.array(mb.perm[:n])
    assert np.array_equal(np.sort(got), np.arange(n, dtype=np.uint32)), "perm is not a permutation of range(n)"
    assert mb.n_runs == r, f"n_runs {mb.n_runs}, want {r}"
    bad = np.flatnonzero(got != perm)
    assert len(bad) == 0, f"perm differs at {len(bad)} positions, first {bad[0]}: {got[bad[0]]} want {perm[bad[0]]}"
    got_act, got_start = np.array(mb.run_act[:r]), np.array(mb.run_start[:r + 1])
    assert np.array_equal(got_act, run_act), f"run_act differs first at {np.flatnonzero(got_act != run_act)[:1]}"
    assert np.array_equal(got_start, run_start), \
        f"run_start differs first at {np.flatnonzero(got_start != run_start)[:1]}"
    assert int(got_start[r]) == n


# ----------------------------------------------------------------------------- the driver's choice
def plan(n_act, n, split=8):
    """(bits, passes, IT, grid) of k_mb_sort_runs<bits, IT> for a zero-copy micro-batch of n messages."""
    key_bits = max(1, int(n_act).bit_length())
    passes = -(-key_bits // MB_MAX_BITS)
    bits = max(4, -(-key_bits // passes))
    it = 4 if n <= 4096 else 8
    grid = max(1, min(split, max(1, n // 256)))
    return bits, passes, it, grid


# ----------------------------------------------------------------------------- registered activations
def activation_numbers(seed=2047, count=MB_MAX):
    """`count` distinct activation numbers <= ACT_MAX and the index arrays of three families among them:
    j (j < 1024), j << 11 (j < 1024), j << 22 (j < 512) -- equal low digits under distinct high digits and
    the reverse, so the hot digit differs from pass to pass -- and, for every bit length that the first
    family leaves open, seeded distinct values of that length (so log-uniform over the lengths), ACT_MAX
    among them.  The values are dealt to the grains in a seeded order.
    Returns (acts u32[count], {"j": idx, "j<<11": idx, "j<<22": idx})."""
    rng = np.random.default_rng(seed)
    fams = {"j": np.arange(1024, dtype=np.uint64), "j<<11": np.arange(1, 1024, dtype=np.uint64) << np.uint64(11),
            "j<<22": np.arange(1, 512, dtype=np.uint64) << np.uint64(22)}
    taken = set()
    for v in fams.values():
        taken.update(v.tolist())
    assert len(taken) == 1024 + 1023 + 511
    lengths = [b for b in range(1, 33) if (1 << b) > 1024]       # 1..10 are all in the family j
    rest = count - len(taken)
    extra = [ACT_MAX]
    taken.add(ACT_MAX)
    for k, b in enumerate(lengths):
        quota = (rest - 1) // len(lengths) + (1 if k < (rest - 1) % len(lengths) else 0)
        lo, hi = 1 << (b - 1), min((1 << b) - 1, ACT_MAX)
        got = 0
        while got < quota:
            for v in rng.integers(lo, hi + 1, size=quota - got, dtype=np.uint64).tolist():
                if v not in taken:
                    taken.add(v)
                    extra.append(v)
                    got += 1
    vals = np.concatenate([fams["j"], fams["j<<11"], fams["j<<22"], np.asarray(extra, dtype=np.uint64)])
    assert len(vals) == count == len(taken)
    deal = rng.permutation(count)                                # vals[i] goes to grain deal[i]
    acts = np.zeros(count, dtype=np.uint32)
    acts[deal] = vals.astype(np.uint32)
    at, idx = 0, {}
    for name, v in fams.items():
        idx[name] = np.sort(deal[at:at + len(v)])
        at += len(v)
    return acts, idx


# ----------------------------------------------------------------------------- the case table
N_ACTS = [1, 15, 16, 63, 127, 255, 256, 1023, 2047,                                  # one pass
          2048, 1 << 13, 1 << 15, 1 << 17, 1 << 19, 1 << 20, (1 << 22) - 1,         # two passes
          1 << 22, 1 << 26, 1 << 29, 1 << 31, 0xFFFFFFFE]                             # three passes
ANCHORS = [2047, 1 << 20, 1 << 22, 0xFFFFFFFE]
ANCHOR_NS = [1, 63, 64, 65, 255, 256, 257, 511, 512, 1000, 4095, 4096, 4097, 6000, 8191, 8192]
OTHER_NS = [1000, 4096, 4097, 8192]
FAMILIES = ["j", "j<<11", "j<<22"]
ANCHOR_PATTERNS = ["uniform", "one", "alt_lane", "alt_row", "descending", "unregistered", "half_unregistered",
                   "j", "j<<11", "j<<22"]
SPLITS = [1, 2, 3, 7, 8, 31, 32, 64]
SPLIT_NS = [255, 256, 257, 767, 768, 1000, 4096, 8191, 8192]
SPLIT_PATTERNS = ["one", "edge", "edge+1"]
REUSE_NS = [8192, 1, 4097, 0, 4096]
STAGED_NS = [1000, 8191]          # mb_zerocopy = 0, once per anchor


def ns_of(n_act):
    return ANCHOR_NS if n_act in ANCHORS else OTHER_NS


def patterns_of(n_act):
    """Every pattern at the anchors; elsewhere uniform, one grain, and the family whose distinct digit
    is the last pass's."""
    if n_act in ANCHORS:
        return ANCHOR_PATTERNS
    return ["uniform", "one", FAMILIES[plan(n_act, 1)[1] - 1]]


def table():
    """Every (n_act, n, split) that test_gpu_mbsort.py runs with zero-copy stores."""
    out = [(na, n, 8) for na in N_ACTS for n in ns_of(na)]
    out += [(na, n, s) for na in ANCHORS for s in SPLITS for n in SPLIT_NS]
    out += [(na, n, 8) for na in ANCHORS for n in REUSE_NS]
    return out
