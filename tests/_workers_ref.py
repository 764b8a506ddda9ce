"""StatelessWorkerDirector.SelectActivationCore (Placement/StatelessWorkerDirector.cs:31-62) over the worker sets of
ActivationDirectory (Catalog/ActivationDirectory.cs:86-158), restated per message.  Paths are the reference's, under
src/Orleans.Runtime/.

select_loop is the literal simulation under the batch model of include/graindispatch.h: messages are addressed in
batch order, each is delivered before the next is addressed, nothing completes inside the batch.  select_closed is
the numpy closed form the kernels follow (tests/test_workers_ref.py proves the two equal).  add_loop / remove_loop
are RecordNewTarget / RemoveTarget's list.Remove per item.  Constants mirror include/graindispatch.h.

The random index is System.Random.Next(maxValue) on the internal sample: Sample() = draw * (1.0 / Int32.MaxValue),
then (int)(Sample() * maxValue) -- two IEEE double roundings, which Python floats reproduce.  It cannot be run
against .NET here.

Left to C# (not modelled): the registration-time overshoot check (Catalog.cs:1284-1293), re-routing of queued
messages when a worker deactivates, the RNG itself.
"""
import copy

import numpy as np

NONE32 = 0xFFFFFFFF
CAT_GRAIN = 3
CTX_VALID, CTX_STATE_MASK = 0, 3
WK_NONE, WK_IDLE, WK_NEW, WK_RANDOM, WK_HELD = range(5)
WK_NOT_GRAIN, WK_ADDED, WK_FULL = range(3)
DRAW_MAX = 0x7FFFFFFF          # Int32.MaxValue: random.Next() < it


def random_index(draw: int, count: int) -> int:
    return int((float(draw) * (1.0 / 2147483647.0)) * float(count))


def _keys(keys):
    return np.ascontiguousarray(np.asarray(keys, dtype=np.uint64).reshape(-1, 3))


def _is_grain(k) -> bool:
    return (int(k[2]) >> 56) == CAT_GRAIN


class Workers:
    """The table: GrainId -> [MaxLocal, the list in List<ActivationData> order]."""

    def __init__(self, slot_capacity: int, default_max_local: int):
        self.sc, self.default_ml = int(slot_capacity), int(default_max_local)
        self.sets = {}

    def clone(self):
        return copy.deepcopy(self)

    def _ml(self, max_local, i):
        m = 0 if max_local is None else int(max_local[i])
        return m if m > 0 else self.default_ml

    def add_loop(self, keys, ctx, max_local=None):
        keys = _keys(keys)
        st = np.zeros(len(keys), np.uint8)
        for i, k in enumerate(keys):
            if not _is_grain(k):
                st[i] = WK_NOT_GRAIN
                continue
            m = self._ml(max_local, i)
            if m > self.sc:
                st[i] = WK_FULL
                continue
            s = self.sets.setdefault(tuple(int(x) for x in k), [m, []])
            if len(s[1]) >= self.sc:
                st[i] = WK_FULL
            else:
                s[1].append(int(ctx[i]))
                st[i] = WK_ADDED
        return st

    def remove_loop(self, keys, ctx):
        keys = _keys(keys)
        out = np.zeros(len(keys), np.uint8)
        for i, k in enumerate(keys):
            t = tuple(int(x) for x in k)
            s = self.sets.get(t) if _is_grain(k) else None
            c = int(ctx[i])
            if s is None or c == NONE32 or c not in s[1]:
                continue
            s[1].remove(c)                      # the first occurrence; the order of the rest is kept
            out[i] = 1
            if not s[1]:
                del self.sets[t]                # RemoveTarget removes the map entry (:116-147)
        return out

    def lookup(self, keys):
        keys = _keys(keys)
        n = len(keys)
        cnt, ml = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        lst = np.full((n, self.sc), NONE32, np.uint32)
        for i, k in enumerate(keys):
            s = self.sets.get(tuple(int(x) for x in k)) if _is_grain(k) else None
            if s is not None:
                cnt[i], ml[i] = len(s[1]), s[0]
                lst[i, :len(s[1])] = s[1]
        return cnt, ml, lst


class _Act:
    """What SelectActivationCore and ActivationData.IsInactive read of one activation."""

    def __init__(self, ctx, valid, running, waiting):
        self.ctx, self.valid, self.running, self.waiting = ctx, valid, running, waiting


def _act_of(ctx, ctx_flags, num_running, wait_offsets):
    n_ctx = 0 if ctx_flags is None else len(ctx_flags)
    if ctx >= n_ctx:
        return _Act(ctx, False, 0, 0)           # a context the turn arrays do not cover: counted, never idle
    nr = int(np.int32(np.uint32(num_running[ctx])))
    w = 0 if wait_offsets is None else int(wait_offsets[ctx + 1]) - int(wait_offsets[ctx])
    return _Act(ctx, (int(ctx_flags[ctx]) & CTX_STATE_MASK) == CTX_VALID, nr, w)


def select_loop(w: Workers, keys, ctx_base, ctx_flags, num_running, wait_offsets=None, max_local=None, draw=None):
    """(ctx u32[n], pick u8[n], new_idx u32[n_new]); w takes the new workers."""
    keys = _keys(keys)
    n = len(keys)
    out_ctx, pick, new_idx = np.full(n, NONE32, np.uint32), np.zeros(n, np.uint8), []
    acts = {}                                   # per grain: the ActivationData records, in list order

    def records(t, s):
        if t not in acts:
            acts[t] = [_act_of(c, ctx_flags, num_running, wait_offsets) for c in s[1]]
        return acts[t]

    for i, k in enumerate(keys):
        if not _is_grain(k):
            pick[i] = WK_NONE                   # the reference throws for clients (:33-34)
            continue
        m = w._ml(max_local, i)
        if m > w.sc:
            pick[i] = WK_HELD
            continue
        t = tuple(int(x) for x in k)
        s = w.sets.setdefault(t, [m, []])
        local = list(records(t, s))             # FindTargets' ToList (ActivationDirectory.cs:150-158)
        chosen = None
        for a in local:                         # :46-53
            if a.valid and a.running <= 0 and a.waiting == 0:
                chosen = a
                break
        if chosen is not None:
            pick[i], out_ctx[i] = WK_IDLE, chosen.ctx
            chosen.running = 1                  # delivered: it is executing for the rest of the batch (RecordRunning;
            #                                     an inconsistent negative count does not keep it idle)
            continue
        if len(local) < s[0]:                   # null -> AddActivation on the local silo (:26-29,61)
            a = _Act(int(ctx_base) + len(new_idx), False, 0, 0)     # state Create: not Valid
            acts[t].append(a)
            s[1].append(a.ctx)
            new_idx.append(i)
            pick[i], out_ctx[i] = WK_NEW, a.ctx
            continue
        if len(local) == 1:                     # :55-59, local.Count == 1 ? 0 : random.Next(local.Count)
            r = 0
        elif draw is None or int(draw[i]) >= DRAW_MAX:
            pick[i] = WK_HELD
            continue
        else:
            r = random_index(int(draw[i]), len(local))
        pick[i], out_ctx[i] = WK_RANDOM, local[r].ctx
        local[r].waiting += 1
    return out_ctx, pick, np.array(new_idx, np.uint32)


def select_closed(w: Workers, keys, ctx_base, ctx_flags, num_running, wait_offsets=None, max_local=None, draw=None):
    """The closed form: per set a = |I|, room = max(0, m - c), C = c + room, and the message of stable rank k is
    IDLE (k < a), NEW (a <= k < a + room) or RANDOM over the final list."""
    keys = _keys(keys)
    n = len(keys)
    out_ctx, pick = np.full(n, NONE32, np.uint32), np.zeros(n, np.uint8)
    n_ctx = 0 if ctx_flags is None else len(ctx_flags)
    grain = (keys[:, 2] >> np.uint64(56)) == CAT_GRAIN
    ml = np.full(n, w.default_ml, np.int64)
    if max_local is not None:
        given = np.asarray(max_local, dtype=np.int64)
        ml = np.where(given > 0, given, w.default_ml)
    part = grain & (ml <= w.sc)
    pick[grain & ~part] = WK_HELD
    idx = np.flatnonzero(part)
    if len(idx) == 0:
        return out_ctx, pick, np.zeros(0, np.uint32)
    _, first, inv = np.unique(keys[idx], axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    is_new = np.zeros(n, bool)
    shape = []
    for g in range(len(first)):
        members = idx[inv == g]                                   # batch order
        t = tuple(int(x) for x in keys[members[0]])
        s = w.sets.setdefault(t, [int(ml[members[0]]), []])       # the first message decides a new set's MaxLocal
        L = np.array(s[1], np.int64)
        c, m = len(L), s[0]
        idle = np.zeros(c, bool)
        known = L < n_ctx
        if known.any():
            lk = L[known]
            ok = (np.asarray(ctx_flags)[lk] & CTX_STATE_MASK) == CTX_VALID
            ok &= np.asarray(num_running, dtype=np.uint32)[lk].view(np.int32) <= 0
            if wait_offsets is not None:
                wo = np.asarray(wait_offsets, dtype=np.int64)
                ok &= wo[lk + 1] == wo[lk]
            idle[known] = ok
        I = L[idle]
        a, room = len(I), max(0, m - c)
        k = np.arange(len(members))
        pick[members[k < a]] = WK_IDLE
        out_ctx[members[k < a]] = I[:min(a, len(members))]
        is_new[members[(k >= a) & (k < a + room)]] = True
        shape.append((members, L, a, room))
    g_rank = np.cumsum(is_new) - 1
    new_idx = np.flatnonzero(is_new).astype(np.uint32)
    pick[is_new] = WK_NEW
    out_ctx[is_new] = (int(ctx_base) + g_rank[is_new]).astype(np.uint32)
    for members, L, a, room in shape:
        c = len(L)
        C = c + room
        made = members[a:a + room]                                 # the messages that append, in list order
        final = np.concatenate([L, out_ctx[made].astype(np.int64)])
        for i in members[a + room:]:
            if C == 1:
                r = 0
            elif draw is None or int(draw[i]) >= DRAW_MAX:
                pick[i] = WK_HELD
                continue
            else:
                r = random_index(int(draw[i]), C)
            pick[i], out_ctx[i] = WK_RANDOM, final[r]
        t = tuple(int(x) for x in keys[members[0]])
        w.sets[t][1].extend(int(x) for x in out_ctx[made])
    return out_ctx, pick, new_idx


def random_world(rng, n_sets, slot_capacity, n_ctx, type_code_data, max_m=None):
    """A table of n_sets grains with random lists over distinct contexts, and random turn arrays: (Workers, keys
    u64[n_sets, 3], ctx_flags, num_running, wait_offsets)."""
    max_m = max_m or slot_capacity
    w = Workers(slot_capacity, max(1, min(3, slot_capacity)))
    keys = np.zeros((n_sets, 3), np.uint64)
    keys[:, 1] = np.arange(1, n_sets + 1, dtype=np.uint64) * np.uint64(7919)
    keys[:, 2] = np.uint64(type_code_data)
    pool = rng.permutation(n_ctx + n_ctx // 4 + 8)                 # a few contexts past n_ctx: never idle
    at = 0
    for k in keys:
        c = int(rng.integers(0, min(slot_capacity, max_m + 2) + 1))
        c = min(c, len(pool) - at)
        m = int(rng.integers(1, max_m + 1))
        if c:
            w.sets[tuple(int(x) for x in k)] = [m, [int(x) for x in pool[at:at + c]]]
        at += c
    state = rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), size=n_ctx)
    ctx_flags = (state | (rng.integers(0, 2, n_ctx).astype(np.uint8) << 4)).astype(np.uint8)
    num_running = np.where(rng.random(n_ctx) < 0.5, 0, rng.integers(-1, 3, n_ctx)).astype(np.int32).view(np.uint32)
    waits = np.where(rng.random(n_ctx) < 0.8, 0, rng.integers(0, 3, n_ctx))
    wait_offsets = np.zeros(n_ctx + 1, np.uint32)
    wait_offsets[1:] = np.cumsum(waits)
    return w, keys, ctx_flags, num_running, wait_offsets
