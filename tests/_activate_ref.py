"""Catalog.GetOrCreateActivation for a received batch, restated per message: what the null-context
closure of Dispatcher.ReceiveMessage (Core/Dispatcher.cs:75-201) does before ReceiveRequest / ReceiveResponse.
Paths are the reference's, under src/Orleans.Runtime/.

activate_loop is the one-by-one rule over a dict in arrival order; activate_closed the closed form the kernels
follow (tests/test_activate_ref.py proves the two equal).  Constants mirror include/graindispatch.h.
"""
import numpy as np

import _turns_ref as T

NONE32 = 0xFFFFFFFF
TTL_NONE = np.iinfo(np.int64).max
RECV_ACTIVATION, RECV_NULL_CONTEXT = 0, 2
AD_VALID, AD_SYSTEM_TARGET, AD_STATELESS_WORKER = 1, 2, 4
DIR_RESPONSE = 1
(ACTV_NONE, ACTV_FOUND, ACTV_CREATED, ACTV_EXPIRED, ACTV_HOST, ACTV_NONEXISTENT, ACTV_NONEXISTENT_RESPONSE) = range(7)
N_KINDS = 7
OUT_NAMES = ("kind", "ctx", "status", "new_idx", "gone_idx", "n_proposed")


class Batch:
    """One batch; None = the optional array is not passed.  entries: {ActivationId (3 ints): (ctx, flags)}, the
    activation directory when the batch starts."""

    def __init__(self, ctx, recv_status, target_activation, n_ctx, cap_new, entries, ctx_base=0, new_ctx=None,
                 direction=None, ttl=None, new_placement=None, terminating=False):
        self.ctx = np.ascontiguousarray(ctx, dtype=np.uint32)
        self.recv_status = np.ascontiguousarray(recv_status, dtype=np.uint8)
        self.target_activation = np.ascontiguousarray(target_activation, dtype=np.uint64).reshape(-1, 3)
        opt = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
        self.direction, self.ttl = opt(direction, np.uint8), opt(ttl, np.int64)
        self.new_placement, self.new_ctx = opt(new_placement, np.uint8), opt(new_ctx, np.uint32)
        self.n_ctx, self.cap_new, self.ctx_base = int(n_ctx), int(cap_new), int(ctx_base)
        self.terminating = bool(terminating)
        self.entries = dict(entries)

    @property
    def n(self):
        return len(self.ctx)

    def keys(self):
        return [tuple(int(x) for x in k) for k in self.target_activation]

    def proposal(self, k):
        return int(self.new_ctx[k]) if self.new_ctx is not None else self.ctx_base + k


def _result(b, kind, ctx, st, entries, n_prop, err_range):
    new_idx = np.flatnonzero(kind == ACTV_CREATED).astype(np.uint32)
    gone_idx = np.flatnonzero(kind == ACTV_NONEXISTENT).astype(np.uint32)
    return dict(kind=kind, ctx=ctx, status=st, new_idx=new_idx, gone_idx=gone_idx, n_proposed=n_prop, entries=entries,
                err_range=err_range)


def _refused(b, n_prop):
    """n_proposed > cap_new, or one of the first cap_new proposals >= n_ctx."""
    bad = any(b.proposal(k) >= b.n_ctx for k in range(min(n_prop, b.cap_new)))
    return n_prop > b.cap_new or bad, bad


def activate_loop(b: Batch) -> dict:
    """The rule, one message at a time over a dict (lock (activations), Catalog/Catalog.cs:443-518)."""
    n = b.n
    keys = b.keys()
    ttl = [int(TTL_NONE)] * n if b.ttl is None else b.ttl.tolist()
    dr = [0] * n if b.direction is None else b.direction.tolist()
    npl = [0] * n if b.new_placement is None else b.new_placement.tolist()

    def run(create):
        act = dict(b.entries)
        kind = np.zeros(n, np.uint8)
        ctx, st = b.ctx.copy(), b.recv_status.copy()
        k = 0
        err = False
        for i in range(n):
            if b.recv_status[i] != RECV_NULL_CONTEXT:
                continue                                      # ACTV_NONE, copied through
            if ttl[i] != int(TTL_NONE) and ttl[i] <= 0:       # Core/Dispatcher.cs:79-85
                kind[i] = ACTV_EXPIRED
                continue
            gone = ACTV_NONEXISTENT_RESPONSE if dr[i] == DIR_RESPONSE else ACTV_NONEXISTENT
            # a candidate takes a proposal whether or not an earlier one of its id created the entry (sparse)
            cand = keys[i] not in b.entries and npl[i] == 1 and not b.terminating
            mine = k
            k += 1 if cand else 0
            e = act.get(keys[i])
            if e is not None and not (e[1] & AD_SYSTEM_TARGET):       # TryGetActivationData, any state
                if e[0] >= b.n_ctx:
                    kind[i], err = ACTV_HOST, True
                else:
                    kind[i], ctx[i], st[i] = ACTV_FOUND, e[0], RECV_ACTIVATION
            elif e is not None:
                kind[i] = ACTV_HOST                           # only a system target: the other dictionary
            elif not create:
                kind[i] = ACTV_HOST                           # the batch is refused whole
            elif cand:                                        # RegisterMessageTarget -> RecordNewTarget
                act[keys[i]] = (b.proposal(mine), 0)
                kind[i], ctx[i], st[i] = ACTV_CREATED, b.proposal(mine), RECV_ACTIVATION
            else:
                kind[i] = gone                                # NonExistentActivationException
        return kind, ctx, st, act, k, err

    n_prop = run(False)[4]
    refused, bad = _refused(b, n_prop)
    kind, ctx, st, act, _, err = run(not refused)
    return _result(b, kind, ctx, st, act, n_prop, err or bad)


def activate_closed(b: Batch) -> dict:
    """The closed form: per id absent at the start, f = its first non-expired candidate; non-expired messages
    before f are NONEXISTENT(_RESPONSE), f is CREATED, those after f FOUND with f's proposal."""
    n = b.n
    keys = b.keys()
    part = b.recv_status == RECV_NULL_CONTEXT
    ttl = np.full(n, TTL_NONE, np.int64) if b.ttl is None else b.ttl
    expired = (ttl != TTL_NONE) & (ttl <= 0)
    resp = np.zeros(n, bool) if b.direction is None else b.direction == DIR_RESPONSE
    npl = np.zeros(n, bool) if b.new_placement is None else b.new_placement == 1
    live = part & ~expired
    present = np.array([k in b.entries for k in keys], bool).reshape(n)
    cand = live & ~present & npl & (not b.terminating)
    kind = np.zeros(n, np.uint8)
    ctx, st = b.ctx.copy(), b.recv_status.copy()
    kind[part & expired] = ACTV_EXPIRED
    err = False
    for i in np.flatnonzero(live & present):
        c, fl = b.entries[keys[i]]
        if fl & AD_SYSTEM_TARGET or c >= b.n_ctx:
            kind[i] = ACTV_HOST
            err |= not (fl & AD_SYSTEM_TARGET)
        else:
            kind[i], ctx[i], st[i] = ACTV_FOUND, c, RECV_ACTIVATION
    n_prop = int(cand.sum())
    refused, bad = _refused(b, n_prop)
    entries = dict(b.entries)
    undecided = live & ~present
    if refused:
        kind[undecided] = ACTV_HOST
    else:
        rank = np.cumsum(cand) - 1                            # a candidate's proposal index
        first = {}
        for i in np.flatnonzero(cand):
            first.setdefault(keys[i], int(i))
        for i in np.flatnonzero(undecided):
            f = first.get(keys[i])
            if f is None or i < f:
                kind[i] = ACTV_NONEXISTENT_RESPONSE if resp[i] else ACTV_NONEXISTENT
            else:
                p = b.proposal(int(rank[f]))
                kind[i], ctx[i], st[i] = (ACTV_CREATED if i == f else ACTV_FOUND), p, RECV_ACTIVATION
        for k, f in first.items():
            entries[k] = (b.proposal(int(rank[f])), 0)
    return _result(b, kind, ctx, st, entries, n_prop, err or bad)


def bucket_resolved(ctx, n_ctx):
    """gd_receive's bucketing of the resolved contexts: (perm, offsets[n_ctx + 3])."""
    key = np.where(ctx != NONE32, ctx.astype(np.int64), n_ctx + 1)
    perm = np.argsort(key, kind="stable").astype(np.uint32)
    offsets = np.zeros(n_ctx + 3, np.uint32)
    offsets[1:] = np.cumsum(np.bincount(key, minlength=n_ctx + 2))
    return perm, offsets


def chain_model(b: Batch, ctx_flags, num_running, request_count, forward_count=None, msg_flags=None,
                sending_activation=None, max_forward_count=2, chain=False, form=activate_loop, turns=T.turns_loop):
    """receive's (ctx, status) in b -> activate -> the bucketing of the resolved contexts -> the turn stage on them.
    The activation outputs, then perm / offsets, then turns_loop's six."""
    a = form(b)
    perm, offs = bucket_resolved(a["ctx"], b.n_ctx)
    tb = T.Batch(a["ctx"], b.n_ctx, ctx_flags, num_running, request_count, a["status"], b.direction, b.ttl,
                 forward_count, msg_flags, b.target_activation, sending_activation, 0, 0, max_forward_count, chain)
    names = ("turn", "num_running_out", "running_idx", "start_idx", "wait_perm", "wait_offsets")
    return dict(a, perm=perm, offsets=offs, **dict(zip(names, turns(tb))))


# ---- generators ---------------------------------------------------------------------------------

def act_keys(rng, m):
    """m distinct ActivationIds (UniqueKey words)."""
    k = rng.integers(1, 1 << 62, size=(m, 3), dtype=np.int64).astype(np.uint64)
    k[:, 0] = np.arange(1, m + 1, dtype=np.uint64) + (k[:, 0] << np.uint64(20))       # distinct
    return k


def scene(rng, n, n_ctx=None, n_existing=12, n_system=3, n_absent=None, p_part=0.85, terminating=False, given=True,
          hot=None):
    """A batch with every case: existing activations (Valid and not), system-target entries, absent ids with and
    without IsNewPlacement, expired candidates, responses.  The first messages script one absent id: a request before
    its creator, an expired candidate, the creator, candidates and plain messages after it.  hot: arrival indices
    that all target one more absent id (its creator is not the first of them).  Returns (Batch, scripted id, hot id)."""
    n_absent = max(4, n // 6) if n_absent is None else n_absent
    n_ctx = n + n_existing + 8 if n_ctx is None else n_ctx
    keys = act_keys(rng, n_existing + n_system + n_absent + 2)
    ex, sy = keys[:n_existing], keys[n_existing:n_existing + n_system]
    ab = keys[n_existing + n_system:-2]
    scripted, hot_id = keys[-2], keys[-1]
    entries = {}
    for j, k in enumerate(ex):
        entries[tuple(int(x) for x in k)] = (j, int(rng.integers(0, 2)) * AD_VALID | (AD_STATELESS_WORKER if j % 5 == 4 else 0))
    for j, k in enumerate(sy):
        entries[tuple(int(x) for x in k)] = (n_existing + j, AD_SYSTEM_TARGET | AD_VALID)
    u = rng.random(n)
    pick = np.where(u < 0.25, 0, np.where(u < 0.32, 1, 2))
    ta = np.empty((n, 3), np.uint64)
    ta[pick == 0] = ex[rng.integers(0, n_existing, int((pick == 0).sum()))]
    ta[pick == 1] = sy[rng.integers(0, n_system, int((pick == 1).sum()))]
    ta[pick == 2] = ab[rng.integers(0, len(ab), int((pick == 2).sum()))]
    rs = np.where(rng.random(n) < p_part, RECV_NULL_CONTEXT, rng.choice(np.array([0, 1, 3, 4, 5, 6], np.uint8), n)).astype(np.uint8)
    ctx = np.where(rs == RECV_NULL_CONTEXT, n_ctx, np.where(rs <= 1, rng.integers(0, n_existing, n), NONE32)).astype(np.uint32)
    dr = rng.choice(np.array([0, 0, 0, 1, 2, 0xFF], np.uint8), size=n)
    ttl = np.where(rng.random(n) < 0.75, TTL_NONE, rng.integers(-3, 20, n)).astype(np.int64)
    npl = rng.choice(np.array([0, 1, 1, 1, 2], np.uint8), size=n)
    script = [(0, TTL_NONE, 0), (1, TTL_NONE, 0), (0, 0, 1), (0, TTL_NONE, 1), (0, 5, 1), (1, TTL_NONE, 1), (2, TTL_NONE, 0)]
    for i, (d, t, p) in enumerate(script[:n]):
        ta[i], rs[i], ctx[i], dr[i], ttl[i], npl[i] = scripted, RECV_NULL_CONTEXT, n_ctx, d, t, p
    if hot is not None:
        hot = [i for i in hot if len(script) <= i < n]
        for j, i in enumerate(hot):
            # two plain requests, then candidates and plain messages alternating
            ta[i], rs[i], ctx[i], dr[i], ttl[i] = hot_id, RECV_NULL_CONTEXT, n_ctx, 0, TTL_NONE
            npl[i] = 0 if j < 2 else (1 if j % 2 == 0 else 0)
    new_ctx = None
    base = n_existing + n_system
    cap = int(((rs == RECV_NULL_CONTEXT) & (npl == 1)).sum())
    if given:                                                 # distinct free contexts, not in order
        new_ctx = (base + rng.permutation(n_ctx - base)[:cap]).astype(np.uint32) if n_ctx - base >= cap else None
    b = Batch(ctx, rs, ta, n_ctx, cap, entries, ctx_base=base, new_ctx=new_ctx, direction=dr, ttl=ttl, new_placement=npl,
              terminating=terminating)
    return b, tuple(int(x) for x in scripted), tuple(int(x) for x in hot_id)


def assert_scene_cases(b: Batch, r: dict, scripted, hot_id=None):
    """The cases a scene of a few hundred messages must contain."""
    kind = r["kind"]
    keys = b.keys()
    assert set(range(N_KINDS)) <= set(kind.tolist()), sorted(set(kind.tolist()))
    s = [i for i, k in enumerate(keys) if k == scripted]
    assert kind[s[0]] == ACTV_NONEXISTENT and kind[s[1]] == ACTV_NONEXISTENT_RESPONSE      # before the creator
    assert kind[s[2]] == ACTV_EXPIRED and kind[s[3]] == ACTV_CREATED                       # expired candidate, live one
    assert all(kind[i] == ACTV_FOUND for i in s[4:7]) and r["ctx"][s[4]] == r["ctx"][s[3]]
    assert b.new_placement[s[4]] == 1 and b.new_placement[s[6]] == 0                       # both sorts after it
    assert r["n_proposed"] > len(r["new_idx"]) > 0                                         # proposals are sparse
    states = {b.entries[keys[i]][1] & AD_VALID for i in np.flatnonzero(kind == ACTV_FOUND) if keys[i] in b.entries}
    assert states == {0, 1}
    assert any(keys[i] in b.entries for i in np.flatnonzero(kind == ACTV_HOST))            # the system-target corner
    if hot_id is not None:
        hs = [i for i, k in enumerate(keys) if k == hot_id]
        c = [i for i in hs if kind[i] == ACTV_CREATED]
        assert len(c) == 1 and hs[0] < c[0] and any(b.new_placement[i] == 1 for i in hs if i > c[0])
        assert all(kind[i] == ACTV_NONEXISTENT for i in hs if i < c[0])
        assert all(kind[i] == ACTV_FOUND for i in hs if i > c[0])
