"""Dispatcher.ReceiveMessage -> ReceiveRequest for a received batch, restated per message: the turn
admission every request gets under lock(activation) after IncomingMessageAgent.ReceiveMessage
(gd_receive) has found its activation.  Paths are the reference's, under src/Orleans.Runtime/.

turns_loop is the literal loop in arrival order; turns_np the vectorised closed form the kernels
follow (tests/test_turns_ref.py proves the two equal).  Constants mirror include/graindispatch.h.

request_count[c] is ActivationData.GetRequestCount() of context c once the agent has enqueued the
whole batch: gd_receive's start value (gd_recv_limits.request_count[c]) plus the messages gd_receive
enqueued on c (offsets[c + 1] - offsets[c] of its bucketing) -- see request_count_after_receive.

Left to C# (not modelled): deadlock detection (Core/Dispatcher.cs:277-293, off by default), the
interface-version check of HandleIncomingRequest (:403-410), TryRescheduleCollection (:118), logging
and statistics, and the cross-cluster return in TryForwardRequest.
"""
import numpy as np

NONE32 = 0xFFFFFFFF
TTL_NONE = np.iinfo(np.int64).max

RECV_ACTIVATION = 0

DIR_REQUEST, DIR_RESPONSE, DIR_ONE_WAY, DIR_ABSENT = 0, 1, 2, 0xFF

MSG_READ_ONLY, MSG_ALWAYS_INTERLEAVE, MSG_MAY_INTERLEAVE = 1, 2, 4

CTX_VALID, CTX_NOT_READY, CTX_INVALID, CTX_STATE_MASK = 0, 1, 2, 3
CTX_HAS_RUNNING, CTX_RUNNING_READ_ONLY, CTX_REENTRANT, CTX_STATELESS_WORKER, CTX_STUCK = 4, 8, 16, 32, 64

(TURN_NONE, TURN_START, TURN_WAIT, TURN_REJECT_OVERLOADED, TURN_STUCK, TURN_FORWARD, TURN_REJECT_TRANSIENT,
 TURN_EXPIRED, TURN_RESPONSE, TURN_RESPONSE_DROPPED) = range(10)
N_TURNS = 10


class Batch:
    """One batch and its context state; None = the optional array is not passed."""

    def __init__(self, ctx, n_ctx, ctx_flags, num_running, request_count, recv_status=None, direction=None, ttl=None,
                 forward_count=None, msg_flags=None, target_activation=None, sending_activation=None, hard_limit=0,
                 hard_limit_sw=0, max_forward_count=2, chain=False):
        self.ctx = np.ascontiguousarray(ctx, dtype=np.uint32)
        self.n_ctx = int(n_ctx)
        self.ctx_flags = np.ascontiguousarray(ctx_flags, dtype=np.uint8)
        self.num_running = np.ascontiguousarray(num_running, dtype=np.uint32)
        self.request_count = np.ascontiguousarray(request_count, dtype=np.uint32)
        opt = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
        self.recv_status = opt(recv_status, np.uint8)
        self.direction = opt(direction, np.uint8)
        self.ttl = opt(ttl, np.int64)
        self.forward_count = opt(forward_count, np.uint8)
        self.msg_flags = opt(msg_flags, np.uint8)
        self.target_activation = None if target_activation is None else \
            np.ascontiguousarray(target_activation, dtype=np.uint64).reshape(-1, 3)
        self.sending_activation = None if sending_activation is None else \
            np.ascontiguousarray(sending_activation, dtype=np.uint64).reshape(-1, 3)
        self.hard_limit, self.hard_limit_sw = int(hard_limit), int(hard_limit_sw)
        self.max_forward_count, self.chain = int(max_forward_count), bool(chain)
        assert len(self.ctx_flags) == len(self.num_running) == len(self.request_count) == self.n_ctx

    @property
    def n(self):
        return len(self.ctx)

    def explicit(self):
        """The same batch with every optional array spelled out as its default."""
        n = self.n
        d = lambda a, v, t: np.full(n, v, t) if a is None else a
        return Batch(self.ctx, self.n_ctx, self.ctx_flags, self.num_running, self.request_count,
                     d(self.recv_status, RECV_ACTIVATION, np.uint8), d(self.direction, DIR_REQUEST, np.uint8),
                     d(self.ttl, TTL_NONE, np.int64), d(self.forward_count, 0, np.uint8), d(self.msg_flags, 0, np.uint8),
                     self.target_activation, self.sending_activation, self.hard_limit, self.hard_limit_sw,
                     self.max_forward_count, self.chain)


def request_count_after_receive(request_count_before, recv_offsets, n_ctx):
    """GetRequestCount() per context after IncomingMessageAgent enqueued the batch (IncrementEnqueuedOn
    DispatcherCount, Messaging/IncomingMessageAgent.cs:176-181): gd_receive's start value plus the messages
    its bucketing put on the context."""
    off = np.asarray(recv_offsets, dtype=np.int64)
    return (np.asarray(request_count_before, dtype=np.int64) + off[1:n_ctx + 1] - off[:n_ctx]).astype(np.uint32)


def _bucket_wait(turn, ctx, n_ctx):
    """Stable bucketing of the WAIT messages by context, every other message in the trailing bucket n_ctx:
    wait_perm[n], wait_offsets[n_ctx + 2] (gd_bucket's layout: bucket c = [off[c], off[c + 1]), off[-1] = n)."""
    n = len(turn)
    key = np.where(turn == TURN_WAIT, ctx.astype(np.int64), n_ctx)
    perm = np.argsort(key, kind="stable").astype(np.uint32)
    off = np.zeros(n_ctx + 2, np.uint32)
    off[1:] = np.cumsum(np.bincount(key, minlength=n_ctx + 1)).astype(np.uint32)
    return perm, off


def _participating(b):
    part = b.ctx < b.n_ctx
    if b.recv_status is not None:
        part &= b.recv_status == RECV_ACTIVATION
    return part


def turns_loop(b):
    """(turn u8[n], num_running_out u32[n_ctx], running_idx u32[n_ctx], start_idx u32[n_start],
    wait_perm u32[n], wait_offsets u32[n_ctx + 2])."""
    n, n_ctx = b.n, b.n_ctx
    turn = np.zeros(n, np.uint8)
    num_running = [int(x) for x in b.num_running]
    has_running = [bool(f & CTX_HAS_RUNNING) for f in b.ctx_flags]
    running_ro = [bool(f & CTX_RUNNING_READ_ONLY) for f in b.ctx_flags]
    count = [int(x) for x in b.request_count]
    running_idx = np.full(n_ctx, NONE32, np.uint32)
    start_idx = []
    # plain lists: the loop reads one element at a time
    ls = lambda a: None if a is None else a.tolist()
    l_ctx, l_rs, l_dir, l_ttl, l_fwd, l_mf = (ls(b.ctx), ls(b.recv_status), ls(b.direction), ls(b.ttl),
                                              ls(b.forward_count), ls(b.msg_flags))
    l_flags = b.ctx_flags.tolist()
    l_same = None
    if b.chain and b.target_activation is not None:       # ActivationId.Equals, all three words
        l_same = (b.target_activation == b.sending_activation).all(axis=1).tolist()
    for i in range(n):
        c = l_ctx[i]
        # only what IncomingMessageAgent enqueued on an activation's context reaches Dispatcher.ReceiveMessage
        # with that activation (Messaging/IncomingMessageAgent.cs:136-152)
        if c >= n_ctx or (l_rs is not None and l_rs[i] != RECV_ACTIVATION):
            turn[i] = TURN_NONE
            continue
        f = l_flags[c]
        state = f & CTX_STATE_MASK
        d = DIR_REQUEST if l_dir is None else l_dir[i]
        if d == DIR_ABSENT:                               # Message.Direction's default (Message.cs:113-116)
            d = DIR_REQUEST
        ttl = TTL_NONE if l_ttl is None else l_ttl[i]
        mf = 0 if l_mf is None else l_mf[i]
        fwd = 0 if l_fwd is None else l_fwd[i]
        if ttl != TTL_NONE and ttl <= 0:                  # Core/Dispatcher.cs:79-85, Message.cs:293-302
            t = TURN_EXPIRED
        elif d == DIR_RESPONSE:                           # ReceiveResponse, Core/Dispatcher.cs:238-254
            t = TURN_RESPONSE_DROPPED if state == CTX_INVALID else TURN_RESPONSE
        elif state == CTX_INVALID:                        # ReceiveRequest :266-273 -> ProcessRequestToInvalidActivation
            # TryForwardRequest: MayForward (:627-630), else the transient rejection (:563-568)
            t = TURN_FORWARD if fwd < b.max_forward_count else TURN_REJECT_TRANSIENT
        else:
            same = l_same is not None and l_same[i]
            # CanInterleave, Core/Dispatcher.cs:326-336; catalog.CanInterleave = IsReentrant || MayInterleave
            # (Catalog/Catalog.cs:409-417)
            can_interleave = (bool(mf & MSG_ALWAYS_INTERLEAVE) or not has_running[c] or
                              (running_ro[c] and bool(mf & MSG_READ_ONLY)) or same or bool(f & CTX_REENTRANT) or
                              bool(mf & MSG_MAY_INTERLEAVE))
            # ActivationMayAcceptRequest, :313-318; IsCurrentlyExecuting = numRunning > 0 (ActivationData.cs:470)
            if state == CTX_VALID and (num_running[c] == 0 or can_interleave):
                t = TURN_START                            # HandleIncomingRequest :399-424
                num_running[c] += 1                       # RecordRunning, Catalog/ActivationData.cs:475-493
                if not has_running[c]:
                    has_running[c] = True
                    running_ro[c] = bool(mf & MSG_READ_ONLY)
                    running_idx[c] = i
                start_idx.append(i)
            else:                                         # EnqueueRequest :431-466
                limit = b.hard_limit_sw if f & CTX_STATELESS_WORKER else b.hard_limit
                if limit > 0 and count[c] > limit:        # CheckOverloaded, Catalog/ActivationData.cs:616-649
                    t = TURN_REJECT_OVERLOADED
                elif f & CTX_STUCK:                       # EnqueueMessage, Catalog/ActivationData.cs:576-594
                    t = TURN_STUCK
                else:
                    t = TURN_WAIT
                    count[c] += 1                         # waiting.Add: GetRequestCount counts the waiting list
        count[c] -= 1                                     # the closure's finally, Messaging/IncomingMessageAgent.cs:184-187
        turn[i] = t
    perm, off = _bucket_wait(turn, b.ctx, n_ctx)
    return (turn, np.array(num_running, np.uint32).reshape(n_ctx), running_idx, np.array(start_idx, np.uint32), perm,
            off)


def turns_np(b):
    """The closed form.  Per context, with F = its first participating, unexpired Request / OneWay on a
    state that is not INVALID ("eligible"):
      - !HAS_RUNNING: F starts and becomes Running; a later eligible message is accepted iff it interleaves
        with Running = F, whose read-only flag is the message's own;
      - HAS_RUNNING: Running never changes; F is accepted outright when num_running starts at 0, every other
        eligible message iff it interleaves with the Running the batch started with;
      - count never rises along a context (each step changes it by -1 or 0), so a would-wait message of rank
        j among the context's participating messages is rejected iff request_count[c] - j > limit.
    """
    n, n_ctx = b.n, b.n_ctx
    part = _participating(b)
    c = np.where(part, b.ctx, 0).astype(np.int64)
    if n_ctx == 0:
        z = np.zeros(n, np.uint8)
        perm, off = _bucket_wait(z, b.ctx, 0)
        return z, np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32), perm, off
    f = b.ctx_flags[c].astype(np.int64)
    state = f & CTX_STATE_MASK
    d = np.zeros(n, np.int64) if b.direction is None else b.direction.astype(np.int64)
    d = np.where(d == DIR_ABSENT, DIR_REQUEST, d)
    ttl = np.full(n, TTL_NONE, np.int64) if b.ttl is None else b.ttl
    mf = np.zeros(n, np.int64) if b.msg_flags is None else b.msg_flags.astype(np.int64)
    fwd = np.zeros(n, np.int64) if b.forward_count is None else b.forward_count.astype(np.int64)
    expired = (ttl != TTL_NONE) & (ttl <= 0)
    resp = d == DIR_RESPONSE
    turn = np.zeros(n, np.uint8)
    live = part & ~expired
    turn[part & expired] = TURN_EXPIRED
    turn[live & resp] = TURN_RESPONSE
    turn[live & resp & (state == CTX_INVALID)] = TURN_RESPONSE_DROPPED
    req = live & ~resp
    inv = req & (state == CTX_INVALID)
    turn[inv & (fwd < b.max_forward_count)] = TURN_FORWARD
    turn[inv & (fwd >= b.max_forward_count)] = TURN_REJECT_TRANSIENT
    elig = req & (state != CTX_INVALID)
    evalid = elig & (state == CTX_VALID)
    idx = np.arange(n, dtype=np.int64)
    # the first eligible message per VALID context (an order-dependent minimum over arrival index)
    first = np.full(n_ctx, n, np.int64)
    np.minimum.at(first, c[evalid], idx[evalid])
    same = np.zeros(n, bool)
    if b.chain and b.target_activation is not None:
        same = (b.target_activation == b.sending_activation).all(axis=1)
    static = ((mf & MSG_ALWAYS_INTERLEAVE) != 0) | same | ((f & CTX_REENTRANT) != 0) | ((mf & MSG_MAY_INTERLEAVE) != 0)
    ro = (mf & MSG_READ_ONLY) != 0
    has = (f & CTX_HAS_RUNNING) != 0
    fc = first[c]
    is_first = fc == idx
    first_ro = ro[np.minimum(fc, max(n - 1, 0))] if n else ro
    nr0 = b.num_running[c].astype(np.int64)
    acc_idle = is_first | static | (ro & first_ro)
    acc_busy = static | (ro & ((f & CTX_RUNNING_READ_ONLY) != 0)) | ((nr0 == 0) & is_first)
    accept = evalid & np.where(has, acc_busy, acc_idle)
    turn[accept] = TURN_START
    notacc = elig & ~accept
    # rank among the context's participating messages
    key = np.where(part, c, n_ctx)
    order = np.argsort(key, kind="stable")
    starts = np.zeros(n_ctx + 2, np.int64)
    starts[1:] = np.cumsum(np.bincount(key, minlength=n_ctx + 1))
    rank = np.empty(n, np.int64)
    rank[order] = idx - starts[key[order]]
    limit = np.where((f & CTX_STATELESS_WORKER) != 0, b.hard_limit_sw, b.hard_limit)
    over = notacc & (limit > 0) & (b.request_count[c].astype(np.int64) - rank > limit)
    stuck = notacc & ~over & ((f & CTX_STUCK) != 0)
    turn[over] = TURN_REJECT_OVERLOADED
    turn[stuck] = TURN_STUCK
    turn[notacc & ~over & ~stuck] = TURN_WAIT
    num_running = b.num_running.astype(np.int64) + np.bincount(c[accept], minlength=n_ctx)
    vctx = (b.ctx_flags & CTX_STATE_MASK) == CTX_VALID
    running_idx = np.where(vctx & ((b.ctx_flags & CTX_HAS_RUNNING) == 0) & (first < n), first, NONE32).astype(np.uint32)
    perm, off = _bucket_wait(turn, b.ctx, n_ctx)
    return turn, num_running.astype(np.uint32), running_idx, idx[accept].astype(np.uint32), perm, off


# ---- generators ---------------------------------------------------------------------------------

def zipf_targets(rng, n, n_ctx, a=1.1):
    w = 1.0 / np.arange(1, n_ctx + 1, dtype=np.float64) ** a
    return rng.choice(n_ctx, size=n, p=w / w.sum()).astype(np.uint32)


def context_state(rng, n_ctx, busy=0.4, invalid=0.1, not_ready=0.1):
    """(ctx_flags, num_running): a plausible mix, including num_running > 0 with no Running and Running with
    num_running == 0 (the rule reads the two independently)."""
    u = rng.random(n_ctx)
    state = np.where(u < invalid, CTX_INVALID, np.where(u < invalid + not_ready, CTX_NOT_READY, CTX_VALID))
    fl = state.astype(np.uint8)
    has = rng.random(n_ctx) < busy
    fl |= np.where(has, CTX_HAS_RUNNING, 0).astype(np.uint8)
    fl |= np.where(has & (rng.random(n_ctx) < 0.5), CTX_RUNNING_READ_ONLY, 0).astype(np.uint8)
    fl |= np.where(rng.random(n_ctx) < 0.15, CTX_REENTRANT, 0).astype(np.uint8)
    fl |= np.where(rng.random(n_ctx) < 0.2, CTX_STATELESS_WORKER, 0).astype(np.uint8)
    fl |= np.where(rng.random(n_ctx) < 0.1, CTX_STUCK, 0).astype(np.uint8)
    nr = np.where(has, rng.integers(0, 3, n_ctx), rng.integers(0, 2, n_ctx) * (rng.random(n_ctx) < 0.2)).astype(np.uint32)
    return fl, nr


def mixed_batch(rng, n, n_ctx, targets="uniform", limits=True, chain=True):
    """Every rule line in one batch: all turn values and all three states once n and n_ctx are a few hundred."""
    if targets == "zipf":
        ctx = zipf_targets(rng, n, n_ctx)
    else:
        ctx = rng.integers(0, n_ctx, size=n).astype(np.uint32)
    fl, nr = context_state(rng, n_ctx)
    u = rng.random(n)
    ctx = np.where(u < 0.03, NONE32, np.where(u < 0.05, n_ctx, ctx)).astype(np.uint32)
    rs = np.where(rng.random(n) < 0.05, rng.integers(1, 7, n), RECV_ACTIVATION).astype(np.uint8)
    dr = rng.choice(np.array([0, 0, 0, 0, 1, 2, 0xFF], np.uint8), size=n)
    ttl = np.where(rng.random(n) < 0.7, TTL_NONE, rng.integers(-5, 50, n)).astype(np.int64)
    fwd = rng.integers(0, 4, n).astype(np.uint8)
    mf = (rng.integers(0, 2, n) * MSG_READ_ONLY | (rng.random(n) < 0.1) * MSG_ALWAYS_INTERLEAVE |
          (rng.random(n) < 0.1) * MSG_MAY_INTERLEAVE).astype(np.uint8)
    ta = rng.integers(0, 1 << 62, size=(n, 3), dtype=np.uint64)
    sa = rng.integers(0, 1 << 62, size=(n, 3), dtype=np.uint64)
    eq = rng.random(n) < 0.1
    sa[eq] = ta[eq]
    near = rng.random(n) < 0.1                          # equal but for the last word
    sa[near, :2] = ta[near, :2]
    # request counts around the limits so the reject / wait boundary falls inside the contexts' runs
    per = max(1, n // max(n_ctx, 1))
    rc = rng.integers(0, 2 * per + 8, n_ctx).astype(np.uint32)
    hl, hls = (per + 3, per // 2 + 2) if limits else (0, 0)
    return Batch(ctx, n_ctx, fl, nr, rc, rs, dr, ttl, fwd, mf, ta, sa, hl, hls, 2, chain)
