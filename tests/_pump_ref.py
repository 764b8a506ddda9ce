"""Dispatcher.OnActivationCompletedRequest for a batch of completions, restated: ResetRunning, then
RunMessagePump over the activation's waiting list.  Paths are the reference's, under
src/Orleans.Runtime/.

pump_loop is the literal loop of include/graindispatch.h's completion block, in arrival order; pump_np
walks each context by regimes as the kernels do (tests/test_pump_ref.py proves the two equal);
merge_loop keeps the waiting lists' CSR between steps; Activation restates RecordRunning / ResetRunning /
EnqueueMessage / RunMessagePump per message object, from the C# and not from the loop.

numRunning is an int: it is kept as a two's-complement int32 and stored in the uint32 arrays.

Left to C# (not modelled): RunningRequestsSenders, the interface-version check of HandleIncomingRequest,
TryRescheduleCollection / RunOnInactive (reported as PUMP_BECAME_IDLE), logging.
"""
import numpy as np

from _turns_ref import (CTX_HAS_RUNNING, CTX_REENTRANT, CTX_RUNNING_READ_ONLY, CTX_STATE_MASK, CTX_VALID,
                        MSG_ALWAYS_INTERLEAVE, MSG_MAY_INTERLEAVE, MSG_READ_ONLY, NONE32, zipf_targets, context_state)

MSG_CALL_CHAIN = 8
DONE_IS_RUNNING, DONE_PUMP_ONLY = 1, 2
PUMP_BECAME_IDLE, PUMP_RUNNING_CLEARED, PUMP_RUNNING_SET = 1, 2, 4
_STATIC = MSG_ALWAYS_INTERLEAVE | MSG_MAY_INTERLEAVE | MSG_CALL_CHAIN

NAMES = ("num_running_out", "ctx_flags_out", "n_dequeued", "running_pos", "event", "n_started_by", "start_pos")


def _i32(x):
    """int arithmetic of the C# field: wraps at 32 bits."""
    return ((int(x) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


class PumpBatch:
    """A batch of completions, the context state and the waiting lists; done_flags None = not passed."""

    def __init__(self, done_ctx, n_ctx, ctx_flags, num_running, offsets, wflags, done_flags=None, wmsg=None):
        self.done_ctx = np.ascontiguousarray(done_ctx, dtype=np.uint32)
        self.n_ctx = int(n_ctx)
        self.ctx_flags = np.ascontiguousarray(ctx_flags, dtype=np.uint8)
        self.num_running = np.ascontiguousarray(num_running, dtype=np.uint32)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        self.wflags = np.ascontiguousarray(wflags, dtype=np.uint8)
        self.wmsg = np.arange(len(self.wflags), dtype=np.uint32) if wmsg is None else \
            np.ascontiguousarray(wmsg, dtype=np.uint32)
        self.done_flags = None if done_flags is None else np.ascontiguousarray(done_flags, dtype=np.uint8)
        assert len(self.ctx_flags) == len(self.num_running) == self.n_ctx and len(self.offsets) == self.n_ctx + 1
        assert int(self.offsets[-1]) == len(self.wflags) == len(self.wmsg)

    @property
    def n_done(self):
        return len(self.done_ctx)


def _flags_out(f, rk, ro):
    return (f & ~(CTX_HAS_RUNNING | CTX_RUNNING_READ_ONLY)) | (CTX_HAS_RUNNING if rk else 0) | \
        (CTX_RUNNING_READ_ONLY if rk and ro else 0)


def pump_loop(b):
    """(num_running_out u32[n_ctx], ctx_flags_out u8[n_ctx], n_dequeued u32[n_ctx], running_pos u32[n_ctx],
    event u8[n_ctx], n_started_by u32[n_done], start_pos u32[n_start])."""
    n_ctx, n_done = b.n_ctx, b.n_done
    off = b.offsets.tolist()
    wf = b.wflags.tolist()
    cf = b.ctx_flags.tolist()
    nr = [_i32(x) for x in b.num_running.tolist()]
    rk = [1 if f & CTX_HAS_RUNNING else 0 for f in cf]        # 0 none, 1 the batch-start Running X, 2 a waiting position
    ro = [bool(f & CTX_RUNNING_READ_ONLY) for f in cf]
    rpos = [NONE32] * n_ctx
    p = off[:n_ctx]
    ev = [0] * n_ctx
    touched = [False] * n_ctx
    nsb = [0] * n_done
    start_pos = []
    l_ctx = b.done_ctx.tolist()
    l_df = None if b.done_flags is None else b.done_flags.tolist()
    for i in range(n_done):
        c = l_ctx[i]
        if c >= n_ctx:
            continue
        touched[c] = True
        df = 0 if l_df is None else l_df[i]
        if not df & DONE_PUMP_ONLY:                           # ResetRunning, Catalog/ActivationData.cs:495-514
            nr[c] = _i32(nr[c] - 1)
            if nr[c] == 0:
                ev[c] |= PUMP_BECAME_IDLE
            if rk[c] == 1 and df & DONE_IS_RUNNING:           # Running != null && !message.Equals(Running): return
                rk[c] = 0
                ev[c] |= PUMP_RUNNING_CLEARED
        if cf[c] & CTX_STATE_MASK != CTX_VALID:               # RunMessagePump, Core/Dispatcher.cs:858
            continue
        while p[c] < off[c + 1]:                              # PeekNextWaitingMessage
            f = wf[p[c]]
            # ActivationMayAcceptRequest / CanInterleave, Core/Dispatcher.cs:313-336
            ok = (nr[c] <= 0 or f & MSG_ALWAYS_INTERLEAVE or rk[c] == 0 or (ro[c] and f & MSG_READ_ONLY) or
                  f & MSG_CALL_CHAIN or cf[c] & CTX_REENTRANT or f & MSG_MAY_INTERLEAVE)
            if not ok:
                break
            nr[c] = _i32(nr[c] + 1)                           # DequeueNextWaitingMessage, RecordRunning :475-493
            if rk[c] == 0:
                rk[c], rpos[c], ro[c] = 2, p[c], bool(f & MSG_READ_ONLY)
                ev[c] |= PUMP_RUNNING_SET
            start_pos.append(p[c])
            nsb[i] += 1
            p[c] += 1
    fo = [_flags_out(cf[c], rk[c], ro[c]) if touched[c] else cf[c] for c in range(n_ctx)]
    return (np.array([x & 0xFFFFFFFF for x in nr], np.uint32).reshape(n_ctx), np.array(fo, np.uint8).reshape(n_ctx),
            np.array([p[c] - off[c] for c in range(n_ctx)], np.uint32).reshape(n_ctx),
            np.array([rpos[c] if rk[c] == 2 else NONE32 for c in range(n_ctx)], np.uint32).reshape(n_ctx),
            np.array(ev, np.uint8).reshape(n_ctx), np.array(nsb, np.uint32).reshape(n_done),
            np.array(start_pos, np.uint32))


def pump_np(b):
    """The regime form the kernels follow.  Completions are bucketed by context (stable).  Along a context R
    takes at most the values X -> none -> one waiting position, and after a pump the list head is blocked (or
    the list is empty) until a completion either clears R == X or brings nr to 0: the completions in between
    only lower nr and are skipped in one step (a prefix count of the non-PUMP_ONLY flags against nr).  A pump
    first takes the accepts nr <= 0 / R == none force, then the run of messages the now fixed R accepts: the
    first clear bit of the predicate over the rest of the list."""
    n_ctx, n_done = b.n_ctx, b.n_done
    key = np.minimum(b.done_ctx.astype(np.int64), n_ctx)
    perm = np.argsort(key, kind="stable")
    boff = np.zeros(n_ctx + 2, np.int64)
    boff[1:] = np.cumsum(np.bincount(key, minlength=n_ctx + 1))
    df_all = np.zeros(n_done, np.int64) if b.done_flags is None else b.done_flags.astype(np.int64)
    nr_out = b.num_running.copy()
    fl_out = b.ctx_flags.copy()
    ndq = np.zeros(n_ctx, np.uint32)
    rpos_out = np.full(n_ctx, NONE32, np.uint32)
    ev_out = np.zeros(n_ctx, np.uint8)
    nsb = np.zeros(n_done, np.uint32)
    first = np.zeros(n_done, np.int64)
    off = b.offsets.astype(np.int64)
    for c in np.flatnonzero(boff[1:n_ctx + 1] > boff[:n_ctx]).tolist():
        idx = perm[boff[c]:boff[c + 1]]
        df = df_all[idx]
        m = len(idx)
        f = int(b.ctx_flags[c])
        valid = f & CTX_STATE_MASK == CTX_VALID
        lo, hi = int(off[c]), int(off[c + 1])
        wf = b.wflags[lo:hi].astype(np.int64)
        static = ((wf & _STATIC) != 0) | bool(f & CTX_REENTRANT)
        wro = (wf & MSG_READ_ONLY) != 0
        nr = _i32(b.num_running[c])
        rk, ro, rpos, p, ev = (1 if f & CTX_HAS_RUNNING else 0), bool(f & CTX_RUNNING_READ_ONLY), NONE32, 0, 0
        non_po = (df & DONE_PUMP_ONLY) == 0
        cum = np.cumsum(non_po)                                # non-PUMP_ONLY completions up to and including k
        is_run = non_po & ((df & DONE_IS_RUNNING) != 0)
        k, blocked = 0, not valid                              # a pump that never runs leaves nothing to re-test
        while k < m:
            if blocked:
                base = int(cum[k - 1]) if k else 0
                trig = non_po[k:] & ((cum[k:] - base) == nr)
                if rk == 1:
                    trig = trig | is_run[k:]
                if not trig.any():
                    nr = _i32(nr - (int(cum[-1]) - base))
                    break
                t = k + int(np.argmax(trig))
                nr = _i32(nr - ((int(cum[t - 1]) if t else 0) - base))
                k = t
            if non_po[k]:
                nr = _i32(nr - 1)
                if nr == 0:
                    ev |= PUMP_BECAME_IDLE
                if rk == 1 and is_run[k]:
                    rk = 0
                    ev |= PUMP_RUNNING_CLEARED
            if valid and p < hi - lo:
                p0 = p
                forced = 1 - nr if nr <= 0 else (1 if rk == 0 else 0)
                take = min(forced, hi - lo - p)
                if take:
                    if rk == 0:
                        rk, rpos, ro = 2, lo + p, bool(wro[p])
                        ev |= PUMP_RUNNING_SET
                    nr = _i32(nr + take)
                    p += take
                if take == forced and p < hi - lo:
                    acc = static[p:] | (wro[p:] & ro)
                    run = len(acc) if acc.all() else int(np.argmin(acc))
                    nr = _i32(nr + run)
                    p += run
                if p > p0:
                    nsb[idx[k]] = p - p0
                    first[idx[k]] = lo + p0
            blocked = True
            k += 1
        nr_out[c] = nr & 0xFFFFFFFF
        fl_out[c] = _flags_out(f, rk, ro)
        ndq[c] = p
        rpos_out[c] = rpos if rk == 2 else NONE32
        ev_out[c] = ev
    # the started positions by triggering completion, then FIFO: a run first[i] .. first[i] + n_started_by[i]
    tot = np.cumsum(nsb.astype(np.int64))
    n_start = int(tot[-1]) if n_done else 0
    owner = np.searchsorted(tot, np.arange(n_start), side="right")
    start = first[owner] + (np.arange(n_start) - (tot[owner] - nsb[owner]))
    return nr_out, fl_out, ndq, rpos_out, ev_out, nsb, start.astype(np.uint32)


def merge_loop(n_ctx, old_offsets, old_msg, old_flags, n_dequeued, wait_perm, wait_offsets, msg_id=None, id_base=0,
               msg_flags=None, target_activation=None, sending_activation=None, chain=False, cap=None):
    """(offsets u32[n_ctx + 1], msg u32[min(total, cap)], flags u8[min(total, cap)], total): for every context
    the undequeued rest of its old list, then bucket c of the gd_turns result, both in order.  old_offsets None
    = no old list.  A batch message i gets msg_id[i] (None: id_base + i) and msg_flags[i] (None: 0), plus
    MSG_CALL_CHAIN when chain and its two activation keys are equal."""
    msg, flags, offsets = [], [], [0]
    same = None
    if chain and target_activation is not None:
        same = (np.asarray(target_activation).reshape(-1, 3) == np.asarray(sending_activation).reshape(-1, 3)).all(axis=1)
    for c in range(n_ctx):
        if old_offsets is not None:
            lo, hi = int(old_offsets[c]), int(old_offsets[c + 1])
            lo = min(hi, lo + (0 if n_dequeued is None else int(n_dequeued[c])))
            for q in range(lo, hi):
                msg.append(int(old_msg[q]))
                flags.append(int(old_flags[q]))
        for j in range(int(wait_offsets[c]), int(wait_offsets[c + 1])):
            i = int(wait_perm[j])
            msg.append((id_base + i) & 0xFFFFFFFF if msg_id is None else int(msg_id[i]))
            fl = 0 if msg_flags is None else int(msg_flags[i])
            if same is not None and same[i]:
                fl |= MSG_CALL_CHAIN
            flags.append(fl)
        offsets.append(len(msg))
    total = len(msg)
    keep = total if cap is None else min(total, cap)
    return (np.array(offsets, np.uint32), np.array(msg[:keep], np.uint32), np.array(flags[:keep], np.uint8), total)


# ---- the per-message object form, from the C# ----------------------------------------------------

class Message:
    def __init__(self, mid, read_only=False, always_interleave=False, may_interleave=False, call_chain=False):
        self.id = mid
        self.read_only, self.always_interleave = bool(read_only), bool(always_interleave)
        self.may_interleave, self.call_chain = bool(may_interleave), bool(call_chain)


class Activation:
    """ActivationData + the Dispatcher methods that act on it under lock(activation)."""

    def __init__(self, valid=True, reentrant=False):
        self.valid, self.reentrant = valid, reentrant
        self.num_running = 0
        self.running = None
        self.waiting = []
        self.became_idle = False

    def record_running(self, m):                              # ActivationData.cs:475-493
        self.num_running += 1
        if self.running is not None:
            return
        self.running = m

    def reset_running(self, m):                               # ActivationData.cs:495-514
        self.num_running -= 1
        if self.num_running == 0:
            self.became_idle = True
        if self.running is not None and m is not self.running:
            return
        self.running = None

    def can_interleave(self, m):                              # Core/Dispatcher.cs:326-336, Catalog.cs:409-417
        return (m.always_interleave or self.running is None or (self.running.read_only and m.read_only) or
                m.call_chain or self.reentrant or m.may_interleave)

    def may_accept(self, m):                                  # Core/Dispatcher.cs:313-318
        if not self.valid:
            return False
        if not self.num_running > 0:
            return True
        return self.can_interleave(m)

    def receive_request(self, m):                             # Core/Dispatcher.cs:262-301, no limits, not stuck
        if self.may_accept(m):
            self.record_running(m)                            # HandleIncomingRequest
            return True
        self.waiting.append(m)                                # EnqueueMessage
        return False

    def run_message_pump(self):                               # Core/Dispatcher.cs:845-874
        started = []
        if not self.valid:
            return started
        while self.waiting:
            m = self.waiting[0]
            if not self.may_accept(m):
                break
            self.waiting.pop(0)
            self.record_running(m)
            started.append(m)
        return started

    def on_completed_request(self, m):                        # Core/Dispatcher.cs:822-843
        self.reset_running(m)
        return self.run_message_pump()


# ---- generators ---------------------------------------------------------------------------------

def wait_flags(rng, total, p_ro=0.5, p_other=0.08):
    return ((rng.random(total) < p_ro) * MSG_READ_ONLY | (rng.random(total) < p_other) * MSG_ALWAYS_INTERLEAVE |
            (rng.random(total) < p_other) * MSG_MAY_INTERLEAVE |
            (rng.random(total) < p_other) * MSG_CALL_CHAIN).astype(np.uint8)


def mixed_pump(rng, n_done, n_ctx, targets="uniform", mean_len=3.0, flags=True):
    """Every rule line in one batch once n_done and n_ctx are a few hundred: all three states, Running set and
    not, num_running 0 and above, lists of length 0 and up, completions outside the contexts."""
    ctx = zipf_targets(rng, n_done, n_ctx) if targets == "zipf" else rng.integers(0, n_ctx, n_done).astype(np.uint32)
    u = rng.random(n_done)
    ctx = np.where(u < 0.03, NONE32, np.where(u < 0.05, n_ctx, ctx)).astype(np.uint32)
    fl, nr = context_state(rng, n_ctx)
    nr = (nr + rng.integers(0, 3, n_ctx) * (rng.random(n_ctx) < 0.5)).astype(np.uint32)
    lens = rng.poisson(mean_len, n_ctx) * (rng.random(n_ctx) < 0.8)
    off = np.zeros(n_ctx + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    wf = wait_flags(rng, int(off[-1]))
    df = None
    if flags:
        df = ((rng.random(n_done) < 0.3) * DONE_IS_RUNNING | (rng.random(n_done) < 0.1) * DONE_PUMP_ONLY).astype(np.uint8)
    return PumpBatch(ctx, n_ctx, fl, nr, off, wf, df)
