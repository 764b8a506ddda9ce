"""The callback table restated literally: InsideRuntimeClient's `callbacks` dictionary as a Python
dict of id -> {handle, deadline, resend, silo}, one loop per gd_callbacks_* entry point with the C# line each
statement stands for, and the closed form of `respond` as numpy (respond_np), which test_callbacks_ref.py proves
equal to the loop.  File names: IRC = src/Orleans.Runtime/Core/InsideRuntimeClient.cs, CBD =
src/Orleans.Core/Runtime/CallbackData.cs, DSP = src/Orleans.Runtime/Core/Dispatcher.cs, MSG =
src/Orleans.Core/Messaging/Message.cs."""
import numpy as np

# outcomes / kinds (include/graindispatch.h GD_CB_*)
CB_NONE, CB_FIRE, CB_RESEND, CB_NO_CALLBACK, CB_GATEWAY_BACK, CB_TIMEOUT, CB_SILO_FAILED = range(7)
CB_INVALIDATE_CACHE = 1                       # out_flags bit
RESP_TARGET_NOT_ME, RESP_HAS_CACHE_HEADER = 1, 2
SUCCESS, ERROR, REJECTION = 0, 1, 2           # Message.ResponseTypes, MSG:89-94
TRANSIENT, OVERLOADED, DUPLICATE, UNRECOVERABLE, GATEWAY_TOO_BUSY = range(5)   # Message.RejectionTypes, MSG:96-103
NO_SILO = 0xFFFFFFFF
NO_HANDLE = 0xFFFFFFFF
TURN_RESPONSE = 8                             # GD_TURN_RESPONSE


class Options:
    """MessagingOptions.MaxResendCount / ResendOnTimeout, and CallbackData.StartTimer's repeat period (CBD:80-85)."""

    def __init__(self, max_resend_count=0, resend_on_timeout=False, period_ticks=0):
        self.max_resend_count = max_resend_count
        self.resend_on_timeout = resend_on_timeout
        self.period_ticks = period_ticks


class Table:
    def __init__(self, opt=None):
        self.opt = opt or Options()
        self.d = {}                           # id -> [handle, deadline, resend, silo]

    def may_resend(self, e):
        return e[2] < self.opt.max_resend_count            # Message.MayResend, MSG:346-349

    def resend(self, e):
        """Dispatcher.TryResendMessage (DSP:581-589): the count, and ResendMessageImpl clears the target (:618-620)."""
        e[2] += 1
        e[3] = NO_SILO

    # ---- gd_callbacks_add: SendRequestMessage's callbacks.TryAdd (IRC:205-218)
    def add(self, ids, handles, deadlines):
        out = np.zeros(len(ids), np.uint8)
        for i in range(len(ids)):
            k = int(ids[i])
            if k not in self.d:                                        # TryAdd: the first add of an id wins
                self.d[k] = [int(handles[i]), int(deadlines[i]), 0, NO_SILO]   # not addressed yet, ResendCount 0
                out[i] = 1
        return out

    # ---- gd_callbacks_set_target: Message.TargetSilo after the batch was addressed
    def set_target(self, ids, silo):
        out = np.zeros(len(ids), np.uint8)
        for i in range(len(ids)):
            e = self.d.get(int(ids[i]))
            if e is not None:
                e[3] = int(silo[i])                                    # batch order: the last one stands
                out[i] = 1
        return out

    # ---- gd_callbacks_lookup
    def lookup(self, ids):
        n = len(ids)
        h, r = np.full(n, NO_HANDLE, np.uint32), np.zeros(n, np.uint32)
        s, f = np.full(n, NO_SILO, np.uint32), np.zeros(n, np.uint8)
        for i in range(n):
            e = self.d.get(int(ids[i]))
            if e is not None:
                h[i], r[i], s[i], f[i] = e[0], e[2], e[3], 1
        return h, r, s, f

    # ---- gd_callbacks_respond: Dispatcher.ReceiveResponse -> InsideRuntimeClient.ReceiveResponse -> DoCallback
    def respond(self, ids, result=None, rejection=None, flags=None, turn=None):
        """(outcome u8, out_flags u8, handle u32, fire_idx u32) for a batch in arrival order."""
        n = len(ids)
        outcome, oflags = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        handle = np.full(n, NO_HANDLE, np.uint32)
        fire = []
        for i in range(n):
            if turn is not None and turn[i] != TURN_RESPONSE:          # not a response of gd_turns*
                continue
            res = SUCCESS if result is None else int(result[i])
            rej = int(rejection[i]) if (res == REJECTION and rejection is not None) else TRANSIENT
            fl = 0 if flags is None else int(flags[i])
            if res == REJECTION:                                       # IRC:571
                if fl & RESP_TARGET_NOT_ME:                            # IRC:573-579: gateway back, return
                    outcome[i] = CB_GATEWAY_BACK
                    continue
                if rej in (TRANSIENT, UNRECOVERABLE) and not (fl & RESP_HAS_CACHE_HEADER):   # IRC:590-600
                    oflags[i] |= CB_INVALIDATE_CACHE
            e = self.d.get(int(ids[i]))                                # IRC:610 callbacks.TryGetValue
            if e is None:
                outcome[i] = CB_NO_CALLBACK                            # IRC:622-626
                continue
            handle[i] = e[0]
            if res == REJECTION and rej == TRANSIENT and self.may_resend(e):   # CBD:135-141, DSP:581-589
                self.resend(e)
                outcome[i] = CB_RESEND
                continue
            outcome[i] = CB_FIRE                                       # CBD:143-149 alreadyFired, unregister
            del self.d[int(ids[i])]                                    # IRC:247-251 TryRemove
            fire.append(i)
        return outcome, oflags, handle, np.array(fire, np.uint32)

    # ---- the scans: (ids i64, handles u32, kinds u8), sorted by id (timers have no order)
    def _scan(self, pred, kind, touch_deadline):
        out = []
        for k in sorted(self.d):
            e = self.d[k]
            if not pred(e):
                continue
            if self.opt.resend_on_timeout and self.may_resend(e):      # CBD:186 OnFail: ResendOnTimeout && resendFunc
                self.resend(e)
                if touch_deadline:
                    e[1] += self.opt.period_ticks                      # the SafeTimer's repeat period, CBD:84,88
                out.append((k, e[0], CB_RESEND))
            else:
                out.append((k, e[0], kind))                            # CBD:192-199 alreadyFired, unregister
                del self.d[k]
        return (np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.uint32),
                np.array([o[2] for o in out], np.uint8))

    def expire(self, now):
        """gd_callbacks_expire: CallbackData.OnTimeout -> OnFail(isOnTimeout) (CBD:97-109,179-212); one tick a call."""
        return self._scan(lambda e: e[1] <= now, CB_TIMEOUT, True)

    def break_silo(self, silo):
        """gd_callbacks_break_silo: BreakOutstandingMessagesToDeadSilo (IRC:726-735) -> OnTargetSiloFail (CBD:111-124)."""
        return self._scan(lambda e: e[3] == silo, CB_SILO_FAILED, False)

    def count(self):
        return len(self.d)


def respond_np(table, ids, result=None, rejection=None, flags=None, turn=None):
    """The closed form of Table.respond, vectorised.  Ids do not interact, so only an id's own responses are
    ordered.  Among the responses of one id that reach the table (rules 3-5) and find it there at the batch start,
    with k = max(max_resend_count - resend_count, 0) resends left: let f = min(rank of the first one that is not a
    transient rejection, k).  Rank < f: RESEND; rank == f: FIRE; rank > f: NO_CALLBACK.  Updates `table` too."""
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    res = np.zeros(n, np.int64) if result is None else np.asarray(result, np.int64)
    rej = np.zeros(n, np.int64) if rejection is None else np.asarray(rejection, np.int64)
    fl = np.zeros(n, np.int64) if flags is None else np.asarray(flags, np.int64)
    part = np.ones(n, bool) if turn is None else np.asarray(turn) == TURN_RESPONSE
    is_rej = res == REJECTION
    gateway = part & is_rej & ((fl & RESP_TARGET_NOT_ME) != 0)
    inval = part & is_rej & ~gateway & np.isin(rej, (TRANSIENT, UNRECOVERABLE)) & ((fl & RESP_HAS_CACHE_HEADER) == 0)
    touch = part & ~gateway
    transient = is_rej & (rej == TRANSIENT)
    present = np.array([int(k) in table.d for k in ids], bool) if n else np.zeros(0, bool)
    outcome = np.zeros(n, np.uint8)
    outcome[gateway] = CB_GATEWAY_BACK
    outcome[touch & ~present] = CB_NO_CALLBACK
    oflags = inval.astype(np.uint8) * np.uint8(CB_INVALIDATE_CACHE)
    handle = np.full(n, NO_HANDLE, np.uint32)
    live = np.flatnonzero(touch & present)
    # rank of each table-touching response among its id's, in arrival order
    order = live[np.argsort(ids[live], kind="stable")]
    sid = ids[order]
    start = np.r_[True, sid[1:] != sid[:-1]] if len(order) else np.zeros(0, bool)
    grp = np.cumsum(start) - 1
    first = np.flatnonzero(start)
    rank = np.arange(len(order)) - first[grp] if len(order) else np.zeros(0, np.int64)
    # the first non-transient rank of each group (the group's size when there is none)
    size = np.diff(np.r_[first, len(order)])
    nt_rank = np.where(~transient[order], rank, np.iinfo(np.int64).max)
    first_nt = np.minimum.reduceat(nt_rank, first) if len(order) else np.zeros(0, np.int64)
    first_nt = np.minimum(first_nt, size)
    r0 = np.array([table.d[int(k)][2] for k in sid[start]], np.int64) if len(order) else np.zeros(0, np.int64)
    h0 = np.array([table.d[int(k)][0] for k in sid[start]], np.uint32) if len(order) else np.zeros(0, np.uint32)
    k_left = np.maximum(table.opt.max_resend_count - r0, 0)
    f = np.minimum(first_nt, k_left)
    if len(order):
        fr = f[grp]
        outcome[order] = np.where(rank < fr, CB_RESEND, np.where(rank == fr, CB_FIRE, CB_NO_CALLBACK)).astype(np.uint8)
        handle[order] = np.where(rank <= fr, h0[grp], np.uint32(NO_HANDLE))
    # the table afterwards: a fired entry leaves; the others took min(f, size) resends
    for g, k in enumerate(sid[start]):
        if f[g] < size[g]:
            del table.d[int(k)]
        elif size[g]:
            e = table.d[int(k)]
            e[2] += int(size[g])
            e[3] = NO_SILO
    fire = np.flatnonzero(outcome == CB_FIRE).astype(np.uint32)
    return outcome, oflags, handle, fire


def mixed_batch(rng, table, n, n_absent_pool=64, max_rep=5):
    """A respond batch mixing present and absent ids, every result / rejection / flag combination and ids repeated
    2 .. max_rep times, shuffled."""
    present = np.array(sorted(table.d), np.int64)
    absent = np.arange(1, n_absent_pool + 1, dtype=np.int64) * -7919
    pool = np.r_[present, absent] if len(present) else absent
    ids = []
    while len(ids) < n:
        k = int(pool[rng.integers(len(pool))])
        ids += [k] * (int(rng.integers(2, max_rep + 1)) if rng.random() < 0.3 else 1)
    ids = np.array(ids[:n], np.int64)
    rng.shuffle(ids)
    result = rng.choice(np.array([SUCCESS, ERROR, REJECTION], np.uint8), n, p=[0.4, 0.1, 0.5])
    rejection = rng.choice(np.array([TRANSIENT, OVERLOADED, DUPLICATE, UNRECOVERABLE, GATEWAY_TOO_BUSY], np.uint8), n,
                           p=[0.6, 0.1, 0.1, 0.1, 0.1])
    flags = rng.choice(np.array([0, 1, 2, 3], np.uint8), n, p=[0.7, 0.1, 0.15, 0.05])
    return ids, result, rejection, flags
