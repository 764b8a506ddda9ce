"""The activation collector restated three times, for tests/test_collect_ref.py (CPU) and
tests/test_gpu_collect.py:

(a) Collector / Act: a lock-free transcription of src/Orleans.Runtime/Catalog/ActivationCollector.cs with a real
    dict[ticket] -> Bucket(dict[ctx]) and the per-activation fields of Catalog/ActivationData.cs, cited line by
    line.  Exceptions are caught into the status codes of include/graindispatch.h.  A bucket is enumerated in
    ascending context index (the reference's order is a ConcurrentDictionary's: unspecified, so ours).
(b) Arrays: the gd_collect_* entry points' rules over numpy arrays -- what the GPU must give bit for bit.
(c) generators of states and batches for the GPU tests; test_collect_ref.py asserts what they cover.
"""
import numpy as np

import _turns_ref as R

EXEMPT, CANCELLED = 1, 2
(SCHEDULED, OUT_OF_RANGE, SKIPPED_EXEMPT, SKIPPED_NO_LIMIT, THROWS_TIMEOUT, THROWS_EARLY, THROWS_TICKETED) = range(7)
FALSE, TRUE, THROWS, NO_PART = range(4)
BAD_STATE, KEPT_ALIVE, ACTIVE, NOT_STALE, COLLECT = range(1, 6)
NOT_ADDED = 0x80
IDLE = 1                                                     # GD_PUMP_BECAME_IDLE
VALID, NOT_READY, INVALID, STATE_MASK = R.CTX_VALID, R.CTX_NOT_READY, R.CTX_INVALID, R.CTX_STATE_MASK
TURN_TAKES_PART = (R.TURN_START, R.TURN_WAIT, R.TURN_REJECT_OVERLOADED, R.TURN_STUCK, R.TURN_FORWARD,
                   R.TURN_REJECT_TRANSIENT)
MAX_QUANTA = 1 << 28


def tdiv(a, b):
    """C#'s integer division (truncating)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def roundup(t, q):                                           # :371
    return (tdiv(t - 1, q) + 1) * q


# ---- (a) the literal transcription ----------------------------------------------------------------------

class Throw(Exception):
    def __init__(self, code):
        self.code = code


class Act:
    """ActivationData's fields the collector reads and writes."""

    def __init__(self, idx, age_limit, exempt=False, state=VALID):
        self.idx, self.age_limit, self.exempt, self.state = idx, age_limit, exempt, state
        self.ticket = 0                                      # CollectionTicket = default(DateTime), :414
        self.cancelled = False                               # collectionCancelledFlag, :415
        self.became_idle = 0                                 # :472
        self.keep_alive_until = 0                            # DateTime.MinValue, :724,748
        self.num_running, self.n_waiting = 0, 0
        self.other_bits = 0                                  # the ctx_flags bits above the state

    def try_set_cancelled(self):                             # ActivationData.cs:417-425
        if self.ticket == 0 or self.cancelled:
            return False
        self.cancelled = True
        return True

    def set_ticket(self, t):                                 # :440-449
        assert t != 0 and self.ticket == 0
        self.ticket = t

    def is_inactive(self):                                   # :689-703
        return not self.num_running > 0 and self.n_waiting == 0

    def ctx_flag_byte(self):
        return self.state | self.other_bits


class Bucket:                                                # ActivationCollector.cs:411-470
    def __init__(self, key, quantum):
        if key == 0 or key % quantum != 0:                   # :421, :341-348
            raise Throw(THROWS)
        self.key, self.items = key, {}

    def add(self, a):                                        # :426-432
        assert a.idx not in self.items
        self.items[a.idx] = a

    def try_remove(self, a):                                 # :434-439
        if not a.try_set_cancelled():
            return False
        return self.items.pop(a.idx, None) is not None

    def cancel_all(self):                                    # :441-459, in ascending context index
        return [a for _, a in sorted(self.items.items()) if a.try_set_cancelled()]


class Collector:
    def __init__(self, quantum, now):                        # :26-40
        assert quantum != 0
        self.quantum, self.buckets = quantum, {}
        self.next_ticket = 0
        self.next_ticket = self.ticket_from_datetime(now)    # :37

    def ticket_from_datetime(self, t):                       # :368-377
        ticket = roundup(t, self.quantum)
        if ticket < self.next_ticket:
            raise Throw(THROWS_EARLY)
        return ticket

    def ticket_from_timespan(self, timeout, now):            # :379-387
        if timeout < self.quantum:
            raise Throw(THROWS_TIMEOUT)
        return self.ticket_from_datetime(now + timeout)

    def is_expired(self, ticket):                            # :363-366
        return ticket < self.next_ticket

    def add(self, a, ticket):                                # :389-401
        a.cancelled = False
        b = self.buckets.get(ticket)
        if b is None:
            b = self.buckets[ticket] = Bucket(ticket, self.quantum)
        b.add(a)
        a.set_ticket(ticket)

    def schedule(self, a, now):                              # :83-108; raises Throw
        if a.exempt:
            return SKIPPED_EXEMPT
        if a.age_limit == 0:
            return SKIPPED_NO_LIMIT
        ticket = self.ticket_from_timespan(a.age_limit, now)
        if a.ticket != 0:
            raise Throw(THROWS_TICKETED)
        self.add(a, ticket)
        return SCHEDULED

    def try_cancel(self, a):                                 # :110-126
        if a.exempt:
            return False
        if a.ticket == 0 or self.is_expired(a.ticket):
            return False
        b = self.buckets.get(a.ticket)
        return b is not None and b.try_remove(a)

    def try_reschedule(self, a, now):                        # :128-139; raises Throw
        if a.exempt:
            return False
        if self._reschedule_impl(a, a.age_limit, now):
            return True
        a.ticket = 0
        return False

    def _reschedule_impl(self, a, timeout, now):             # :141-164
        if a.ticket == 0:
            return False
        if a.ticket % self.quantum != 0:                     # ThrowIfTicketIsInvalid, :145
            raise Throw(THROWS)
        if self.is_expired(a.ticket):
            return False
        old = a.ticket
        try:
            new = self.ticket_from_timespan(timeout, now)
        except Throw:
            raise Throw(THROWS)
        if new == old:
            return True
        b = self.buckets.get(old)
        if b is None or not b.try_remove(a):
            return False
        a.ticket = 0
        self.add(a, new)
        return True

    def dequeue_quantum(self, now):                          # :166-190; None = false
        if self.next_ticket > now:
            return None
        key = self.next_ticket
        self.next_ticket += self.quantum
        b = self.buckets.pop(key, None)
        return [] if b is None else b.cancel_all()

    def scan_stale(self, now):                               # :206-264 -> (condemned, {ctx: verdict})
        result, verdict = [], {}
        while True:
            acts = self.dequeue_quantum(now)
            if acts is None:
                break
            for a in acts:
                a.ticket = 0                                 # :218
                if a.state != VALID:
                    v, again = BAD_STATE, False
                elif a.keep_alive_until >= now:              # ShouldBeKeptAlive, ActivationData.cs:726
                    v, again = KEPT_ALIVE, True
                elif not a.is_inactive():
                    v, again = ACTIVE, True
                elif not now - a.became_idle >= a.age_limit:  # IsStale, :719-722
                    v, again = NOT_STALE, True
                else:
                    v, again = COLLECT, False
                    a.state = NOT_READY                      # PrepareForDeactivation, :395-400
                    result.append(a.idx)
                if again:
                    try:
                        if self.schedule(a, now) != SCHEDULED:
                            v |= NOT_ADDED
                    except Throw:
                        v |= NOT_ADDED
                verdict[a.idx] = v
        return result, verdict

    def scan_all(self, age_limit, now):                      # :271-325 -> (condemned by context, {ctx: verdict})
        result, verdict = [], {}
        for b in list(self.buckets.values()):
            for _, a in sorted(b.items.items()):
                if a.state != VALID:
                    v = BAD_STATE
                elif a.keep_alive_until >= now:
                    v = KEPT_ALIVE
                elif not a.is_inactive():
                    v = ACTIVE
                elif now - a.became_idle >= age_limit:       # GetIdleness, :304
                    v = COLLECT
                    if b.try_remove(a):                      # :306
                        a.state = NOT_READY
                        result.append(a.idx)
                else:
                    v = NOT_STALE
                verdict[a.idx] = v
        return sorted(result), verdict                       # across buckets the reference's order is unspecified

    def num_recently_used(self, shortest_age_limit, recency, now):   # :58-81
        if shortest_age_limit == 0:
            return sum(len(b.items) for b in self.buckets.values())
        return sum(len(b.items) for b in self.buckets.values() if shortest_age_limit - (b.key - now) <= recency)

    def members(self):
        """{ctx: bucket key} of everything in a bucket."""
        return {c: b.key for b in self.buckets.values() for c in b.items}


def literal_call(f, *args):
    """An answer of (a) as the entry points code it: the exception's code, else the value."""
    try:
        return f(*args)
    except Throw as e:
        return e.code


# ---- (b) the array form ---------------------------------------------------------------------------------

def _roundup_v(x, q):
    d = np.where(x - 1 >= 0, (x - 1) // q, -((-(x - 1)) // q))
    return (d + 1) * q


class Arrays:
    """gd_collect_state and the handle's two words; each method is one entry point."""

    def __init__(self, quantum, now, ticket, became_idle, keep_alive_until, age_limit, flags):
        assert quantum > 0
        self.quantum, self.next = quantum, roundup(now, quantum)
        self.ticket, self.became_idle = np.array(ticket, np.int64), np.array(became_idle, np.int64)
        self.keep_alive_until = None if keep_alive_until is None else np.array(keep_alive_until, np.int64)
        self.age_limit, self.flags = np.array(age_limit, np.int64), np.array(flags, np.uint8)
        self.n_ctx = len(self.ticket)

    def copy(self):
        c = Arrays.__new__(Arrays)
        c.__dict__.update(self.__dict__)
        for k in ("ticket", "became_idle", "keep_alive_until", "age_limit", "flags"):
            if getattr(self, k) is not None:
                setattr(c, k, getattr(self, k).copy())
        return c

    def state(self):
        return self.ticket, self.became_idle, self.flags

    def in_bucket(self):
        """The invariant that replaces the dictionaries."""
        return (self.ticket != 0) & ((self.flags & CANCELLED) == 0) & (self.ticket >= self.next)

    def _schedule_rule(self, cs, now):
        """ScheduleCollection on distinct contexts cs."""
        q, fl, age, t = self.quantum, self.flags[cs], self.age_limit[cs], self.ticket[cs]
        new = _roundup_v(now + age, q)
        st = np.select([(fl & EXEMPT) != 0, age == 0, age < q, new < self.next, t != 0],
                       [SKIPPED_EXEMPT, SKIPPED_NO_LIMIT, THROWS_TIMEOUT, THROWS_EARLY, THROWS_TICKETED],
                       SCHEDULED).astype(np.uint8)
        ok = st == SCHEDULED
        self.ticket[cs[ok]] = new[ok]
        self.flags[cs[ok]] &= np.uint8(~CANCELLED & 0xFF)
        return st

    def _reschedule_rule(self, cs, now):
        """TryRescheduleCollection on distinct contexts cs."""
        q, fl, age, t = self.quantum, self.flags[cs], self.age_limit[cs], self.ticket[cs]
        new = _roundup_v(now + age, q)
        k = np.select([(fl & EXEMPT) != 0, t == 0, t % q != 0, t < self.next, age < q, new < self.next, new == t,
                       (fl & CANCELLED) != 0], list(range(8)), 8)
        self.ticket[cs[(k == 3) | (k == 7)]] = 0
        self.ticket[cs[k == 8]] = new[k == 8]
        return np.array([FALSE, FALSE, THROWS, FALSE, THROWS, THROWS, TRUE, FALSE, TRUE], np.uint8)[k]

    @staticmethod
    def _first(c):
        """The distinct values of c, each one's index into them, and which entries are first occurrences."""
        uniq, first, inv = np.unique(c, return_index=True, return_inverse=True)
        is_first = np.zeros(len(c), bool)
        is_first[first] = True
        return uniq, inv.reshape(-1), is_first

    def schedule(self, ctx, now):
        ctx = np.asarray(ctx, np.uint32)
        status = np.full(len(ctx), OUT_OF_RANGE, np.uint8)
        i = np.flatnonzero(ctx < self.n_ctx)
        uniq, inv, is_first = self._first(ctx[i].astype(np.int64))
        s = self._schedule_rule(uniq, now)[inv]
        status[i] = np.where(~is_first & (s == SCHEDULED), THROWS_TICKETED, s)
        return status

    def cancel(self, ctx):
        ctx = np.asarray(ctx, np.uint32)
        out = np.zeros(len(ctx), np.uint8)
        i = np.flatnonzero(ctx < self.n_ctx)
        uniq, inv, is_first = self._first(ctx[i].astype(np.int64))
        fl, t = self.flags[uniq], self.ticket[uniq]
        r = ((fl & EXEMPT) == 0) & (t != 0) & (t >= self.next) & ((fl & CANCELLED) == 0)
        self.flags[uniq[r]] |= np.uint8(CANCELLED)
        out[i] = r[inv] & is_first
        return out

    def touch(self, ctx_flags, ctx, now, turn=None):
        ctx, ctx_flags = np.asarray(ctx, np.uint32), np.asarray(ctx_flags, np.uint8)
        ok = np.full(len(ctx), NO_PART, np.uint8)
        part = ctx < self.n_ctx
        if turn is not None:
            part &= np.isin(np.asarray(turn, np.uint8), TURN_TAKES_PART)
        part[part] = (ctx_flags[ctx[part]] & STATE_MASK) == VALID
        i = np.flatnonzero(part)
        uniq, inv, _ = self._first(ctx[i].astype(np.int64))
        ok[i] = self._reschedule_rule(uniq, now)[inv]
        return ok

    def idle(self, event, now):
        event = np.asarray(event, np.uint8)
        ok = np.full(self.n_ctx, NO_PART, np.uint8)
        cs = np.flatnonzero(event & IDLE)
        self.became_idle[cs] = now
        ok[cs] = self._reschedule_rule(cs, now)
        return ok

    def _chain(self, d, ctx_flags, num_running, wait_offsets, now, age):
        cf = ctx_flags[d]
        ka = np.zeros(len(d), bool) if self.keep_alive_until is None else self.keep_alive_until[d] >= now
        active = np.asarray(num_running, np.uint32)[d].view(np.int32) > 0
        if wait_offsets is not None:
            wo = np.asarray(wait_offsets, np.uint32)
            active |= wo[d + 1] != wo[d]
        return np.select([(cf & STATE_MASK) != VALID, ka, active, now - self.became_idle[d] < age],
                         [BAD_STATE, KEPT_ALIVE, ACTIVE, NOT_STALE], COLLECT).astype(np.uint8)

    def quanta(self, now):
        return 0 if self.next > now else (now - self.next) // self.quantum + 1

    def scan_stale(self, ctx_flags, num_running, now, wait_offsets=None):
        """ctx_flags (uint8 array) is updated in place.  -> (condemned u32, verdict u8[n_ctx]); ValueError =
        GD_EINVAL with nothing changed."""
        q, next0 = self.quantum, self.next
        n_q = self.quanta(now)
        if n_q > MAX_QUANTA:
            raise ValueError("more than 2^28 quanta")
        due = self.in_bucket() & (self.ticket <= now) & ((self.ticket - next0) % q == 0)
        d = np.flatnonzero(due)
        old = self.ticket[d].copy()
        self.flags[d] |= np.uint8(CANCELLED)
        self.ticket[d] = 0
        self.next = next0 + n_q * q
        v = self._chain(d, ctx_flags, num_running, wait_offsets, now, self.age_limit[d])
        again = (v >= KEPT_ALIVE) & (v <= NOT_STALE)
        v[again] |= np.where(self._schedule_rule(d[again], now) != SCHEDULED, NOT_ADDED, 0).astype(np.uint8)
        col = v == COLLECT
        ctx_flags[d[col]] = (ctx_flags[d[col]] & np.uint8(~STATE_MASK & 0xFF)) | np.uint8(NOT_READY)
        verdict = np.zeros(self.n_ctx, np.uint8)
        verdict[d] = v
        order = np.lexsort((d[col], old[col]))
        return d[col][order].astype(np.uint32), verdict

    def scan_all(self, ctx_flags, num_running, now, age_limit_ticks, wait_offsets=None):
        d = np.flatnonzero(self.in_bucket())
        v = self._chain(d, ctx_flags, num_running, wait_offsets, now, age_limit_ticks)
        col = d[v == COLLECT]
        self.flags[col] |= np.uint8(CANCELLED)
        ctx_flags[col] = (ctx_flags[col] & np.uint8(~STATE_MASK & 0xFF)) | np.uint8(NOT_READY)
        verdict = np.zeros(self.n_ctx, np.uint8)
        verdict[d] = v
        return col.astype(np.uint32), verdict

    def count_recent(self, now, shortest_age_limit, recency):
        m = self.in_bucket()
        if shortest_age_limit != 0:
            m &= shortest_age_limit - (self.ticket - now) <= recency
        return int(m.sum())


# ---- (c) generators -------------------------------------------------------------------------------------

Q = 600_000_000                                              # one minute in ticks
T0 = 636_000_000_000_000_000                                 # a DateTime in 2016
AGES = np.array([0, Q // 2, Q, 2 * Q, 5 * Q, 3 * Q + 7], np.int64)


def targets(rng, n, n_ctx, kind="uniform", p_out=0.02):
    """n context indices, uniform or Zipf(1.1), a few of them >= n_ctx."""
    if kind == "zipf":
        c = (rng.zipf(1.1, n) - 1) % n_ctx
    else:
        c = rng.integers(0, n_ctx, n)
    c = c.astype(np.uint32)
    out = rng.random(n) < p_out
    c[out] = n_ctx + rng.integers(0, 5, int(out.sum())).astype(np.uint32)
    if n:
        c[rng.integers(0, n)] = 0xFFFFFFFF if n > 3 else c[0]
    return c


class World:
    """A collector state of n_ctx contexts with every kind of context in it, and the host's arrays beside it:
    ctx_flags, num_running, wait_offsets.  n_q: the quanta a scan_stale at self.now dequeues."""

    def __init__(self, rng, n_ctx, n_q=1, due="mixed", keep_alive=True):
        now = T0 + 12345
        nxt = roundup(now, Q) - n_q * Q if n_q else roundup(now, Q) + Q
        self.now, self.n_ctx, self.n_q = now, n_ctx, n_q
        configured_at = nxt - 5                              # roundup(configured_at) == nxt
        span = max(n_q, 1)
        k = rng.integers(0, span, n_ctx)
        due_t = nxt + k * Q if n_q else np.zeros(n_ctx, np.int64)
        kind = rng.choice(6, n_ctx, p=[0.2, 0.45, 0.2, 0.05, 0.05, 0.05])
        if due == "all":
            kind[:] = 1
        elif due == "none":
            kind[kind == 1] = 2
            kind[kind == 5] = 0
        elif due != "mixed":                                 # a list of the only due contexts
            kind[kind == 1] = 2
            kind[kind == 5] = 0
            kind[np.asarray(due, np.int64)] = 1
        future = nxt + (span + rng.integers(0, 4, n_ctx)) * Q
        ticket = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                           [0, due_t if n_q else future, future, nxt - (1 + rng.integers(0, 3, n_ctx)) * Q,
                            (due_t if n_q else future) + 1], due_t if n_q else future).astype(np.int64)
        flags = np.where(rng.random(n_ctx) < 0.05, EXEMPT, 0).astype(np.uint8)
        flags |= np.where((kind == 5) | (rng.random(n_ctx) < 0.05), CANCELLED, 0).astype(np.uint8)
        age = AGES[rng.choice(len(AGES), n_ctx, p=[0.05, 0.05, 0.3, 0.3, 0.2, 0.1])]
        idle = now - np.array([0, Q, 3 * Q, 10 * Q], np.int64)[rng.integers(0, 4, n_ctx)]
        ka = np.array([0, now - 1, now, now + 5 * Q], np.int64)[rng.choice(4, n_ctx, p=[0.6, 0.2, 0.1, 0.1])]
        state = rng.choice([VALID, NOT_READY, INVALID], n_ctx, p=[0.8, 0.1, 0.1]).astype(np.uint8)
        if not isinstance(due, str) or due != "mixed":
            state[:], flags[:] = VALID, flags & ~np.uint8(EXEMPT)
        if not isinstance(due, str):
            flags[np.asarray(due, np.int64)] = 0
        self.ctx_flags = state | (rng.integers(0, 32, n_ctx).astype(np.uint8) << 2)
        self.num_running = rng.choice(np.array([0, 1, 3, 0xFFFFFFFF], np.uint32), n_ctx, p=[0.8, 0.1, 0.05, 0.05])
        lens = np.where(rng.random(n_ctx) < 0.1, rng.integers(1, 4, n_ctx), 0)
        self.wait_offsets = np.zeros(n_ctx + 1, np.uint32)
        self.wait_offsets[1:] = np.cumsum(lens)
        if due == "all":                                     # every context condemned
            age[:], idle[:], ka[:], flags[:] = Q, now - 10 * Q, 0, 0
            self.num_running[:], self.wait_offsets[:] = 0, 0
        self.arrays = Arrays(Q, configured_at, ticket, idle, ka if keep_alive else None, age, flags)
        assert self.arrays.next == nxt and self.arrays.quanta(now) == n_q
