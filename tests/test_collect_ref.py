"""CPU: the array form of the activation collector (_collect_ref.Arrays, what the GPU is held to) against the
literal transcription of ActivationCollector.cs with real dictionaries (_collect_ref.Collector) -- every output and
the whole state after every step of seeded random lifecycles, the bucket-membership invariant after every step, the
idempotence that lets gd_collect_touch run without an election, and what the GPU tests' generators cover."""
import numpy as np
import pytest

import _collect_ref as K
import _turns_ref as R

Q = K.Q


class Both:
    """One collector twice: Act objects under a Collector, and Arrays; each op runs on both and is compared."""

    def __init__(self, seed, n_ctx=40):
        self.rng = rng = np.random.default_rng(seed)
        self.n_ctx, self.now = n_ctx, K.T0 + int(rng.integers(0, 5 * Q))
        age = K.AGES[rng.choice(len(K.AGES), n_ctx, p=[0.08, 0.08, 0.34, 0.3, 0.1, 0.1])]
        exempt = rng.random(n_ctx) < 0.1
        self.acts = [K.Act(c, int(age[c]), bool(exempt[c])) for c in range(n_ctx)]
        self.lit = K.Collector(Q, self.now)
        self.arr = K.Arrays(Q, self.now, np.zeros(n_ctx), np.zeros(n_ctx), np.zeros(n_ctx), age,
                            np.where(exempt, K.EXEMPT, 0))
        self.seen = {k: set() for k in ("schedule", "cancel", "touch", "idle", "verdict", "jump", "early")}
        self.condemned = 0
        self.compare()

    # -- the host's arrays, from the objects
    def ctx_flags(self):
        return np.array([a.ctx_flag_byte() for a in self.acts], np.uint8)

    def num_running(self):
        return np.array([a.num_running & 0xFFFFFFFF for a in self.acts], np.uint32)

    def wait_offsets(self):
        return np.concatenate([[0], np.cumsum([a.n_waiting for a in self.acts])]).astype(np.uint32)

    def compare(self):
        a = self.arr
        assert a.next == self.lit.next_ticket
        assert a.ticket.tolist() == [x.ticket for x in self.acts]
        assert a.became_idle.tolist() == [x.became_idle for x in self.acts]
        assert [bool(f & K.CANCELLED) for f in a.flags] == [x.cancelled for x in self.acts]
        assert [bool(f & K.EXEMPT) for f in a.flags] == [x.exempt for x in self.acts]
        # the invariant that replaces the dictionaries
        members = self.lit.members()
        assert sorted(members) == np.flatnonzero(a.in_bucket()).tolist()
        assert all(a.ticket[c] == key for c, key in members.items())

    def ctx_list(self, n):
        return K.targets(self.rng, n, self.n_ctx, "zipf" if self.rng.random() < 0.5 else "uniform", 0.05)

    def stamp(self):
        """The call's `now`: the clock, or now and then a batch stamped long before (the :372 throw needs one)."""
        return self.now - 50 * Q if self.rng.random() < 0.1 else self.now

    def op_schedule(self):
        ctx, now = self.ctx_list(int(self.rng.integers(0, 30))), self.stamp()
        want = [K.OUT_OF_RANGE if c >= self.n_ctx else K.literal_call(self.lit.schedule, self.acts[c], now)
                for c in ctx.tolist()]
        got = self.arr.schedule(ctx, now)
        assert got.dtype == np.uint8 and got.tolist() == want
        self.seen["schedule"] |= set(want)

    def op_cancel(self):
        ctx = self.ctx_list(int(self.rng.integers(0, 30)))
        want = [int(c < self.n_ctx and self.lit.try_cancel(self.acts[c])) for c in ctx.tolist()]
        assert self.arr.cancel(ctx).tolist() == want
        self.seen["cancel"] |= set(want)

    def literal_touch(self, ctx, turn, now=None):
        now = self.now if now is None else now
        out = []
        for i, c in enumerate(ctx.tolist()):
            part = c < self.n_ctx and (turn is None or int(turn[i]) in K.TURN_TAKES_PART) and \
                self.acts[c].state == K.VALID                # Dispatcher.cs:114-119
            out.append(int(K.literal_call(self.lit.try_reschedule, self.acts[c], now)) if part else K.NO_PART)
        return out

    def op_touch(self):
        ctx = self.ctx_list(int(self.rng.integers(0, 60)))
        turn = None if self.rng.random() < 0.3 else self.rng.integers(0, 10, len(ctx)).astype(np.uint8)
        cf, now = self.ctx_flags(), self.stamp()
        want = self.literal_touch(ctx, turn, now)
        assert self.arr.touch(cf, ctx, now, turn).tolist() == want
        self.seen["touch"] |= set(want)
        # every occurrence of a context got its first's answer, by the literal loop
        first = {}
        for c, w in zip(ctx.tolist(), want):
            if w != K.NO_PART:
                assert first.setdefault(c, w) == w

    def op_idle(self):
        ev = (self.rng.random(self.n_ctx) < 0.3).astype(np.uint8) * K.IDLE | \
            (self.rng.integers(0, 4, self.n_ctx).astype(np.uint8) << 1)
        want = []
        for a, e in zip(self.acts, ev):
            if e & K.IDLE:                                   # ActivationData.cs:500-507
                a.num_running = 0
                a.became_idle = self.now
                want.append(K.FALSE if a.exempt else int(K.literal_call(self.lit.try_reschedule, a, self.now)))
            else:
                want.append(K.NO_PART)
        assert self.arr.idle(ev, self.now).tolist() == want
        self.seen["idle"] |= set(want)

    def _scan(self, lit_scan, arr_scan):
        cf, nr, wo = self.ctx_flags(), self.num_running(), self.wait_offsets()
        want_list, want_v = lit_scan()
        got_list, got_v = arr_scan(cf, nr, wo)
        assert got_list.dtype == np.uint32 and got_list.tolist() == want_list
        assert got_v.tolist() == [want_v.get(c, 0) for c in range(self.n_ctx)]
        assert cf.tolist() == [a.ctx_flag_byte() for a in self.acts]
        self.seen["verdict"] |= set(want_v.values())
        self.condemned += len(want_list)

    def op_scan_stale(self):
        self.seen["jump"].add(min(self.arr.quanta(self.now), 3))
        self._scan(lambda: self.lit.scan_stale(self.now),
                   lambda cf, nr, wo: self.arr.scan_stale(cf, nr, self.now, wo))

    def op_scan_all(self):
        limit = int(self.rng.choice([0, Q, 3 * Q, 50 * Q]))
        self._scan(lambda: self.lit.scan_all(limit, self.now),
                   lambda cf, nr, wo: self.arr.scan_all(cf, nr, self.now, limit, wo))

    def op_count(self):
        for shortest, rec in ((0, 0), (Q, 0), (Q, 2 * Q), (2 * Q, 10 * Q)):
            assert self.arr.count_recent(self.now, shortest, rec) == self.lit.num_recently_used(shortest, rec, self.now)

    def op_host(self):
        """What the host writes between calls: turns start, lists grow, DelayDeactivation, states, age limits."""
        rng = self.rng
        for c in rng.integers(0, self.n_ctx, 6).tolist():
            a, what = self.acts[c], int(rng.integers(0, 8))
            if what == 0:
                a.num_running = int(rng.choice([0, 1, 2, -1]))
            elif what == 1:
                a.n_waiting = int(rng.integers(0, 3))
            elif what == 2:
                a.keep_alive_until = int(rng.choice([0, self.now, self.now + 3 * Q]))
                self.arr.keep_alive_until[c] = a.keep_alive_until
            elif what == 3:
                a.state = int(rng.choice([K.VALID, K.VALID, K.NOT_READY, K.INVALID]))
            elif what == 4:
                a.other_bits = int(rng.integers(0, 32)) << 2
            elif what == 5:
                a.age_limit = int(K.AGES[rng.integers(0, len(K.AGES))])
                self.arr.age_limit[c] = a.age_limit
            elif what == 7:                                  # collector == null is the host's to say
                a.exempt = not a.exempt
                self.arr.flags[c] ^= np.uint8(K.EXEMPT)
            else:
                a.became_idle = self.now - int(rng.choice([0, Q, 20 * Q]))
                self.arr.became_idle[c] = a.became_idle

    def op_clock(self):
        jump = int(self.rng.choice([0, 0, 1, Q // 3, Q, 2 * Q, 1000 * Q], p=[0.2, 0.1, 0.1, 0.2, 0.2, 0.15, 0.05]))
        self.now += jump
        if self.now < self.arr.next:
            self.seen["early"].add(True)

    def step(self):
        ops = [self.op_schedule, self.op_cancel, self.op_touch, self.op_idle, self.op_scan_stale, self.op_scan_all,
               self.op_count, self.op_host, self.op_clock]
        self.rng.choice(ops, p=[0.2, 0.08, 0.17, 0.1, 0.1, 0.04, 0.05, 0.1, 0.16])()
        self.compare()


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_array_form_equals_the_literal_collector(seed):
    w = Both(seed)
    for _ in range(400):
        w.step()
    assert w.seen["jump"] >= {0, 1, 2, 3} and w.seen["early"]            # 0, 1, 2 and 1000 quanta; now < nextTicket
    assert w.condemned > 0


def test_lifecycles_reach_every_answer():
    seen = {}
    for seed in range(1, 9):
        w = Both(seed)
        for _ in range(400):
            w.step()
        for k, v in w.seen.items():
            seen.setdefault(k, set()).update(v)
    assert seen["schedule"] == set(range(7))
    assert seen["cancel"] == {0, 1}
    assert seen["touch"] >= {K.FALSE, K.TRUE, K.THROWS, K.NO_PART} and seen["idle"] >= {K.FALSE, K.TRUE, K.NO_PART}
    assert {v & 0x7F for v in seen["verdict"]} == {K.BAD_STATE, K.KEPT_ALIVE, K.ACTIVE, K.NOT_STALE, K.COLLECT}
    assert any(v & K.NOT_ADDED for v in seen["verdict"])


def test_touch_is_idempotent_at_one_now():
    """Entry 3's claim: the literal loop over a list with duplicates gives every occurrence the first's answer, for
    every kind of context a lifecycle reaches -- so the kernel needs no election."""
    for seed in (5, 6, 7):
        w = Both(seed, 25)
        for _ in range(150):
            w.step()
            ctx = np.repeat(np.arange(w.n_ctx, dtype=np.uint32), 3)
            w.rng.shuffle(ctx)
            want = w.literal_touch(ctx, None)
            assert w.arr.touch(w.ctx_flags(), ctx, w.now).tolist() == want
            first = {}
            for c, r in zip(ctx.tolist(), want):
                assert first.setdefault(c, r) == r
            w.compare()


def test_rounding_and_the_early_throw():
    assert [K.roundup(t, 10) for t in (1, 9, 10, 11, 20)] == [10, 10, 10, 20, 20]
    c = K.Collector(10, 95)
    assert c.next_ticket == 100
    a = K.Act(0, 10)
    assert K.literal_call(c.schedule, a, 50) == K.THROWS_EARLY and K.literal_call(c.schedule, a, 95) == K.SCHEDULED
    assert a.ticket == 110 and c.members() == {0: 110}
    b = K.Arrays(10, 95, [0], [0], None, [10], [0])
    assert b.schedule([0, 0, 7], 50).tolist() == [K.THROWS_EARLY, K.THROWS_EARLY, K.OUT_OF_RANGE]
    assert b.schedule([0, 0], 95).tolist() == [K.SCHEDULED, K.THROWS_TICKETED] and b.ticket[0] == 110
    with pytest.raises(ValueError):
        b.scan_stale(np.zeros(1, np.uint8), [0], 100 + 10 * (K.MAX_QUANTA + 1))
    assert b.next == 100 and b.ticket[0] == 110


# ---- what the GPU tests' generators cover (tests/test_gpu_collect.py uses exactly these) ------------------

@pytest.mark.parametrize("n_q", [0, 1, 2, 1000])
def test_world_generator_covers_every_verdict(n_q):
    w = K.World(np.random.default_rng(n_q), 5000, n_q)
    a = w.arrays.copy()
    cf = w.ctx_flags.copy()
    lst, v = a.scan_stale(cf, w.num_running, w.now, w.wait_offsets)
    if n_q == 0:
        assert len(lst) == 0 and not v.any()
        return
    assert {int(x) & 0x7F for x in np.unique(v)} == {0, K.BAD_STATE, K.KEPT_ALIVE, K.ACTIVE, K.NOT_STALE, K.COLLECT}
    assert (v & K.NOT_ADDED).any()
    assert 0 < len(lst) < int((v != 0).sum()) < w.n_ctx      # the condemned share: neither nothing nor everything
    if n_q > 1:                                              # ticket order differs from context order
        assert (np.diff(lst.astype(np.int64)) < 0).any()


def test_world_generator_variants():
    rng = np.random.default_rng(9)
    w = K.World(rng, 4097, 1, "all")
    lst, v = w.arrays.copy().scan_stale(w.ctx_flags.copy(), w.num_running, w.now, w.wait_offsets)
    assert lst.tolist() == list(range(4097)) and (v == K.COLLECT).all()
    w = K.World(rng, 4097, 1, "none")
    lst, v = w.arrays.copy().scan_stale(w.ctx_flags.copy(), w.num_running, w.now, w.wait_offsets)
    assert len(lst) == 0 and not v.any()
    w = K.World(rng, 8200, 1, [63, 64, 4095, 4096, 8191])
    lst, v = w.arrays.copy().scan_stale(w.ctx_flags.copy(), w.num_running, w.now, w.wait_offsets)
    assert np.flatnonzero(v).tolist() == [63, 64, 4095, 4096, 8191]


def test_world_generator_covers_the_list_forms_and_scan_all():
    w = K.World(np.random.default_rng(4), 1025, 2)
    ctx = K.targets(np.random.default_rng(5), 20000, 1025, "zipf")
    assert set(w.arrays.copy().schedule(ctx, w.now).tolist()) == set(range(7)) - {K.THROWS_EARLY}
    assert set(w.arrays.copy().schedule(ctx, w.now - 50 * Q).tolist()) >= {K.THROWS_EARLY}
    assert set(w.arrays.copy().cancel(ctx).tolist()) == {0, 1}
    turn = np.random.default_rng(6).integers(0, 10, len(ctx)).astype(np.uint8)
    assert set(w.arrays.copy().touch(w.ctx_flags, ctx, w.now, turn).tolist()) == {K.FALSE, K.TRUE, K.THROWS, K.NO_PART}
    ev = np.random.default_rng(7).integers(0, 8, 1025).astype(np.uint8)
    assert set(w.arrays.copy().idle(ev, w.now).tolist()) == {K.FALSE, K.TRUE, K.THROWS, K.NO_PART}
    a = w.arrays.copy()
    lst, v = a.scan_all(w.ctx_flags.copy(), w.num_running, w.now, 3 * Q, w.wait_offsets)
    assert set(np.unique(v).tolist()) == {0, K.BAD_STATE, K.KEPT_ALIVE, K.ACTIVE, K.NOT_STALE, K.COLLECT}
    assert 0 < len(lst) < int((v != 0).sum()) and (np.diff(lst.astype(np.int64)) > 0).all()
    n_in = w.arrays.count_recent(w.now, 0, 0)
    assert 0 < w.arrays.count_recent(w.now, Q, 2 * Q) < n_in < 1025
