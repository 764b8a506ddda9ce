"""CPU tests of the completion / message-pump rule: the regime form equals the literal loop,
one hand-written case per line of the rule, and a lifecycle in which gd_turns' rule, the wait-list merge and
the pump are driven step by step beside per-message Activation objects written from the C#."""
import numpy as np
import pytest

import _pump_ref as P
import _turns_ref as R

V, NR, INV = R.CTX_VALID, R.CTX_NOT_READY, R.CTX_INVALID
HAS, RRO, REENT = R.CTX_HAS_RUNNING, R.CTX_RUNNING_READ_ONLY, R.CTX_REENTRANT
RO, AI, MI, CC = R.MSG_READ_ONLY, R.MSG_ALWAYS_INTERLEAVE, R.MSG_MAY_INTERLEAVE, P.MSG_CALL_CHAIN
ISR, PO = P.DONE_IS_RUNNING, P.DONE_PUMP_ONLY
IDLE, CLEARED, SET = P.PUMP_BECAME_IDLE, P.PUMP_RUNNING_CLEARED, P.PUMP_RUNNING_SET
NONE = R.NONE32


def _same(a, b):
    for name, x, y in zip(P.NAMES, a, b):
        assert x.dtype == y.dtype, name
        np.testing.assert_array_equal(x, y, err_msg=name)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("targets", ["uniform", "zipf"])
def test_regime_form_equals_the_loop(seed, targets):
    rng = np.random.default_rng(seed)
    for n_done, n_ctx in ((0, 5), (1, 1), (700, 1), (3000, 40), (5000, 700), (300, 2000)):
        for fl in (True, False):
            b = P.mixed_pump(rng, n_done, n_ctx, targets, flags=fl)
            _same(P.pump_np(b), P.pump_loop(b))


def test_mixed_batches_reach_every_event_and_state():
    b = P.mixed_pump(np.random.default_rng(5), 5000, 700)
    nr, fl, ndq, rpos, ev, nsb, start = P.pump_loop(b)
    assert set(np.unique(ev).tolist()) >= {0, IDLE, CLEARED, SET, IDLE | CLEARED | SET}
    assert (rpos != NONE).any() and (ndq > 1).any() and (nsb > 1).any() and int(nsb.sum()) == len(start)
    assert (nr > 0x80000000).any()                           # a context driven below zero


def _one(ctx_flags, num_running, wflags, done_flags, done_ctx=None):
    """One context, its list, a run of completions."""
    n = len(done_flags)
    b = P.PumpBatch(np.zeros(n, np.uint32) if done_ctx is None else done_ctx, 1, [ctx_flags], [num_running],
                    [0, len(wflags)], wflags, done_flags)
    out = P.pump_loop(b)
    _same(P.pump_np(b), out)
    nr, fl, ndq, rpos, ev, nsb, start = out
    return int(nr[0]), int(fl[0]), int(ndq[0]), int(rpos[0]), int(ev[0]), nsb.tolist(), start.tolist()


def test_plain_completion_starts_the_head():
    # the Running writer completes: idle, Running cleared, the head starts and becomes Running; the next writer waits
    assert _one(V | HAS, 1, [0, 0], [ISR]) == (1, V | HAS, 1, 0, IDLE | CLEARED | SET, [1], [0])


def test_pump_only_skips_the_reset():
    # nothing completed: numRunning and Running stay; an idle activation's pump starts its head
    assert _one(V | HAS, 1, [0], [PO]) == (1, V | HAS, 0, NONE, 0, [0], [])
    assert _one(V, 0, [RO, 0], [PO | ISR]) == (1, V | HAS | RRO, 1, 0, SET, [1], [0])


def test_is_running_on_a_context_whose_running_is_none():
    # nr 2 -> 1, R stays none, nothing cleared; CanInterleave holds while Running == null: the head starts,
    # becomes Running and blocks the next writer
    assert _one(V, 2, [0, 0, 0], [ISR]) == (2, V | HAS, 1, 0, SET, [1], [0])


def test_second_is_running_flag_changes_nothing_more():
    # the first clears R and its pump makes position 0 Running; the second equals neither X nor a started message
    assert _one(V | HAS, 3, [0, 0], [ISR, ISR]) == (2, V | HAS, 1, 0, CLEARED | SET, [1, 0], [0])


@pytest.mark.parametrize("state", [NR, INV, 3])
def test_not_valid_contexts_reset_but_do_not_pump(state):
    assert _one(state | HAS | REENT, 2, [AI, 0], [ISR, 0]) == (0, state | REENT, 0, NONE, IDLE | CLEARED, [0, 0], [])


def test_read_only_running_takes_the_read_only_run_then_stops_at_the_writer():
    # Running stays X (read-only, not completed): a completion of another reader lets the read-only run in
    assert _one(V | HAS | RRO, 2, [RO, RO, RO, 0, RO], [0]) == (4, V | HAS | RRO, 3, NONE, 0, [3], [0, 1, 2])
    # a writer Running blocks readers too
    assert _one(V | HAS, 2, [RO, RO], [0]) == (1, V | HAS, 0, NONE, 0, [0], [])
    # the started head's own read-only flag decides for the rest
    assert _one(V | HAS, 2, [RO, RO, 0, RO], [ISR]) == (3, V | HAS | RRO, 2, 0, CLEARED | SET, [2], [0, 1])


@pytest.mark.parametrize("bit", [CC, MI, AI])
def test_interleaving_messages_drain_the_list(bit):
    assert _one(V | HAS, 2, [bit] * 5, [0]) == (6, V | HAS, 5, NONE, 0, [5], [0, 1, 2, 3, 4])
    assert _one(V | HAS, 2, [bit, bit, 0, bit], [0]) == (3, V | HAS, 2, NONE, 0, [2], [0, 1])


def test_reentrant_context_drains_the_list():
    assert _one(V | HAS | REENT, 2, [0] * 70, [0]) == (71, V | HAS | REENT, 70, NONE, 0, [70], list(range(70)))


def test_empty_list():
    assert _one(V | HAS, 1, [], [ISR]) == (0, V, 0, NONE, IDLE | CLEARED, [0], [])


def test_nr_reaching_zero_under_the_old_running():
    # the inconsistent case is followed literally: nr == 0 accepts one message while Running stays X
    assert _one(V | HAS, 1, [0, 0], [0]) == (1, V | HAS, 1, NONE, IDLE, [1], [0])


def test_num_running_zero_on_entry_goes_negative():
    assert _one(INV, 0, [0], [0]) == (0xFFFFFFFF, INV, 0, NONE, 0, [0], [])
    # nr <= 0 accepts until it is positive again: -1 -> the pump takes two
    assert _one(V | HAS, 0, [0, 0, 0], [0]) == (1, V | HAS, 2, NONE, 0, [2], [0, 1])


def test_completions_outside_the_contexts_take_no_part():
    ctx = np.array([1, NONE, 0, 7], np.uint32)
    assert _one(V | HAS, 5, [AI], [ISR, ISR, 0, ISR], ctx) == (5, V | HAS, 1, NONE, 0, [0, 0, 1, 0], [0])


def test_a_context_without_completions_is_copied():
    b = P.PumpBatch([1], 2, [V | RRO, V | HAS], [7, 1], [0, 2, 3], [AI, AI, AI], [ISR])
    nr, fl, ndq, rpos, ev, nsb, start = P.pump_loop(b)
    assert (int(nr[0]), int(fl[0]), int(ndq[0]), int(rpos[0]), int(ev[0])) == (7, V | RRO, 0, NONE, 0)
    assert start.tolist() == [2]


def test_start_order_is_by_completion_then_fifo():
    # contexts 0 and 1 interleaved in arrival order
    b = P.PumpBatch([1, 0, 1], 2, [V | REENT, V | HAS], [1, 1], [0, 2, 4], [0, 0, 0, 0], [ISR, 0, 0])
    out = P.pump_loop(b)
    _same(P.pump_np(b), out)
    assert out[5].tolist() == [1, 2, 1] and out[6].tolist() == [2, 0, 1, 3]


def test_merge_loop():
    # context 0 keeps [11], context 1 dequeued everything, context 2 had nothing
    off, msg, fl, total = P.merge_loop(3, [0, 2, 3, 3], [10, 11, 12], [1, 2, 4], [1, 1, 0], [2, 0, 3, 1], [0, 1, 1, 3, 4],
                                       id_base=100, msg_flags=[1, 0, 2, 4])
    assert (off.tolist(), msg.tolist(), fl.tolist(), total) == ([0, 2, 2, 4], [11, 102, 100, 103], [2, 2, 1, 4], 4)
    ta = np.arange(12, dtype=np.uint64).reshape(4, 3)
    sa = ta.copy()
    sa[0, 2] += 1
    off, msg, fl, total = P.merge_loop(3, None, None, None, None, [2, 0, 3, 1], [0, 1, 1, 3, 4], msg_id=[5, 6, 7, 8],
                                       target_activation=ta, sending_activation=sa, chain=True, cap=2)
    assert (off.tolist(), msg.tolist(), fl.tolist(), total) == ([0, 1, 1, 3], [7, 5], [CC, 0], 3)


# ---- lifecycle -------------------------------------------------------------------------------------

class Lifecycle:
    """Steps of turns -> merge -> pump on arrays (the *_loop references, or any callables with their
    signatures) beside the Activation objects, driven with the same events in the same order."""

    def __init__(self, seed, n_ctx=24, turns=R.turns_loop, merge=P.merge_loop, pump=P.pump_loop):
        self.rng = np.random.default_rng(seed)
        self.n_ctx = n_ctx
        self.turns, self.merge, self.pump = turns, merge, pump
        rng = self.rng
        self.flags = np.where(rng.random(n_ctx) < 0.2, NR, V).astype(np.uint8)
        self.flags |= np.where(rng.random(n_ctx) < 0.15, REENT, 0).astype(np.uint8)
        self.nr = np.zeros(n_ctx, np.uint32)
        self.off, self.wmsg, self.wfl = np.zeros(n_ctx + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8)
        self.running_id = [None] * n_ctx                     # the host's copy of Running, from the calls' outputs
        self.acts = [Activation_(bool(f & R.CTX_STATE_MASK == V), bool(f & REENT)) for f in self.flags]
        self.msgs = {}
        self.in_flight = [[] for _ in range(n_ctx)]          # started, not completed
        self.next_id = 0
        self.seen = set()
        self.log = []                                        # per step: the inputs and the two start orders

    def step(self, n):
        rng, n_ctx = self.rng, self.n_ctx
        # -- a received batch of requests
        ctx = rng.integers(0, n_ctx, n).astype(np.uint32)
        mf = P.wait_flags(rng, n, 0.5, 0.06) & np.uint8(7)
        ta = rng.integers(0, 1 << 60, (n, 3), dtype=np.uint64)
        sa = ta.copy()
        diff = rng.random(n) < 0.9
        sa[diff, 1] += np.uint64(1)
        ids = np.arange(self.next_id, self.next_id + n, dtype=np.uint32)
        self.next_id += n
        b = R.Batch(ctx, n_ctx, self.flags, self.nr, np.zeros(n_ctx), msg_flags=mf, target_activation=ta,
                    sending_activation=sa, chain=True)
        turn, nro, run_idx, start_idx, wperm, woff = self.turns(b)
        started = []
        for i in range(n):
            m = P.Message(int(ids[i]), mf[i] & RO, mf[i] & AI, mf[i] & MI, not diff[i])
            self.msgs[m.id] = m
            if self.acts[ctx[i]].receive_request(m):
                started.append(i)
                self.in_flight[ctx[i]].append(m)
        assert started == start_idx.tolist()
        for c in np.flatnonzero(run_idx != NONE):
            self.running_id[c] = int(ids[run_idx[c]])
        self.nr = nro
        self.flags = self.flags.copy()
        has = run_idx != NONE
        self.flags[has] |= HAS
        if n:
            self.flags[has & ((mf[np.minimum(run_idx, n - 1)] & RO) != 0)] |= RRO
        # -- the batch's WAIT messages join the lists (nothing was dequeued since the last merge: the pump's
        # -- n_dequeued is applied right below, in the same step)
        self.off, self.wmsg, self.wfl, total = self.merge(n_ctx, self.off, self.wmsg, self.wfl, None, wperm, woff,
                                                          msg_id=ids, msg_flags=mf, target_activation=ta,
                                                          sending_activation=sa, chain=True)
        assert total == len(self.wmsg)
        self._compare()
        # -- NOT_READY activations turn Valid: a bare RunMessagePump (Catalog.cs:1146-1158); then a random
        # -- subset of the running turns completes, in a random order
        done_ctx, done_flags, done_msg, flips = [], [], [], []
        for c in range(n_ctx):
            if self.flags[c] & R.CTX_STATE_MASK == NR and rng.random() < 0.3:
                self.flags[c] = (self.flags[c] & ~np.uint8(R.CTX_STATE_MASK)) | V
                self.acts[c].valid = True
                flips.append(c)
                done_ctx.append(c), done_flags.append(PO), done_msg.append(None)
            for m in list(self.in_flight[c]):
                if rng.random() < 0.5:
                    self.in_flight[c].remove(m)
                    done_ctx.append(c), done_flags.append(ISR if self.running_id[c] == m.id else 0), done_msg.append(m)
        order = rng.permutation(len(done_ctx))
        done_ctx = np.array(done_ctx, np.uint32)[order]
        done_flags = np.array(done_flags, np.uint8)[order]
        done_msg = [done_msg[k] for k in order]
        pb = P.PumpBatch(done_ctx, n_ctx, self.flags, self.nr, self.off, self.wfl, done_flags, self.wmsg)
        nr, fl, ndq, rpos, ev, nsb, start = self.pump(pb)
        obj_start, obj_by = [], []
        for a in self.acts:
            a.became_idle = False
        for c, m in zip(done_ctx.tolist(), done_msg):
            a = self.acts[c]
            s = a.run_message_pump() if m is None else a.on_completed_request(m)
            obj_start += [x.id for x in s]
            obj_by.append(len(s))
            self.in_flight[c] += s
        assert self.wmsg[start].tolist() == obj_start and nsb.tolist() == obj_by
        assert [bool(e & IDLE) for e in ev] == [a.became_idle for a in self.acts]
        self.log.append(dict(ctx=ctx, msg_flags=mf, ta=ta, sa=sa, ids=ids, done_ctx=done_ctx, done_flags=done_flags,
                             flips=np.array(flips, np.int64), turn_start=start_idx, pump_start_ids=self.wmsg[start].copy()))
        for c in range(n_ctx):
            if ev[c] & CLEARED:
                self.running_id[c] = None
            if rpos[c] != NONE:
                self.running_id[c] = int(self.wmsg[rpos[c]])
        self.seen |= set(np.unique(ev).tolist())
        self.nr, self.flags = nr, fl
        self.off, self.wmsg, self.wfl, _ = self.merge(n_ctx, self.off, self.wmsg, self.wfl, ndq,
                                                      np.zeros(0, np.uint32), np.zeros(n_ctx + 2, np.uint32))
        self._compare()

    def _compare(self):
        for c, a in enumerate(self.acts):
            assert a.num_running == P._i32(self.nr[c]), c
            assert (a.running is not None) == bool(self.flags[c] & HAS), c
            assert (None if a.running is None else a.running.id) == self.running_id[c], c
            if a.running is not None:
                assert a.running.read_only == bool(self.flags[c] & RRO), c
            assert [m.id for m in a.waiting] == self.wmsg[self.off[c]:self.off[c + 1]].tolist(), c
            assert [bool(m.call_chain) for m in a.waiting] == \
                [bool(f & CC) for f in self.wfl[self.off[c]:self.off[c + 1]]], c


Activation_ = P.Activation


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_lifecycle_against_the_activation_objects(seed):
    life = Lifecycle(seed)
    for n in (60, 5, 90, 0, 40, 70, 30, 50):
        life.step(n)
    assert life.seen >= {0, IDLE | CLEARED, CLEARED | SET, IDLE | CLEARED | SET}
    assert any(a.waiting for a in life.acts) and any(a.num_running for a in life.acts)
