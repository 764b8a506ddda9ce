"""GPU parity for the callback table: gd_callbacks_* and their device forms through the C ABI
against the literal restatement of InsideRuntimeClient's callbacks dictionary (_callbacks_ref.Table), every output
bit for bit, dtype included, and the table's contents through lookup and count after every call."""
import ctypes as C

import numpy as np
import pytest

import _callbacks_ref as R
from _callbacks_ref import (CB_FIRE, CB_GATEWAY_BACK, CB_NO_CALLBACK, CB_NONE, CB_RESEND, CB_SILO_FAILED, CB_TIMEOUT,
                            NO_HANDLE, NO_SILO, Options, Table)

pytestmark = pytest.mark.gpu

EDGES = [0, 1, 63, 64, 65, 4095, 4096, 4097]      # a wave, the fire list's 4,096-byte tile
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


@pytest.fixture()
def eng(gd):
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        yield e


def home_group(i, cap):
    """gd_callbacks.h cb_home: the id's home group of 4 slots."""
    x = int(i) & M64
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & M64
    x ^= x >> 31
    return (x * (cap // 4)) >> 64


class Mirror:
    """The engine's table and the literal one, driven together."""

    def __init__(self, e, hint, max_resend=0, resend_on_timeout=False, period=0):
        self.e, self.t = e, Table(Options(max_resend, resend_on_timeout, period))
        e.callbacks_configure(hint, max_resend, resend_on_timeout, period)
        self.seen = set()

    def verify(self, extra=()):
        ids = np.array(sorted(self.seen | set(int(x) for x in extra)), np.int64)
        _eq(self.e.callbacks_lookup(ids), self.t.lookup(ids), ("handle", "resend", "silo", "found"))
        live, cap = self.e.callbacks_count()
        assert live == self.t.count()
        return cap

    def add(self, ids, handles, deadlines):
        self.seen |= set(int(x) for x in ids)
        _eq((self.e.callbacks_add(ids, handles, deadlines),), (self.t.add(ids, handles, deadlines),), ("added",))
        return self.verify()

    def set_target(self, ids, silo):
        self.seen |= set(int(x) for x in ids)
        _eq((self.e.callbacks_set_target(ids, silo),), (self.t.set_target(ids, silo),), ("found",))
        self.verify()

    def respond(self, ids, result=None, rejection=None, flags=None, turn=None):
        self.seen |= set(int(x) for x in ids)
        want = self.t.respond(ids, result, rejection, flags, turn)
        _eq(self.e.callbacks_respond(ids, result, rejection, flags, turn), want, ("outcome", "flags", "handle", "fire_idx"))
        self.verify()
        return want

    def scan(self, which, arg, cap=None):
        want = getattr(self.t, which)(arg)
        got = getattr(self.e, "callbacks_" + which)(arg, len(want[0]) if cap is None else cap)
        o = np.argsort(got[0], kind="stable")                # timers have no order: compared as sets, sorted by id
        _eq(tuple(a[o] for a in got), want, ("id", "handle", "kind"))
        self.verify()
        return want


def _eq(got, want, names):
    assert len(got) == len(want) == len(names)
    for name, a, b in zip(names, got, want):
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a, b, err_msg=name)


def fresh_ids(rng, n, lo=1):
    """Distinct ids: a counter's run (what CorrelationId.GetNext gives) in a random order, some negative."""
    ids = np.arange(lo, lo + n, dtype=np.int64)
    ids[::7] *= -1
    rng.shuffle(ids)
    return ids


def filled(e, n, max_resend=0, hint=8192, seed=0):
    rng = np.random.default_rng(seed)
    m = Mirror(e, hint, max_resend)
    ids = fresh_ids(rng, n)
    m.add(ids, rng.integers(0, 1 << 32, n, dtype=np.uint32), rng.integers(-5, 1 << 40, n, dtype=np.int64))
    return m, rng


# ---- add -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", EDGES)
def test_add_shapes(eng, n):
    rng = np.random.default_rng(n)
    m = Mirror(eng, 16384)
    ids = fresh_ids(rng, n)
    m.add(ids, np.arange(n, dtype=np.uint32), rng.integers(0, 1 << 50, n, dtype=np.int64))
    m.verify(extra=fresh_ids(rng, 50, lo=1 << 40))          # absent ids stay absent
    # the same batch again adds nothing; half old, half new
    m.add(ids, np.zeros(n, np.uint32), np.zeros(n, np.int64))
    if n > 1:
        mix = np.r_[ids[: n // 2], fresh_ids(rng, n - n // 2, lo=1 << 30)]
        rng.shuffle(mix)
        m.add(mix, np.arange(n, dtype=np.uint32) + 9, np.full(n, 3, np.int64))


def test_add_duplicates_first_wins(eng):
    """One id twice in a wave, across waves, across workgroups; and a 64-fold twin filling a wave."""
    m = Mirror(eng, 4096)
    n = 1024
    ids = np.arange(1000, 1000 + n, dtype=np.int64)
    for a, b in [(3, 4), (10, 200), (20, 700), (255, 256), (63, 64)]:
        ids[b] = ids[a]
    ids[320:384] = 77
    ids[900] = 77
    m.add(ids, np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.int64))
    h, _, _, f = eng.callbacks_lookup(np.array([1003, 1010, 1020, 1255, 1063, 77], np.int64))
    assert list(h) == [3, 10, 20, 255, 63, 320] and f.all()
    # re-add of a live id, alone and twice in the batch
    m.add(np.array([77, 1003, 5, 5], np.int64), np.array([1, 2, 3, 4], np.uint32), np.zeros(4, np.int64))


def test_add_after_fire_takes_the_tombstone(eng):
    m, rng = filled(eng, 2000, hint=4096)
    cap = m.verify()
    assert cap == 4096
    ids = np.array(sorted(m.t.d), np.int64)
    for _ in range(3):                                       # the third round's adds need the counters: 4,000 > 3,072
        m.respond(ids[:1000])
        assert m.add(ids[:1000], np.arange(1000, dtype=np.uint32), np.zeros(1000, np.int64)) == cap
    assert m.t.count() == 2000


# ---- a small table: long chains that wrap ---------------------------------------------------------

def test_small_table_chains_wrap(eng):
    m = Mirror(eng, 64)
    pool = np.arange(1, 4000, dtype=np.int64)
    g = np.array([home_group(i, 64) for i in pool])
    late = pool[g >= 13][:48]                                # 48 entries homed in the last 12 slots: they wrap
    assert len(late) == 48
    assert m.add(late, np.arange(48, dtype=np.uint32), np.arange(48, dtype=np.int64)) == 64
    absent = pool[g >= 13][48:96]
    assert len(absent) == 48
    h, _, _, f = eng.callbacks_lookup(np.r_[late, absent])
    assert f[:48].all() and not f[48:].any() and list(h[:48]) == list(range(48))
    # fire every other one and look again: tombstones keep the chains whole
    m.respond(late[::2])
    m.verify(extra=absent)
    m.add(absent[:10], np.arange(10, dtype=np.uint32), np.zeros(10, np.int64))


def _tombstoned_chain_add(e, device):
    """28 entries homed in the last three groups of a 64-slot table (the engine's minimum): one chain over slots
    52 .. 63, 0 .. 15.  Every other one fires, which leaves 14 tombstones inside it.  Then one batch of 20 items adds
    15 new ids, every third of them twice; 28 + 20 = 48 is all the 0.75 load rule admits without a rebuild, which
    would sweep the tombstones under test away.  The new ids are homed in the chain's first group, so every
    tombstone lies ahead of every one of them and the counts afterwards do not depend on which lane claims first:
    14 tombstones reused, one EMPTY slot taken, 29 live, no tombstone, 64 slots.  device: the batch goes through
    gd_callbacks_add_device (the gated passes), else gd_callbacks_add (read-back-driven ones).  Returns the
    batch's `added` and what a lookup of its ids finds."""
    import torch
    m = Mirror(e, 64)
    pool = np.arange(1, 4000, dtype=np.int64)
    g = np.array([home_group(i, 64) for i in pool])
    old = pool[g >= 13][:28]
    assert m.add(old, np.arange(28, dtype=np.uint32) + 100, np.arange(28, dtype=np.int64)) == 64
    m.respond(old[::2])
    new = np.setdiff1d(pool[g == 13], old)[:15]
    assert len(new) == 15
    batch = np.r_[new, new[2::3]]
    np.random.default_rng(3).shuffle(batch)                  # twins at any distance, either order
    handles, dl = np.arange(20, dtype=np.uint32) + 500, np.arange(20, dtype=np.int64) + 7
    want = m.t.add(batch, handles, dl)
    assert want.sum() == 15
    m.seen |= set(int(x) for x in batch)
    if device:
        dev = torch.device("cuda:0")
        d_ids, d_h, d_dl = (torch.from_numpy(a.view(np.uint8).copy()).to(dev) for a in (batch, handles, dl))
        d_added = torch.zeros(20, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        e.callbacks_add_device(d_ids.data_ptr(), d_h.data_ptr(), d_dl.data_ptr(), 20, d_added.data_ptr())
        e.synchronize()
        added = d_added.cpu().numpy().copy()
    else:
        added = e.callbacks_add(batch, handles, dl)
    _eq((added,), (want,), ("added",))                       # the first item of each id, not its repeats
    # the next synchronising calls report no GD_ETIMEOUT (they raise on one); survivors, fired and new ids as the model
    assert m.verify() == 64 and e.callbacks_count() == (29, 64)
    # no tombstone is left: 19 more adds fit the host's bound, 29 + 0 + 19 <= 48, without the rebuild that one
    # leftover tombstone would bring
    e.set_kernel_timing(True)
    e.kernel_times_reset()
    more = pool[g == 5][:19]
    m.add(more, np.zeros(19, np.uint32), np.zeros(19, np.int64))
    times = e.kernel_times()
    e.set_kernel_timing(False)
    assert "k_cb_claim" in times and "k_cb_rebuild" not in times
    return (added,) + tuple(e.callbacks_lookup(batch))


def test_tombstoned_wrapped_chain_device_form(eng):
    _tombstoned_chain_add(eng, device=True)


def test_tombstoned_wrapped_chain_host_form_matches_device(eng):
    host = _tombstoned_chain_add(eng, device=False)
    eng.callbacks_clear()
    dev = _tombstoned_chain_add(eng, device=True)
    _eq(host, dev, ("added", "handle", "resend", "silo", "found"))


# ---- respond ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", EDGES)
def test_respond_shapes_mixed(eng, n):
    max_resend = (0, 1, 3)[n % 3]
    m, rng = filled(eng, 3000, max_resend, seed=n)
    ids, res, rej, fl = R.mixed_batch(rng, m.t, n)
    want = m.respond(ids, res, rej, fl)
    if n >= 4095:
        assert len(set(want[0])) == (4 if max_resend else 3) and len(want[3]) > 100


def test_respond_each_rule(eng):
    m, _ = filled(eng, 64, 2)
    ids = np.array(sorted(m.t.d), np.int64)
    U8 = lambda *a: np.array(a, np.uint8)
    o = m.respond(ids[:1], U8(2), U8(0), U8(1))[0]                               # 1: gateway back
    assert o[0] == CB_GATEWAY_BACK
    for rej, hdr in [(0, 0), (3, 0), (0, 2), (3, 2), (1, 0), (2, 0), (4, 0)]:     # 2: the invalidation bit
        f = m.respond(np.array([-999], np.int64), U8(2), U8(rej), U8(hdr))[1]
        assert f[0] == (1 if rej in (0, 3) and not hdr else 0)
    assert m.respond(np.array([-999], np.int64))[0][0] == CB_NO_CALLBACK          # 3
    m.set_target(ids[1:2], np.array([5], np.uint32))
    assert m.respond(ids[1:2], U8(2), U8(0))[0][0] == CB_RESEND                   # 4, twice, then 5
    assert m.respond(ids[1:2], U8(2), U8(0))[0][0] == CB_RESEND
    assert m.respond(ids[1:2], U8(2), U8(0))[0][0] == CB_FIRE
    assert m.respond(ids[2:3], U8(2), U8(1))[0][0] == CB_FIRE                     # 5: not transient
    assert m.respond(ids[3:4], U8(1))[0][0] == CB_FIRE
    assert m.respond(ids[4:5])[0][0] == CB_FIRE                                   # all arrays NULL
    assert m.respond(ids[4:5])[0][0] == CB_NO_CALLBACK


@pytest.mark.parametrize("max_resend", [0, 1, 3])
def test_respond_one_id_many_times(eng, max_resend):
    """An id answered 2, 3 and 5 times in one batch; transient rejections before and after a Success."""
    m, rng = filled(eng, 600, max_resend)
    ids = np.array(sorted(m.t.d), np.int64)
    T, S, O = (2, 0), (0, 0), (2, 1)                         # transient rejection, Success, Overloaded rejection
    cases = [[T, S], [S, T], [T, T], [T, T, S], [S, T, T], [T, S, T], [T, T, T, T, T], [T, T, T, S, T], [S, S, S, S, S],
             [T, O, T], [T, T, T, T, O]]
    batch = []
    for k, c in enumerate(cases * 6):
        batch += [(ids[k], r, j) for r, j in c]
    # spread each id's answers over waves and workgroups, keeping their order
    pad = [(int(x), 0, 0) for x in ids[300:600]]
    order = np.sort(rng.choice(len(batch) + len(pad), len(batch), replace=False))
    full = [None] * (len(batch) + len(pad))
    for p, b in zip(order, batch):
        full[p] = b
    it = iter(pad)
    full = [b if b is not None else next(it) for b in full]
    bi = np.array([b[0] for b in full], np.int64)
    want = m.respond(bi, np.array([b[1] for b in full], np.uint8), np.array([b[2] for b in full], np.uint8))
    assert (CB_RESEND in want[0]) == (max_resend > 0)
    # and once more over the survivors, with the resend counts they now carry
    left = np.array(sorted(m.t.d), np.int64)
    m.respond(np.repeat(left, 3), np.full(3 * len(left), 2, np.uint8), np.zeros(3 * len(left), np.uint8))


def test_respond_turn_mask_and_fire_order_across_tiles(eng):
    m, rng = filled(eng, 6000, 1)
    ids = np.array(sorted(m.t.d), np.int64)
    rng.shuffle(ids)
    n = 4096 + 300
    turn = np.full(n, 8, np.uint8)
    turn[rng.choice(n, 500, replace=False)] = rng.choice(np.array([0, 1, 2, 9], np.uint8), 500)
    turn[4094:4098] = 8                                      # fires on both sides of the tile edge
    res = np.zeros(n, np.uint8)
    res[::11] = 2
    res[4094:4098] = 0
    want = m.respond(ids[:n], res, np.zeros(n, np.uint8), None, turn)
    assert {4094, 4095, 4096, 4097} <= set(want[3]) and np.all(np.diff(want[3].astype(np.int64)) > 0)
    assert np.all(want[0][turn != 8] == CB_NONE)


def test_respond_device_after_turns_device(gd, eng):
    """gd_turns_device -> gd_callbacks_respond_device on its d_turn, nothing read back in between; the adds and the
    targets go in through the device forms too."""
    import torch
    dev = torch.device("cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
    host = lambda t, dt: t.cpu().numpy().view(dt).copy()
    rng = np.random.default_rng(5)
    n, n_ctx = 5000, 37
    m = Mirror(eng, 16384, 1)
    ids = fresh_ids(rng, n)
    handles, dl = np.arange(n, dtype=np.uint32), rng.integers(0, 1000, n, dtype=np.int64)
    silo = rng.integers(0, 9, n, dtype=np.uint32)
    d_ids, d_h, d_dl, d_silo = d(ids), d(handles), d(dl), d(silo)
    d_added, d_found = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    eng.callbacks_add_device(d_ids.data_ptr(), d_h.data_ptr(), d_dl.data_ptr(), n, d_added.data_ptr())
    eng.callbacks_set_target_device(d_ids.data_ptr(), d_silo.data_ptr(), n, d_found.data_ptr())
    # a received batch: requests and responses over valid and invalid activations
    ctx = rng.integers(0, n_ctx, n, dtype=np.uint32)
    direction = rng.choice(np.array([0, 1], np.uint8), n)
    cflags = rng.choice(np.array([0, 2], np.uint8), n_ctx, p=[0.8, 0.2])      # VALID / INVALID
    nr = np.zeros(n_ctx, np.uint32)
    want_turn = eng.turns(ctx, n_ctx, cflags, nr, None, direction=direction, lists=False)[0]
    assert (want_turn == 8).sum() > 1000 and (want_turn == 9).sum() > 100
    resp_ids = ids.copy()
    resp_ids[::9] = ids[1::9][: len(resp_ids[::9])]          # some ids answered twice
    res = rng.choice(np.array([0, 2], np.uint8), n, p=[0.7, 0.3])
    rej = rng.choice(np.array([0, 1], np.uint8), n)
    d_ctx, d_dir, d_cf, d_nr = d(ctx), d(direction), d(cflags), d(nr)
    d_rid, d_res, d_rej = d(resp_ids), d(res), d(rej)
    d_turn = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_nro, d_ridx = torch.zeros(n_ctx * 4, dtype=torch.uint8, device=dev), torch.zeros(n_ctx * 4, dtype=torch.uint8, device=dev)
    d_oc, d_of = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    d_oh, d_fi = torch.zeros(n * 4, dtype=torch.uint8, device=dev), torch.zeros(n * 4, dtype=torch.uint8, device=dev)
    d_nf = torch.zeros(4, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.turns_device(d_ctx.data_ptr(), None, d_dir.data_ptr(), None, None, None, None, None, n, n_ctx,
                     eng.turn_state_device(d_cf.data_ptr(), d_nr.data_ptr()), d_turn.data_ptr(), d_nro.data_ptr(),
                     d_ridx.data_ptr())
    eng.callbacks_respond_device(d_rid.data_ptr(), d_res.data_ptr(), d_rej.data_ptr(), None, d_turn.data_ptr(), n,
                                 d_oc.data_ptr(), d_of.data_ptr(), d_oh.data_ptr(), d_fi.data_ptr(), d_nf.data_ptr())
    eng.synchronize()
    _eq((host(d_added, np.uint8),), (m.t.add(ids, handles, dl),), ("added",))
    _eq((host(d_found, np.uint8),), (m.t.set_target(ids, silo),), ("found",))
    np.testing.assert_array_equal(host(d_turn, np.uint8), want_turn)
    want = m.t.respond(resp_ids, res, rej, None, want_turn)
    nf = int(host(d_nf, np.uint32)[0])
    _eq((host(d_oc, np.uint8), host(d_of, np.uint8), host(d_oh, np.uint32), host(d_fi, np.uint32)[:nf]), want,
        ("outcome", "flags", "handle", "fire_idx"))
    m.seen |= set(int(x) for x in ids)
    m.verify()


# ---- churn ------------------------------------------------------------------------------------------

def test_churn_steady_state_does_not_grow(eng):
    """200 cycles of add 4,096 / respond 4,096 on a table configured for 8,192."""
    m = Mirror(eng, 8192)
    e, n = m.e, 4096
    assert e.callbacks_count() == (0, 8192)
    hd, dl = np.arange(n, dtype=np.uint32), np.zeros(n, np.int64)
    for c in range(200):
        ids = np.arange(c * n + 1, (c + 1) * n + 1, dtype=np.int64)
        added = e.callbacks_add(ids, hd, dl)
        assert added.all()
        if c == 199:
            m.t.add(ids, hd, dl)
            m.seen = set(int(x) for x in ids)
            assert m.verify(extra=range(1, 300)) == 8192     # the last cycle's ids are all found, old ones are not
            m.respond(ids)
        else:
            oc = e.callbacks_respond(ids, fire=False)[0]
            assert (oc == CB_FIRE).all()
    assert e.callbacks_count() == (0, 8192)


@pytest.mark.parametrize("batches", [1, 3])
def test_growth(eng, batches):
    m = Mirror(eng, 1024)
    rng = np.random.default_rng(batches)
    ids = fresh_ids(rng, 3 * 1024)
    cap = 1024
    for part in np.split(ids, batches):
        cap = m.add(part, np.arange(len(part), dtype=np.uint32), np.zeros(len(part), np.int64))
    assert cap == 4096 and m.t.count() == 3072
    m.verify(extra=fresh_ids(rng, 100, lo=1 << 33))
    m.respond(ids[::2])


# ---- expire / break_silo ----------------------------------------------------------------------------

@pytest.mark.parametrize("resend_on_timeout", [False, True])
def test_expire(gd, eng, resend_on_timeout):
    m = Mirror(eng, 1024, 1, resend_on_timeout, 50)
    n = 300
    ids = np.arange(1, n + 1, dtype=np.int64)
    dl = np.where(ids % 3 == 0, 999, np.where(ids % 3 == 1, 1000, 1001)).astype(np.int64)   # now - 1, now, now + 1
    m.add(ids, (ids * 3).astype(np.uint32), dl)
    m.set_target(ids[:50], np.full(50, 2, np.uint32))
    due = int((dl <= 1000).sum())
    # cap one short: GD_EINVAL and the table is unchanged
    with pytest.raises(gd.GrainDispatchError) as ei:
        m.e.callbacks_expire(1000, due - 1)
    assert ei.value.code == gd.GD_EINVAL
    m.verify()
    want = m.scan("expire", 1000)
    assert len(want[0]) == due and set(want[2]) == {CB_RESEND if resend_on_timeout else CB_TIMEOUT}
    assert len(m.scan("expire", 1000)[0]) == 0               # one tick a call
    want = m.scan("expire", 1050, cap=2000)                  # the second tick: the resent ones time out
    assert len(want[0]) == (n if resend_on_timeout else n - due)
    if resend_on_timeout:
        assert (want[2] == CB_TIMEOUT).sum() == due and (want[2] == CB_RESEND).sum() == n - due
    m.scan("expire", 1 << 60, cap=n)
    assert m.t.count() == 0


@pytest.mark.parametrize("resend_on_timeout", [False, True])
def test_break_silo(gd, eng, resend_on_timeout):
    m = Mirror(eng, 1024, 2, resend_on_timeout, 50)
    n = 200
    ids = np.arange(1, n + 1, dtype=np.int64)
    m.add(ids, ids.astype(np.uint32), np.full(n, 7, np.int64))
    silo = np.full(n, 4, np.uint32)
    silo[0] = 5
    silo[1] = R.NO_SILO
    m.set_target(ids, silo)
    m.set_target(np.array([2, 2, 3], np.int64), np.array([4, 6, NO_SILO], np.uint32))        # the last stands
    assert len(m.scan("break_silo", 9)[0]) == 0              # a silo with no entry
    assert len(m.scan("break_silo", 5)[0]) == 1              # ... with one
    with pytest.raises(gd.GrainDispatchError) as ei:
        m.e.callbacks_break_silo(4, n - 5)
    assert ei.value.code == gd.GD_EINVAL
    m.verify()
    want = m.scan("break_silo", 4)                           # ... with all the rest
    assert len(want[0]) == n - 3 and set(want[2]) == {CB_RESEND if resend_on_timeout else CB_SILO_FAILED}
    assert len(m.scan("break_silo", 4)[0]) == 0
    m.scan("expire", 7, cap=n)                               # break_silo left the deadlines alone


# ---- errors -----------------------------------------------------------------------------------------

def test_argument_errors_clear_and_capture_refusal(gd, eng):
    import torch
    lib, h = gd.lib, eng.h
    Pt = lambda a: C.c_void_p(a.ctypes.data)
    ids, hd, dl = np.array([1, 2], np.int64), np.array([1, 2], np.uint32), np.array([5, 6], np.int64)
    o8, o32, one = np.zeros(4, np.uint8), np.zeros(4, np.uint32), np.zeros(1, np.uint32)
    # before configure: GD_ESTATE; a NULL handle: GD_EINVAL
    assert lib.gd_callbacks_add(h, Pt(ids), Pt(hd), Pt(dl), 2, None) == gd.GD_ESTATE
    assert lib.gd_callbacks_count(h, None, None) == gd.GD_ESTATE
    assert lib.gd_callbacks_add(None, Pt(ids), Pt(hd), Pt(dl), 2, None) == gd.GD_EINVAL
    assert lib.gd_callbacks_configure(h, 64, 256, 0, 0) == gd.GD_EINVAL
    assert lib.gd_callbacks_configure(h, 64, 1, 0, -1) == gd.GD_EINVAL
    m = Mirror(eng, 64)
    big = (1 << 31) + 1
    assert lib.gd_callbacks_add(h, None, Pt(hd), Pt(dl), 2, None) == gd.GD_EINVAL
    assert lib.gd_callbacks_add(h, Pt(ids), None, Pt(dl), 2, None) == gd.GD_EINVAL
    assert lib.gd_callbacks_add(h, Pt(ids), Pt(hd), None, 2, None) == gd.GD_EINVAL
    assert lib.gd_callbacks_add(h, Pt(ids), Pt(hd), Pt(dl), big, None) == gd.GD_EINVAL
    assert lib.gd_callbacks_add(h, None, None, None, 0, None) == gd.GD_OK
    assert lib.gd_callbacks_set_target(h, Pt(ids), None, 2, None) == gd.GD_EINVAL
    assert lib.gd_callbacks_set_target(h, Pt(ids), Pt(np.array([1, 0xFFFF], np.uint32)), 2, None) == gd.GD_EINVAL
    assert lib.gd_callbacks_lookup(h, None, 2, None, None, None, None) == gd.GD_EINVAL
    assert lib.gd_callbacks_lookup(h, Pt(ids), big, None, None, None, None) == gd.GD_EINVAL
    resp = lambda i=Pt(ids), oc=Pt(o8), fi=None, nf=None, n=2: lib.gd_callbacks_respond(
        h, i, None, None, None, None, n, oc, Pt(o8), Pt(o32), fi, nf)
    assert resp(i=None) == gd.GD_EINVAL and resp(oc=None) == gd.GD_EINVAL and resp(n=big) == gd.GD_EINVAL
    assert resp(fi=Pt(o32)) == gd.GD_EINVAL and resp(nf=Pt(one)) == gd.GD_EINVAL
    assert lib.gd_callbacks_expire(h, 0, 4, Pt(dl), Pt(o32), Pt(o8), None) == gd.GD_EINVAL
    assert lib.gd_callbacks_expire(h, 0, 4, None, Pt(o32), Pt(o8), Pt(one)) == gd.GD_EINVAL
    assert lib.gd_callbacks_break_silo(h, 0xFFFF, 4, Pt(dl), Pt(o32), Pt(o8), Pt(one)) == gd.GD_EINVAL
    m.verify(extra=[1, 2])                                   # none of it touched the table
    # clear
    m.add(ids, hd, dl)
    eng.callbacks_clear()
    m.t = Table()
    assert m.verify() == 64
    m.add(ids, hd, dl)
    # inside a stream capture a call that needs a read-back is refused before anything is launched: every host
    # form, and the device add once its room cannot be told without the counters
    dev = torch.device("cuda:0")
    n = 60                                                   # 2 + 60 > 0.75 * 64
    d_ids = torch.arange(100, 100 + n, dtype=torch.int64, device=dev)
    d_hd = torch.zeros(n, dtype=torch.int32, device=dev)
    d_dl = torch.zeros(n, dtype=torch.int64, device=dev)
    mine = torch.zeros(4, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.set_stream(s.cuda_stream)
    eng.set_kernel_timing(True)
    eng.kernel_times_reset()
    g = torch.cuda.CUDAGraph()
    codes = []
    with torch.cuda.graph(g, stream=s):
        mine.add_(1)                                         # the capture holds one node of the test's own
        for call in (lambda: eng.callbacks_add_device(d_ids.data_ptr(), d_hd.data_ptr(), d_dl.data_ptr(), n),
                     lambda: eng.callbacks_respond(ids), lambda: eng.callbacks_count(),
                     lambda: eng.callbacks_expire(0, 4)):
            with pytest.raises(gd.GrainDispatchError) as ei:
                call()
            codes.append(ei.value.code)
    eng.set_stream(None)
    assert codes == [gd.GD_ESTATE] * 4
    assert not any(k.startswith("k_") for k in eng.kernel_times())
    eng.set_kernel_timing(False)
    m.verify(extra=range(100, 160))
