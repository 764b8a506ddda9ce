"""The activation directory's batch calls (gd_actdir_add / remove / set_flags / lookup) on one probe chain.

test_gpu_receive.py fills the table with random ids, where twins in a batch and keys colliding on a slot are
rare.  Here every key shares one home slot (_chain_keys.py) and every batch carries duplicates, so the
in-batch elections (the first add of a key wins, the first removal removes, the last flag update stays),
tombstones inside a chain, their reuse by a later add and a chain that wraps past the table's last slot
all run on purpose.  The table stays at its first size (1,024 slots: every batch has at most 60 items and
live + tombstones + incoming stays far below ad_reserve's 3/4 bound, 768), each step is compared item by
item with oracle/receive.py's ActivationDirectory, and actdir_count() is asserted after each step."""
from functools import lru_cache

import numpy as np
import pytest

import oracle as o
import receive as rv
from _chain_keys import keys_with_home

pytestmark = pytest.mark.gpu

TC = o.grain_type_code(o.PING_GRAIN_CLASS)
AD_CAP = 1024                        # the activation directory's first size (ad_reserve)
HOME_MID, HOME_WRAP = 512, 1016      # 1016: the last home group, a chain of 20 wraps to slot 0
N_FIRST, N_MORE = 20, 15             # the first set; ten fresh keys and five that are never added


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


@lru_cache(maxsize=None)
def _chain(home):
    """(first 20 keys, ten fresh keys, five absent keys) of one home, computed once and shared."""
    first = keys_with_home(TC, AD_CAP, home, N_FIRST)
    more = keys_with_home(TC, AD_CAP, home, N_MORE, start=int(first[-1, 1]) + 1)
    assert len({(int(k[0]), int(k[1]), int(k[2])) for k in np.concatenate([first, more])}) == N_FIRST + N_MORE
    parts = (first, more[:10], more[10:])
    for p in parts:
        p.setflags(write=False)
    return parts


def _t(k):
    return (int(k[0]), int(k[1]), int(k[2]))


class _Model:
    """An engine's activation directory beside the oracle's: every call's report is compared item by
    item (the oracle applies the batch in order), then the count and a lookup of every key of the chain."""

    def __init__(self, gd, home):
        self.e = gd.GrainDispatch(device=0, table_capacity=1024)
        self.ad = rv.ActivationDirectory()
        self.rng = np.random.default_rng(7)
        self.all_keys = np.concatenate(_chain(home))
        self.next_ctx = 100

    def _shuffled(self, keys):
        return np.ascontiguousarray(keys[self.rng.permutation(len(keys))])

    def _check(self):
        assert self.e.actdir_count() == len(self.ad.entries)
        ctx, fl, found = self.e.actdir_lookup(self.all_keys)
        want = [self.ad.entries.get(_t(k)) for k in self.all_keys]
        np.testing.assert_array_equal(found, [w is not None for w in want])
        np.testing.assert_array_equal(ctx, [rv.M32 if w is None else w[0] for w in want])
        np.testing.assert_array_equal(fl, [0 if w is None else w[1] for w in want])

    def add(self, keys, times):
        """Each key `times` times in one shuffled batch; every item its own context and flags."""
        k = self._shuffled(np.repeat(keys, times, axis=0))
        assert len(k) <= 60
        ctx = np.arange(self.next_ctx, self.next_ctx + len(k), dtype=np.uint32)
        self.next_ctx += len(k)
        fl = (1 + np.arange(len(k)) % 7).astype(np.uint8)
        got = self.e.actdir_add(k, ctx, fl)
        want = [self.ad.add(_t(x), int(c), int(f)) for x, c, f in zip(k, ctx, fl)]
        np.testing.assert_array_equal(got, want)
        self._check()
        return np.asarray(want)

    def remove(self, keys):
        k = self._shuffled(keys)
        assert len(k) <= 60
        got = self.e.actdir_remove(k)
        want = [self.ad.remove(_t(x)) for x in k]
        np.testing.assert_array_equal(got, want)
        self._check()
        return np.asarray(want)

    def set_flags(self, keys):
        k = self._shuffled(keys)
        assert len(k) <= 60
        fl = (8 + np.arange(len(k)) % 23).astype(np.uint8)
        got = self.e.actdir_set_flags(k, fl)
        want = [self.ad.set_flags(_t(x), int(f)) for x, f in zip(k, fl)]
        np.testing.assert_array_equal(got, want)
        self._check()
        return np.asarray(want)


def _add_first(m, home):
    """20 keys of one home, each three times, shuffled: 60 items, 20 of them added."""
    first, _, _ = _chain(home)
    added = m.add(first, 3)
    assert added.sum() == N_FIRST and m.e.actdir_count() == N_FIRST


def _remove_half(m, home):
    """Ten of the keys twice each and five absent keys: ten items remove, ten keys stay behind tombstones."""
    first, _, absent = _chain(home)
    removed = m.remove(np.concatenate([first[::2], first[::2], absent]))
    assert removed.sum() == 10 and m.e.actdir_count() == 10


def _readd(m, home):
    """The ten removed keys and ten fresh ones of the same home, each twice: 20 of 40 items added."""
    first, fresh, _ = _chain(home)
    added = m.add(np.concatenate([first[::2], fresh]), 2)
    assert added.sum() == 20 and m.e.actdir_count() == 30


@pytest.mark.parametrize("home", [HOME_MID, HOME_WRAP], ids=["mid", "wrapped"])
def test_add_twins_and_colliders(gd, home):
    m = _Model(gd, home)
    try:
        _add_first(m, home)
    finally:
        m.e.close()


def test_remove_with_duplicates(gd):
    m = _Model(gd, HOME_MID)
    try:
        _add_first(m, HOME_MID)
        _remove_half(m, HOME_MID)
    finally:
        m.e.close()


def test_readd_onto_tombstones(gd):
    m = _Model(gd, HOME_MID)
    try:
        _add_first(m, HOME_MID)
        _remove_half(m, HOME_MID)
        _readd(m, HOME_MID)
    finally:
        m.e.close()


def test_set_flags_on_the_same_chain(gd):
    """After an add, a removal and a re-add the election words must be zero again: set_flags keeps 1 + index
    in them, and a word left behind would outvote a low batch index."""
    m = _Model(gd, HOME_MID)
    try:
        _add_first(m, HOME_MID)
        _remove_half(m, HOME_MID)
        _readd(m, HOME_MID)
        first, fresh, absent = _chain(HOME_MID)
        found = m.set_flags(np.concatenate([first, first[:12], fresh, fresh[:5], absent]))   # 52 items
        assert found.sum() == 47 and m.e.actdir_count() == 30   # all but the five absent keys
    finally:
        m.e.close()
