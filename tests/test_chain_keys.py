"""The colliding-key builder of the chain tests (_chain_keys.py) against a scalar restatement of
home_slot (gd_common.h): the keys it returns are distinct long keys of the requested home, at both ends
of the table too, and the home follows the table size as the header comment says (the top bits of
fmix32 of the uniform hash, whatever the size)."""
import numpy as np
import pytest

import oracle as o
from _chain_keys import HOME_ALIGN, home_slot_np, keys_with_home

TC = o.grain_type_code(o.PING_GRAIN_CLASS)
TCD = o.type_code_data(o.CAT_GRAIN, TC)


def _fmix32(h: int) -> int:
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def _home(key, cap: int) -> int:
    n0, n1, tcd = (int(x) for x in key)
    return ((_fmix32(o.jenkins_u64x3(tcd, n0, n1)) * cap) >> 32) & ~(HOME_ALIGN - 1)


@pytest.mark.parametrize("cap", [4096, 1 << 14])
@pytest.mark.parametrize("where", ["first", "mid", "last"])
def test_keys_with_home(cap, where):
    home = {"first": 0, "mid": (cap // 2 + 264) & ~7, "last": cap - 8}[where]
    keys = keys_with_home(TC, cap, home, 100)
    assert keys.shape == (100, 3) and keys.dtype == np.uint64
    assert len({tuple(int(x) for x in k) for k in keys}) == 100
    assert (keys[:, 0] == 0).all() and (keys[:, 1] < 1 << 32).all() and (keys[:, 2] == TCD).all()
    assert (np.diff(keys[:, 1].astype(np.int64)) > 0).all()                 # id order
    assert [_home(k, cap) for k in keys] == [home] * 100
    log2 = cap.bit_length() - 1
    for k in keys:                                                          # the top bits, whatever the size
        n0, n1, tcd = (int(x) for x in k)
        assert _home(k, cap) >> 3 == _fmix32(o.jenkins_u64x3(tcd, n0, n1)) >> (35 - log2)
    # a later start gives later keys of the same home, none shared; the scan misses none
    more = keys_with_home(TC, cap, home, 30, start=int(keys[-1, 1]) + 1)
    assert int(more[0, 1]) > int(keys[-1, 1]) and [_home(k, cap) for k in more] == [home] * 30
    ids = np.arange(0, int(keys[-1, 1]) + 1)
    brute = [i for i, k in zip(ids, o.grain_keys(TC, ids)) if _home(k, cap) == home] if cap == 4096 else None
    if brute is not None:
        assert brute == [int(x) for x in keys[:, 1]]


def test_home_slot_np_matches_scalar_and_follows_the_table_size():
    rng = np.random.default_rng(3)
    keys = o.grain_keys(TC, rng.integers(0, 1 << 32, size=2000))
    keys[::5, 0] = rng.integers(1, 1 << 62, size=len(keys[::5])).astype(np.uint64)      # Guid-like keys too
    for cap in (8, 4096, 1 << 14, 1 << 21, 1 << 32):
        got = home_slot_np(keys, cap)
        assert [int(x) for x in got] == [_home(k, cap) for k in keys]
        assert (got % HOME_ALIGN == 0).all() and (got < cap).all()
    # doubling the table keeps a grain in the same fraction of it: home(2 cap) >> 1 rounds to home(cap)
    a, b = home_slot_np(keys, 4096), home_slot_np(keys, 8192)
    assert ((b >> np.uint64(1)) & ~np.uint64(7) == a).all()
