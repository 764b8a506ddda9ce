"""Grain keys that collide in the directory table: a numpy restatement of home_slot (gd_common.h) and a
builder of long keys sharing one home, for the tests that need long, wrapped or tombstoned probe chains
(test_gpu_dir_chains.py).  Checked on the CPU by test_chain_keys.py."""
import numpy as np

import oracle as o

HOME_ALIGN = 8          # gd_common.h HOME_ALIGN (SLOT_GROUP 1)


def home_slot_np(keys, cap: int) -> np.ndarray:
    """home_slot of each (n0, n1, tcd) key in a table of `cap` slots (a power of two, at most 2^32):
    ((fmix32(uniform hash) * cap) >> 32) & ~(HOME_ALIGN - 1)."""
    assert cap >= HOME_ALIGN and cap & (cap - 1) == 0 and cap <= 1 << 32
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    h = o.jenkins_u64x3_np(keys[:, 2], keys[:, 0], keys[:, 1])
    m = o.fmix32_np(h).astype(np.uint64)                      # < 2^32, cap <= 2^32: the product fits in u64
    return ((m * np.uint64(cap)) >> np.uint64(32)) & ~np.uint64(HOME_ALIGN - 1)


def keys_with_home(type_code: int, cap: int, home: int, count: int, start: int = 0) -> np.ndarray:
    """The first `count` long keys (N0 = 0, N1 = id < 2^32, so the 8-B index holds them) of class
    `type_code` with id >= start whose home slot in a table of `cap` slots is `home`, in id order."""
    assert 0 <= home < cap and home % HOME_ALIGN == 0
    found, n, lo = [], 0, int(start)
    chunk = min(1 << 20, max(4096, 2 * count * (cap // HOME_ALIGN)))   # ~2 * count hits expected a chunk
    while n < count:
        assert lo + chunk <= 1 << 32, "ran out of 32-bit ids"
        k = o.grain_keys(type_code, np.arange(lo, lo + chunk))
        hit = k[home_slot_np(k, cap) == np.uint64(home)]
        found.append(hit)
        n += len(hit)
        lo += chunk
    return np.concatenate(found)[:count]
