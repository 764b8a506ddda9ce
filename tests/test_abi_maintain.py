"""The maintainer's entry points through ctypes: the symbols exist, null arguments are refused, and the size-query
forms work."""
import ctypes as C

import numpy as np
import pytest

import oracle as o

pytestmark = pytest.mark.gpu

SYMBOLS = ["gd_cache_maintain_configure", "gd_cache_clock_set", "gd_cache_entries_age", "gd_cache_scan_device",
           "gd_cache_scan", "gd_cache_scan_fetch", "gd_dir_lookup_many_device", "gd_dir_lookup_many",
           "gd_cache_refresh_apply_device", "gd_cache_refresh_apply"]


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


def test_symbols_and_arguments(gd):
    lib = C.CDLL(gd.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    L = gd.lib
    e = gd.GrainDispatch(device=0, table_capacity=1024)
    h = e.h
    n64, n32a, n32b = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    counts = np.zeros(5, dtype=np.uint64)
    # no cache configured: GD_ESTATE; a null handle: GD_EINVAL
    assert L.gd_cache_scan(h, 0, counts.ctypes.data, C.byref(n32a), C.byref(n32b), C.byref(n64)) == gd.GD_ESTATE
    assert L.gd_cache_clock_set(None, 0) == gd.GD_EINVAL
    assert L.gd_dir_lookup_many(None, None, None, 0, None, None, None) == gd.GD_EINVAL
    e.ring_set_silos("D", [(s.ip, s.port, s.gen) for s in o.bench_silos(8)])
    e.cache_configure(8, [], 8)
    keys = o.grain_keys(o.grain_type_code(o.PING_GRAIN_CLASS), np.arange(3, dtype=np.int64))
    e.cache_add(keys, [1, 2, 3], [1, 2, 3], [7, 8, 9])
    # null arguments
    assert L.gd_cache_entries_age(h, None, None, None, 0, None) == gd.GD_EINVAL
    assert L.gd_cache_scan(h, 0, None, C.byref(n32a), C.byref(n32b), C.byref(n64)) == gd.GD_EINVAL
    assert L.gd_cache_scan_device(h, 0, None) == gd.GD_EINVAL
    assert L.gd_dir_lookup_many(h, None, None, 3, None, None, None) == gd.GD_EINVAL
    assert L.gd_dir_lookup_many_device(h, None, None, 3, None, None, None) == gd.GD_EINVAL
    assert L.gd_cache_refresh_apply(h, 0, None, None, None, None, None, 3, None) == gd.GD_EINVAL
    assert L.gd_cache_refresh_apply_device(h, 0, None, None, None, 3, None) == gd.GD_EINVAL
    kind = np.array([gd.GD_LM_UPDATED] * 3, dtype=np.uint8)
    assert L.gd_cache_refresh_apply(h, 0, keys.ctypes.data, None, kind.ctypes.data, None, None, 3, None) == gd.GD_EINVAL
    assert L.gd_cache_scan_fetch(h, None, None, None, None, None, None, None, None, 0, 0, 0) == gd.GD_ESTATE   # no scan held
    # size queries
    assert L.gd_cache_entries_age(h, None, None, None, 0, C.byref(n64)) == gd.GD_OK and n64.value == 3
    e.cache_lookup(keys[:2])
    now = 31 * 10_000_000
    assert L.gd_cache_scan(h, now, counts.ctypes.data, C.byref(n32a), C.byref(n32b), C.byref(n64)) == gd.GD_OK
    assert list(counts) == [3, 0, 0, 1, 2] and n32b.value == 2 and n64.value == 0 and 1 <= n32a.value <= 2
    small = np.zeros(1, dtype=np.int32)
    assert L.gd_cache_scan_fetch(h, None, None, None, small.ctypes.data, None, None, None, None, 0, 1, 0) == gd.GD_EINVAL
    et = np.zeros(2, dtype=np.int32)
    assert L.gd_cache_scan_fetch(h, None, None, None, et.ctypes.data, None, None, None, None, 0, 2, 0) == gd.GD_OK
    assert sorted(et) == [7, 8]
    r = gd.gd_cache_scan_result()
    assert L.gd_cache_scan_device(h, now, C.byref(r)) == gd.GD_OK
    assert list(r.counts) == [2, 0, 0, 2, 0] and r.n == 0 and r.n_owners == 0
    e.close()
