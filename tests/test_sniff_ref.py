"""CPU tests of the sniff stage's reference (_sniff_ref.py): its two forms agree, the batch generator meets the
conditions the GPU tests rely on for the sizes and seeds they use, and the bindings exist."""
import numpy as np
import pytest

import _sniff_ref as S
from orleans_amd import graindispatch as g

LIB_INV = (g.GD_INV_MISS, g.GD_INV_REMOVED, g.GD_INV_KEPT, g.GD_INV_HOST, g.GD_INV_NO_ID)   # the stage's bindings

SIZES = (1, 63, 64, 65, 257, 1000)           # tests/test_gpu_sniff.py: test_random_batches
SEED = 4100


@pytest.mark.parametrize("n", SIZES)
def test_forms_agree_and_conditions_hold(n):
    sc = S.Scene(n, SEED + n)
    for pad in (b"", b"\x01", b"\x01\x02", b"\x01\x02\x03"):
        buf, offs = sc.pack(pad)
        cache = sc.new_cache()
        before = cache.state()
        want = S.sniff_messages(buf, offs, cache)
        inv, after = S.sniff_vectorised(buf, offs, before, sc.act_ids)
        np.testing.assert_array_equal(inv, want["inv"])
        kv, nacc, stats = cache.state()
        assert after[0] == kv and after[1] == nacc and after[2] == stats
        S.check_conditions(sc, want)
        assert (want["ent_ext_len"] >= 0).any()
        for e in range(want["m"]):                           # the strings lie where ent_ext_off says
            x = want["ent_ext"][e]
            if x is not None:
                o = int(want["ent_ext_off"][e])
                assert buf[o:o + len(x)] == x


def test_order_inside_a_batch():
    sc = S.Scene(1, 7)
    cache = sc.new_cache()
    k = sc.key(0)
    good = sc._entry(0, "match")[2][0]
    g0 = cache.state()[2][2]
    assert [S.invalidate_cache_entry(cache, k, a) for a in ((1, 2, 3), good, good)] == \
        [S.INV_KEPT, S.INV_REMOVED, S.INV_MISS]
    assert cache.state()[2][2] == g0 + 2 and k not in cache.state()[0]


def test_the_library_exports_the_stage():
    for name in ("gd_sniff_frames", "gd_sniff_frames_device", "gd_cache_invalidate", "gd_cache_invalidate_device",
                 "gd_sniff_invalidate", "gd_sniff_invalidate_device"):
        assert hasattr(g.lib, name)
    assert LIB_INV == \
        (S.INV_MISS, S.INV_REMOVED, S.INV_KEPT, S.INV_HOST, S.INV_NO_ID)
