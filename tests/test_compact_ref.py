"""CPU tests of the compact route's reference helpers (tests/_compact_ref.py): the record-to-key expansion the
GPU tests feed the oracle with, and the packed-silo rule."""
import numpy as np

import oracle as o
import _compact_ref as cr

TC = o.grain_type_code(o.PING_GRAIN_CLASS)


def test_expand_reproduces_grain_keys():
    rng = np.random.default_rng(3)
    ids = np.concatenate([rng.integers(0, 1 << 31, size=500), [0, 1, (1 << 32) - 1]])
    want = o.grain_keys(TC, ids)
    tcd = o.type_code_data(o.CAT_GRAIN, TC)
    np.testing.assert_array_equal(cr.expand([tcd], None, ids.astype(np.uint32)), want)      # u32 N1s, cls NULL
    np.testing.assert_array_equal(cr.expand([tcd], None, ids.astype(np.uint64)), want)
    other = o.type_code_data(o.CAT_GRAIN, 0x777)
    cls = rng.integers(0, 2, size=len(ids)).astype(np.uint8)
    got = cr.expand([other, tcd], cls, ids)
    np.testing.assert_array_equal(got[cls == 1], want[cls == 1])
    np.testing.assert_array_equal(got[cls == 0], o.grain_keys(0x777, ids[cls == 0]))
    big = np.array([1 << 32, (1 << 63) + 5], np.uint64)                                      # zero-extended u64
    np.testing.assert_array_equal(cr.expand([tcd], None, big), o.grain_keys(TC, big.view(np.int64)))
    assert (cr.expand([tcd], None, ids)[:, 0] == 0).all()


def test_bad_class_and_pack():
    tcd = o.type_code_data(o.CAT_GRAIN, TC)
    cls = np.array([0, 1, 2, 255], np.uint8)
    assert cr.bad([tcd, tcd], cls, 4).tolist() == [False, False, True, True]
    assert not cr.bad([tcd], None, 3).any()
    st, s16, act, wide = cr.pack([tcd, tcd], cls, np.zeros(4, np.uint8), np.array([3, 4, 5, 6], np.uint32),
                                 np.array([7, 8, 9, 10], np.uint32))
    assert st.tolist() == [0, 0, cr.ST_BAD_CLASS, cr.ST_BAD_CLASS]
    assert s16.tolist() == [3, 4, 0xFFFF, 0xFFFF] and act.tolist() == [7, 8, o.M32, o.M32] and wide == 0


def test_packed_silo_rule():
    s16, wide = cr.pack_silo16(np.array([0, 7, 0xFFFE, 0xFFFF, 0x10000, 0xFFFFFFFE, o.M32], np.uint32))
    assert s16.dtype == np.uint16
    assert s16.tolist() == [0, 7, 0xFFFE, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF]
    assert wide == 3                                  # 0xFFFF, 0x10000, 0xFFFFFFFE; GD_NO_SILO is not counted
    assert cr.pack_silo16(np.array([o.M32], np.uint32)) == (np.array([0xFFFF], np.uint16), 0)
    assert cr.pack_silo16(np.array([0xFFFE], np.uint32))[1] == 0
    assert cr.pack_silo16(np.array([0xFFFF], np.uint32))[1] == 1
