"""The compact route's reference (gd_route_compact*): records (class id, N1) expanded into the
24-B keys the oracle routes, and the packed results.  Constants mirror include/graindispatch.h."""
import numpy as np

import oracle as o

NO_SILO16 = 0xFFFF
ST_BAD_CLASS = 8


def expand(classes, cls, n1):
    """(n, 3) u64 keys {0, n1[i], classes[cls[i]]}; cls None: class 0.  An out-of-range class id gets
    TypeCodeData 0 (see `bad`): its key is never looked at."""
    n1 = np.asarray(n1).astype(np.uint64)
    classes = np.asarray(classes, dtype=np.uint64)
    c = np.zeros(len(n1), np.int64) if cls is None else np.asarray(cls).astype(np.int64)
    keys = np.zeros((len(n1), 3), np.uint64)
    keys[:, 1] = n1
    ok = c < len(classes)
    keys[ok, 2] = classes[c[ok]]
    return keys


def bad(classes, cls, n):
    return np.zeros(n, bool) if cls is None else np.asarray(cls).astype(np.int64) >= len(classes)


def pack_silo16(silo):
    """(silo16 u16[n], count of silos that do not fit): GD_NO_SILO -> 0xFFFF, 0..0xFFFE pass, 0xFFFF..0xFFFFFFFE
    are stored as 0xFFFF and counted."""
    s = np.asarray(silo, dtype=np.uint32)
    wide = (s >= NO_SILO16) & (s != o.M32)
    return np.where(s >= NO_SILO16, NO_SILO16, s).astype(np.uint16), int(wide.sum())


def pack(classes, cls, st, silo, act):
    """The oracle's 24-B routes of the expanded keys as the compact calls return them."""
    b = bad(classes, cls, len(st))
    st, silo, act = st.copy(), silo.copy(), act.copy()
    st[b], silo[b], act[b] = ST_BAD_CLASS, o.M32, o.M32
    s16, wide = pack_silo16(silo)
    return st.astype(np.uint8), s16, act.astype(np.uint32), wide


def expect(classes, cls, n1, spec, d, my_silo=0, seed_silo=o.M32):
    """(status u8, silo16 u16, act u32, wide count)."""
    st, silo, act, _, _ = o.route_batch_np(expand(classes, cls, n1), spec, d, my_silo=my_silo, seed_silo=seed_silo)
    return pack(classes, cls, st, silo, act)
