"""The compact route (gd_classes_set, gd_route_compact*, gd_route_bucket_compact*): messages given as
(class id, N1) records, results packed as act u32 / silo u16 / status u8.

Every result is compared bit for bit with the oracle (route_batch_np, bucket_stable, the cache model) run on the
expanded 24-B keys (tests/_compact_ref.py), never with the library's own 24-B route.  The device forms write into
buffers with 64 guard bytes (0xA5) behind every output: the u16 and u8 streams must end at n.

The silo-width case: the issue asks for a directory entry with silo 0x10000.  The directory, the cache and the ring
all refuse a silo index above 0xFFFE (their slots hold 16 bits; the test asserts the refusals), so the only silo
values that can be too wide are gd_config's my_silo and seed_silo; the case drives the count through my_silo =
0x10000 and system-target messages instead."""
import ctypes as C

import numpy as np
import pytest

import dircache as co
import oracle as o
import _compact_ref as cr
import _turns_ref as tr

pytestmark = pytest.mark.gpu

TC = o.grain_type_code(o.PING_GRAIN_CLASS)
SILOS = o.bench_silos(8)
GRAIN_TCS = [TC] + [0x700 + k for k in range(9)]          # 10 grain classes: two more than the 8-B index holds
N_GRAIN = len(GRAIN_TCS)
CLS_SYS, CLS_KEYEXT, CLS_BAD = N_GRAIN, N_GRAIN + 1, 200
CLASSES = np.array([o.type_code_data(o.CAT_GRAIN, t) for t in GRAIN_TCS] +
                   [o.type_code_data(o.CAT_SYSTEM_TARGET, 1), o.type_code_data(o.CAT_KEYEXT_GRAIN, TC)], np.uint64)
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 773]            # wave and BLOCK edges, one ragged multi-block size
FORMS = ["u32", "u64", "cls_u32", "cls_u64"]
G = 3000                                                  # grains of class 0; the other classes hold G // 10 each
MY_SILO, SEED_SILO = 2, 6
GUARD = 64


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


def _engine(gd, mode, n_reg_classes, my_silo=MY_SILO, cap=1 << 14, wide_silo=False, **opts):
    """An engine with the class table set and grains of the first n_reg_classes classes registered: class c holds
    N1 = 0 .. G_c - 1 less one in seven; grain 5 of class 0 has several activations; wide_silo: grain 1 of class
    0 sits on silo 0xFFFE (16 silo bits leave the 8-B index room for two classes only)."""
    e = gd.GrainDispatch(device=0, table_capacity=cap, my_silo=my_silo, seed_silo=SEED_SILO, options=opts or None)
    e.ring_set_silos(mode, [(s.ip, s.port, s.gen) for s in SILOS])
    e.classes_set(CLASSES)
    spec = o.ring_spec(SILOS, mode)
    keys = []
    for c in range(n_reg_classes):
        gc = G if c == 0 else G // 10
        ids = np.array([i for i in range(gc) if i % 7 != 3])
        keys.append(o.grain_keys(GRAIN_TCS[c], ids))
    reg = np.concatenate(keys)
    acts = (np.arange(len(reg), dtype=np.uint32) * 3 + 1)
    own = _owner(spec, reg)
    if wide_silo:
        own[1] = 0xFFFE                                  # the widest silo index a directory entry holds
    e.register(reg, acts, own)
    assert reg[4, 1] == 5 and reg[1, 1] == 1
    acts[4] = o.ACT_MULTI
    e.upsert(reg[4:5], acts[4:5], own[4:5])
    return e, spec, _Live(reg, acts, own)


def _owner(spec, k):
    return o.ring_owner_np(spec, o.jenkins_u64x3_np(k[:, 2], k[:, 0], k[:, 1])).astype(np.uint32)


class _Live:
    """The directory as the test believes it: key -> (act, silo)."""

    def __init__(self, keys, acts, silos):
        self.m = {}
        self.put(keys, acts, silos)

    def put(self, keys, acts, silos):
        for k, x, s in zip(np.asarray(keys).tolist(), acts, silos):
            self.m[tuple(k)] = (int(x), int(s))

    def drop(self, keys):
        for k in np.asarray(keys).tolist():
            del self.m[tuple(k)]

    def arrays(self):
        keys = np.array(list(self.m.keys()), np.uint64).reshape(-1, 3)
        vals = np.array(list(self.m.values()), np.uint32).reshape(-1, 2)
        return o.DirectoryArrays(keys, vals[:, 0], vals[:, 1])


def _records(rng, form, n, n_cls_used=N_GRAIN):
    """(cls or None, n1): hits, misses (N1 past the registered range, and the one-in-seven holes), with class
    ids: every grain class, the system-target and the KeyExt class and an out-of-range id; u64: N1 >= 2^32 whose
    low word is a live entry's."""
    wide = form.endswith("u64")
    n1 = rng.integers(0, G + G // 8, size=n).astype(np.uint64 if wide else np.uint32)
    cls = None
    if form.startswith("cls"):
        cls = rng.integers(0, n_cls_used, size=n).astype(np.uint8)
        small = cls > 0
        n1[small] = n1[small] % np.uint64(G // 10 + 40) if wide else n1[small] % np.uint32(G // 10 + 40)
        u = rng.random(n)
        cls[u < 0.04] = CLS_SYS
        cls[(u >= 0.04) & (u < 0.08)] = CLS_KEYEXT
        cls[(u >= 0.08) & (u < 0.12)] = CLS_BAD
        cls[(u >= 0.12) & (u < 0.14)] = len(CLASSES)      # the first id past the table
    if wide and n:
        n1[rng.random(n) < 0.05] += np.uint64(1 << 32)
        n1[n - 1] = np.uint64((1 << 32) + 8)
    if n > 2:
        n1[1], n1[2] = 5, 1                               # the multi-activation grain, the silo 0xFFFE entry
        if cls is not None:
            cls[1] = cls[2] = 0
    return cls, n1


def _dev_call(e, cls, n1, n_act=None, wide=True):
    """The device form over guarded buffers: (status, silo16, act[, perm, offsets], wide count)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(n1)
    w = n1.dtype.itemsize
    up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev) if len(a) else torch.zeros(8, dtype=torch.uint8, device=dev)
    d_cls = None if cls is None else up(cls)
    d_n1 = up(n1)
    sizes = {"act": 4 * n, "silo": 2 * n, "st": n}
    if n_act is not None:
        sizes.update(perm=4 * n, off=4 * (n_act + 2))
    bufs = {k: torch.full((b + GUARD,), 0xA5, dtype=torch.uint8, device=dev) for k, b in sizes.items()}
    d_wide = torch.full((1 + GUARD // 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()                              # the fills ran on torch's stream
    p = lambda t: None if t is None else t.data_ptr()
    if n_act is None:
        e.route_compact_device(p(d_cls), p(d_n1), w, n, p(bufs["act"]), p(bufs["silo"]), p(bufs["st"]),
                               p(d_wide) if wide else None)
    else:
        e.route_bucket_compact_device(p(d_cls), p(d_n1), w, n, n_act, p(bufs["act"]), p(bufs["silo"]), p(bufs["st"]),
                                      p(bufs["perm"]), p(bufs["off"]), p(d_wide) if wide else None)
    e.synchronize()
    host = {k: t.cpu().numpy() for k, t in bufs.items()}
    for k, b in sizes.items():
        assert (host[k][b:] == 0xA5).all(), f"{k}: guard bytes overwritten at n = {n}"
    dw = d_wide.cpu().numpy().view(np.uint32)
    assert (dw[1:] == 0x5A5A5A5A).all()
    out = [host["st"][:n].copy(), host["silo"][:2 * n].copy().view(np.uint16), host["act"][:4 * n].copy().view(np.uint32)]
    if n_act is not None:
        out += [host["perm"][:4 * n].copy().view(np.uint32), host["off"][:4 * (n_act + 2)].copy().view(np.uint32)]
    return out + [int(dw[0]) if wide else None]


def _same(got, want, what=""):
    for name, x, y in zip(("status", "silo16", "act", "perm", "offsets"), got, want):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {name}")


def _check_all(e, rng, spec, d, forms=FORMS, sizes=SIZES, host=True, my_silo=MY_SILO):
    seen = set()
    for form in forms:
        for n in sizes:
            cls, n1 = _records(rng, form, n)
            st, s16, act, wide = cr.expect(CLASSES, cls, n1, spec, d, my_silo, SEED_SILO)
            assert wide == 0
            got = _dev_call(e, cls, n1)
            _same(got[:3], (st, s16, act), f"device {form} n={n}")
            assert got[3] == 0
            if host:
                _same(e.route_compact(cls, n1), (st, s16, act), f"host {form} n={n}")
            seen |= set(st.tolist())
    return seen


EVERY_STATUS = {o.ST_OK, o.ST_MISS, o.ST_SYSTEM_TARGET, o.ST_KEYEXT, o.ST_MULTI_ACT, cr.ST_BAD_CLASS}


@pytest.mark.parametrize("n_reg", [1, 8, 10])
@pytest.mark.parametrize("mode", ["D", "R", "V"])
def test_every_input_form_and_size(gd, mode, n_reg):
    """Every input form at every size, device and host forms, in each ring mode, over a directory of one class
    (the pure 8-B index), eight (the 8-B index full) and ten (keys of two classes fall back to the table)."""
    rng = np.random.default_rng(100 + n_reg)
    e, spec, live = _engine(gd, mode, n_reg, probe=4)
    seen = _check_all(e, rng, spec, live.arrays())
    assert seen == EVERY_STATUS
    e.close()


@pytest.mark.parametrize("n_reg", [1, 10])
@pytest.mark.parametrize("how", ["probe0", "probe2", "probe3", "probe4", "pin0", "pin1", "pin2", "pin3"])
def test_every_probe_form(gd, how, n_reg):
    """The probe forms of the 24-B route, forced by GD_OPT_PROBE (0 the directory, 2 / 3 the 16-B index in group
    / slot reads, 4 the 8-B index: pure with one class, with the directory behind it with ten) and, measured
    mode, by pinning GD_TUNE_PROBE_KEYS, which the compact route follows."""
    rng = np.random.default_rng(200 + n_reg)
    if how.startswith("probe"):
        e, spec, live = _engine(gd, "D", n_reg, probe=int(how[-1]))
    else:
        # measured mode builds the indexes for a launch of at least capacity / 16 messages: 773 >= 512, first
        e, spec, live = _engine(gd, "D", n_reg, cap=1 << 13, probe=1)
        e.tune_set("probe_keys", int(how[-1]))
    e.set_kernel_timing(True)
    for _ in range(2):
        seen = _check_all(e, rng, spec, live.arrays(), sizes=[773, 1, 257], host=False)
    assert seen == EVERY_STATUS
    kt = e.kernel_times()
    assert kt["k_route_compact"][0] == 2 * 4 * 3 and "k_route" not in kt
    e.close()


def test_direct_table_form(gd):
    """One class, dense N1s, the directory quiet: the second route after a read-back builds the direct table and
    the compact route reads it (k_cxd_build launched by a compact route; no 24-B route ran on the handle)."""
    rng = np.random.default_rng(300)
    e, spec, live = _engine(gd, "D", 1, probe=4)
    e.set_kernel_timing(True)
    d = live.arrays()
    e.stats()
    for k in range(3):
        _check_all(e, rng, spec, d, forms=["u32"], sizes=[773], host=False)
        assert e.kernel_times().get("k_cxd_build", (0, 0.0))[0] == (0 if k == 0 else 1)
    seen = _check_all(e, rng, spec, d)
    assert seen == EVERY_STATUS
    assert e.kernel_times()["k_cxd_build"][0] == 1 and "k_route" not in e.kernel_times()
    e.close()


def test_churn_and_rehash_between_routes(gd):
    """Register / unregister / upsert batches between compact routes (the indexes re-projected by the batches),
    then a rehash (the indexes rebuilt)."""
    rng = np.random.default_rng(400)
    e, spec, live = _engine(gd, "D", 10, probe=4)
    sizes = [65, 773]
    _check_all(e, rng, spec, live.arrays(), sizes=sizes, host=False)
    for step in range(3):
        new = o.grain_keys(GRAIN_TCS[step], np.arange(G + 10 + 40 * step, G + 40 + 40 * step))
        nacts, nown = np.arange(len(new), dtype=np.uint32) + 50000 + step, _owner(spec, new)
        assert e.register(new, nacts, nown)[2].all()
        live.put(new, nacts, nown)
        _check_all(e, rng, spec, live.arrays(), sizes=sizes, host=False)
        gone = new[::3]
        assert e.unregister(gone, nacts[::3]).all()
        live.drop(gone)
        _check_all(e, rng, spec, live.arrays(), sizes=sizes, host=False)
        up = o.grain_keys(GRAIN_TCS[0], rng.choice(np.arange(8, 200), size=40, replace=False))
        uacts, uown = rng.integers(0, 1 << 20, size=40).astype(np.uint32), ((_owner(spec, up) + 1) % 8).astype(np.uint32)
        e.upsert(up, uacts, uown)
        live.put(up, uacts, uown)
        seen = _check_all(e, rng, spec, live.arrays(), sizes=sizes, host=False)
    assert seen == EVERY_STATUS
    e.rehash(1 << 15)
    assert e.stats()["table_capacity"] == 1 << 15
    for _ in range(2):
        assert _check_all(e, rng, spec, live.arrays(), sizes=sizes) == EVERY_STATUS
    e.close()


def test_local_lookup_mode(gd):
    """LocalLookup (cache) mode: the same routes and, afterwards, the same cache entries, generations and
    statistics as the oracle's cache model gives for the expanded keys; an out-of-range class touches nothing."""
    rng = np.random.default_rng(500)
    spec = o.ring_spec(SILOS, "D")
    local, valid = {2, 5}, set(range(7))
    reg = o.grain_keys(TC, np.arange(G))
    owner = _owner(spec, reg)
    mine = np.nonzero(np.isin(owner, list(local)))[0]
    mine = mine[mine % 5 != 0]
    e = gd.GrainDispatch(device=0, table_capacity=1 << 13, my_silo=MY_SILO, seed_silo=SEED_SILO)
    e.ring_set_silos("D", [(s.ip, s.port, s.gen) for s in SILOS])
    e.classes_set(CLASSES)
    e.register(reg[mine], mine.astype(np.uint32), owner[mine])
    dirmap = {tuple(int(x) for x in reg[i]): (int(i), int(owner[i])) for i in mine}
    M = 500
    e.cache_configure(M, sorted(local), 8, sorted(valid))
    oc = co.DirectoryCacheOracle(M)
    remote = np.nonzero(~np.isin(owner, list(local)))[0]
    empty = o.DirectoryArrays(np.zeros((0, 3), np.uint64), [], [])
    for rnd, (form, n, device) in enumerate([("u32", 773, True), ("cls_u64", 773, False), ("cls_u32", 257, True),
                                              ("u64", 65, False), ("cls_u32", 1, True)]):
        add = rng.choice(remote, size=300)
        a_act, a_silo = (add + 100000).astype(np.uint32), rng.integers(0, 8, size=300).astype(np.uint32)
        a_ver = rng.integers(0, 50, size=300).astype(np.int32)
        e.cache_add(reg[add], a_act, a_silo, a_ver)
        for i, gi in enumerate(add):
            oc.add_or_update(tuple(int(x) for x in reg[gi]), int(a_act[i]), int(a_silo[i]), int(a_ver[i]))
        cls, n1 = _records(rng, form, n, n_cls_used=2)
        keys = cr.expand(CLASSES, cls, n1)
        w_st, w_silo, w_act, w_owner, _ = o.route_batch_np(keys, spec, empty, my_silo=MY_SILO, seed_silo=SEED_SILO)
        isbad = cr.bad(CLASSES, cls, n)
        lookup = (w_st == o.ST_MISS) & ~isbad
        kt = [tuple(int(x) for x in r) for r in keys]
        want = co.local_lookup_route(kt, [int(w_owner[i]) if lookup[i] else None for i in range(n)], local, valid,
                                     dirmap.get, oc)
        for i, (ws, wsi, wa) in enumerate(want):
            if ws is not None:
                w_st[i], w_silo[i] = (o.ST_OK if ws == "OK" else o.ST_MISS), wsi
                w_act[i] = o.M32 if wa is None else wa
        st, s16, act, wide = cr.pack(CLASSES, cls, w_st, w_silo, w_act)
        got = _dev_call(e, cls, n1) if device else list(e.route_compact(cls, n1)) + [0]
        _same(got[:3], (st, s16, act), f"round {rnd}")
        assert got[3] == 0 and wide == 0
        assert e.cache_entries() == oc.key_values()
        cs = e.cache_stats()
        assert cs["next_generation"] == oc.next_generation
        assert cs["accesses"] == oc.num_accesses and cs["hits"] == oc.num_hits
    assert oc.num_hits > 30
    e.close()


@pytest.mark.parametrize("n_act", [1, 40, G * 3 + 2])
def test_bucket_forms(gd, n_act):
    """perm / offsets equal to bucket_stable of the oracle's acts: n_act = 1, n_act below most acts (the trailing
    bucket takes them with the misses) and n_act above every act; host and device forms, n = 0 included."""
    rng = np.random.default_rng(600 + n_act)
    e, spec, live = _engine(gd, "V", 10, probe=4)
    d = live.arrays()
    for form in FORMS:
        for n in (0, 1, 257, 773):
            cls, n1 = _records(rng, form, n)
            st, s16, act, _ = cr.expect(CLASSES, cls, n1, spec, d, MY_SILO, SEED_SILO)
            wp, wo = o.bucket_stable(act, n_act)
            got = _dev_call(e, cls, n1, n_act=n_act)
            _same(got[:5], (st, s16, act, wp, wo), f"device {form} n={n}")
            _same(e.route_bucket_compact(cls, n1, n_act), (st, s16, act, wp, wo), f"host {form} n={n}")
    if n_act == 40:
        assert wo[n_act + 1] - wo[n_act] > 700            # the trailing bucket is in use
    e.close()


@pytest.mark.parametrize("pinned", [True, False])
def test_host_pipeline(gd, pinned):
    """GD_OPT_HOST_CHUNK = 64 and n = 128 (two chunks exactly), 129 (a one-message tail), 323 (a ragged tail), from
    gd_host_alloc'd buffers (the three-stream chunk pipeline) and from pageable ones (the staging helper)."""
    rng = np.random.default_rng(700)
    e, spec, live = _engine(gd, "D", 10, probe=4, host_chunk=64)
    d = live.arrays()
    bufs = []

    def arr(n, dt):
        if not pinned:
            return np.zeros(n, dt)
        p = C.c_void_p()
        nb = max(n, 1) * np.dtype(dt).itemsize
        assert gd.lib.gd_host_alloc(nb, C.byref(p)) == 0
        bufs.append(p)
        return np.ctypeslib.as_array((C.c_uint8 * nb).from_address(p.value)).view(dt)[:n]

    n_act = 2000
    for form in FORMS:
        for n in (128, 129, 323):
            cls, n1 = _records(rng, form, n)
            st, s16, act, _ = cr.expect(CLASSES, cls, n1, spec, d, MY_SILO, SEED_SILO)
            wp, wo = o.bucket_stable(act, n_act)
            h_n1 = arr(n, n1.dtype)
            h_n1[:] = n1
            h_cls = None
            if cls is not None:
                h_cls = arr(n, np.uint8)
                h_cls[:] = cls
            o_act, o_s16, o_st, o_perm = arr(n, np.uint32), arr(n, np.uint16), arr(n, np.uint8), arr(n, np.uint32)
            o_off = arr(n_act + 2, np.uint32)
            pc = None if h_cls is None else h_cls.ctypes.data
            for _ in range(2):                              # the streams and events are reused
                o_act[:], o_s16[:], o_st[:], o_perm[:], o_off[:] = 7, 7, 7, 7, 7
                e._c(gd.lib.gd_route_bucket_compact(e.h, pc, h_n1.ctypes.data, n1.dtype.itemsize, n, n_act,
                                                    o_act.ctypes.data, o_s16.ctypes.data, o_st.ctypes.data,
                                                    o_perm.ctypes.data, o_off.ctypes.data))
                _same((o_st, o_s16, o_act, o_perm, o_off), (st, s16, act, wp, wo), f"bucket {form} n={n}")
                o_act[:], o_s16[:], o_st[:] = 7, 7, 7
                e._c(gd.lib.gd_route_compact(e.h, pc, h_n1.ctypes.data, n1.dtype.itemsize, n, o_act.ctypes.data,
                                             o_s16.ctypes.data, o_st.ctypes.data))
                _same((o_st, o_s16, o_act), (st, s16, act), f"route {form} n={n}")
    e.close()
    for p in bufs:
        assert gd.lib.gd_host_free(p) == 0


def test_silo_width(gd):
    """Silo 0xFFFE round-trips through a directory entry.  No directory entry, cache entry or ring owner can hold
    0x10000 (asserted); my_silo = 0x10000 reaches the output for system targets: the device form's d_wide is
    their count, the host form stores GD_NO_SILO16, brings every result down and returns GD_EINVAL."""
    rng = np.random.default_rng(800)
    e, spec, live = _engine(gd, "D", 1, my_silo=0x10000, wide_silo=True, probe=4)
    d = live.arrays()
    n1 = np.array([1, 2, 1], np.uint32)                    # N1 = 1: the entry registered with silo 0xFFFE
    st, s16, act, wide = cr.expect(CLASSES, None, n1, spec, d, 0x10000, SEED_SILO)
    assert s16.tolist()[::2] == [0xFFFE, 0xFFFE] and st.tolist() == [0, 0, 0] and wide == 0
    _same(e.route_compact(None, n1), (st, s16, act))
    for refuse in (lambda: e.upsert(o.grain_keys(TC, [9]), [1], [0x10000]),
                   lambda: e.register(o.grain_keys(TC, [G + 9]), [1], [0x10000]),
                   lambda: e.ring_set("D", [1, 2], [0, 0x10000])):
        with pytest.raises(gd.GrainDispatchError):
            refuse()
    _same(e.route_compact(None, n1), (st, s16, act))
    for n in (1, 65, 773):
        cls, n1 = _records(rng, "cls_u32", n)
        cls[::3] = CLS_SYS
        st, s16, act, wide = cr.expect(CLASSES, cls, n1, spec, d, 0x10000, SEED_SILO)
        assert wide == int((cls == CLS_SYS).sum()) > 0 and (s16[cls == CLS_SYS] == 0xFFFF).all()
        got = _dev_call(e, cls, n1)
        _same(got[:3], (st, s16, act))
        assert got[3] == wide
        assert _dev_call(e, cls, n1, wide=False)[3] is None            # d_wide NULL is allowed
        assert _dev_call(e, cls, n1, n_act=50)[5] == wide
        o_act, o_s16, o_st = np.full(n, 7, np.uint32), np.full(n, 7, np.uint16), np.full(n, 7, np.uint8)
        rc = gd.lib.gd_route_compact(e.h, cls.ctypes.data, n1.ctypes.data, 4, n, o_act.ctypes.data, o_s16.ctypes.data,
                                     o_st.ctypes.data)
        assert rc == gd.GD_EINVAL and b"16 bits" in gd.lib.gd_last_error(e.h)
        _same((o_st, o_s16, o_act), (st, s16, act))
        perm, off = np.zeros(n, np.uint32), np.zeros(52, np.uint32)
        rc = gd.lib.gd_route_bucket_compact(e.h, cls.ctypes.data, n1.ctypes.data, 4, n, 50, o_act.ctypes.data,
                                            o_s16.ctypes.data, o_st.ctypes.data, perm.ctypes.data, off.ctypes.data)
        assert rc == gd.GD_EINVAL
        wp, wo = o.bucket_stable(act, 50)
        _same((o_st, o_s16, o_act, perm, off), (st, s16, act, wp, wo))
    e.close()


def test_error_returns_and_class_table(gd):
    lib = gd.lib
    e = gd.GrainDispatch(device=0, table_capacity=1 << 10)
    e.ring_set_silos("D", [(s.ip, s.port, s.gen) for s in SILOS])
    n = 5
    n1, cls = np.arange(n, dtype=np.uint32), np.zeros(n, np.uint8)
    act, s16, st = np.zeros(n, np.uint32), np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    perm, off = np.zeros(n, np.uint32), np.full(12, 9, np.uint32)
    P = lambda a: a.ctypes.data
    host = lambda c, k, w, m=n: lib.gd_route_compact(e.h, c, k, w, m, P(act), P(s16), P(st))
    assert e.classes_get().tolist() == []
    assert host(P(cls), P(n1), 4) == gd.GD_ESTATE            # no class table, cls given
    assert host(None, P(n1), 4) == gd.GD_ESTATE              # class 0 is absent
    assert lib.gd_route_compact_device(e.h, None, P(n1), 4, n, P(act), P(s16), P(st), None) == gd.GD_ESTATE
    assert lib.gd_route_bucket_compact(e.h, None, P(n1), 4, n, 10, P(act), P(s16), P(st), P(perm), P(off)) == gd.GD_ESTATE
    assert lib.gd_classes_set(e.h, P(CLASSES), 257) == gd.GD_EINVAL
    assert lib.gd_classes_set(e.h, None, 3) == gd.GD_EINVAL
    assert lib.gd_classes_set(None, P(CLASSES), 3) == gd.GD_EINVAL
    e.classes_set(CLASSES)
    assert e.classes_get().tolist() == CLASSES.tolist()
    full = np.arange(256, dtype=np.uint64) + np.uint64(o.type_code_data(o.CAT_GRAIN, 0))
    e.classes_set(full)                                       # 256 classes: the whole LDS table
    assert e.classes_get().tolist() == full.tolist()
    e.classes_set(CLASSES[:2])                                # replaces
    assert e.classes_get().tolist() == CLASSES[:2].tolist()
    for w in (0, 2, 3, 5, 16):
        assert host(P(cls), P(n1), w) == gd.GD_EINVAL
        assert host(None, None, w, 0) == gd.GD_EINVAL         # the width is checked at n = 0 too
        assert lib.gd_route_compact_device(e.h, None, P(n1), w, n, P(act), P(s16), P(st), None) == gd.GD_EINVAL
    assert host(None, None, 4) == gd.GD_EINVAL
    assert lib.gd_route_compact(e.h, None, P(n1), 4, n, None, P(s16), P(st)) == gd.GD_EINVAL
    assert lib.gd_route_compact(e.h, None, P(n1), 4, n, P(act), None, P(st)) == gd.GD_EINVAL
    assert lib.gd_route_compact(e.h, None, P(n1), 4, n, P(act), P(s16), None) == gd.GD_EINVAL
    assert lib.gd_route_compact(None, None, P(n1), 4, n, P(act), P(s16), P(st)) == gd.GD_EINVAL
    assert lib.gd_route_bucket_compact(e.h, None, P(n1), 4, n, 10, P(act), P(s16), P(st), None, P(off)) == gd.GD_EINVAL
    assert lib.gd_route_bucket_compact(e.h, None, P(n1), 4, n, 10, P(act), P(s16), P(st), P(perm), None) == gd.GD_EINVAL
    assert lib.gd_route_bucket_compact_device(e.h, None, P(n1), 4, n, 10, P(act), P(s16), P(st), P(perm), None,
                                              None) == gd.GD_EINVAL
    # n = 0 is GD_OK, and the bucket forms write the offsets
    assert host(None, None, 4, 0) == gd.GD_OK and host(None, None, 8, 0) == gd.GD_OK
    assert lib.gd_route_bucket_compact(e.h, None, None, 4, 0, 10, None, None, None, None, P(off)) == gd.GD_OK
    assert off.tolist() == [0] * 12
    e.classes_set([])                                         # n = 0 clears the table
    assert e.classes_get().tolist() == [] and host(None, P(n1), 4) == gd.GD_ESTATE
    assert host(None, None, 4, 0) == gd.GD_OK
    assert gd.lib.gd_abi_version() == 1
    e.close()


def test_composition_with_turns(gd):
    """gd_route_bucket_compact_device's act, left on the device, is gd_turns_device's ctx: the turns are what the
    reference gives for the oracle's acts of the expanded keys (activation index = context index)."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(900)
    e = gd.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=MY_SILO)
    e.ring_set_silos("D", [(s.ip, s.port, s.gen) for s in SILOS])
    e.classes_set(CLASSES)
    spec = o.ring_spec(SILOS, "D")
    n_ctx, n = 300, 1500
    reg = np.concatenate([o.grain_keys(GRAIN_TCS[0], np.arange(200)), o.grain_keys(GRAIN_TCS[1], np.arange(100))])
    acts = rng.permutation(n_ctx).astype(np.uint32)
    e.register(reg, acts, _owner(spec, reg))
    d = o.DirectoryArrays(reg, acts, _owner(spec, reg))
    cls = rng.integers(0, 2, size=n).astype(np.uint8)
    n1 = np.where(cls == 0, rng.integers(0, 230, size=n), rng.integers(0, 120, size=n)).astype(np.uint32)
    cls[::50] = CLS_BAD
    st, s16, act, _ = cr.expect(CLASSES, cls, n1, spec, d, MY_SILO)
    assert (st == o.ST_OK).sum() > 1000 and (st == o.ST_MISS).sum() > 100
    fl, nr = tr.context_state(rng, n_ctx)
    rc = rng.integers(0, 12, n_ctx).astype(np.uint32)
    mf = (rng.integers(0, 2, n) * tr.MSG_READ_ONLY).astype(np.uint8)
    b = tr.Batch(act, n_ctx, fl, nr, rc, msg_flags=mf, hard_limit=8, hard_limit_sw=4)
    want = tr.turns_np(b)
    up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)
    z = lambda m, dt: torch.zeros(max(m, 1), dtype=dt, device=dev)
    d_cls, d_n1, d_mf = up(cls), up(n1), up(mf)
    d_fl, d_nr, d_rc = up(fl), up(nr), up(rc)
    d_act, d_s16, d_st = z(n, torch.int32), z(n, torch.int16), z(n, torch.uint8)
    d_perm, d_off = z(n, torch.int32), z(n_ctx + 2, torch.int32)
    d_turn, d_nro, d_run = z(n, torch.uint8), z(n_ctx, torch.int32), z(n_ctx, torch.int32)
    d_start, d_nstart = z(n, torch.int32), z(1, torch.int32)
    d_wperm, d_woff = z(n, torch.int32), z(n_ctx + 2, torch.int32)
    torch.cuda.synchronize()
    e.route_bucket_compact_device(d_cls.data_ptr(), d_n1.data_ptr(), 4, n, n_ctx, d_act.data_ptr(), d_s16.data_ptr(),
                                  d_st.data_ptr(), d_perm.data_ptr(), d_off.data_ptr())
    state = gd.gd_turn_state(d_fl.data_ptr(), d_nr.data_ptr(), d_rc.data_ptr(), 8, 4, 2, 0)
    e.turns_device(d_act.data_ptr(), None, None, None, None, d_mf.data_ptr(), None, None, n, n_ctx, state,
                   d_turn.data_ptr(), d_nro.data_ptr(), d_run.data_ptr(), d_start.data_ptr(), d_nstart.data_ptr(),
                   d_wperm.data_ptr(), d_woff.data_ptr())
    e.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(u32(d_act), act)
    wp, wo = o.bucket_stable(act, n_ctx)
    np.testing.assert_array_equal(u32(d_perm), wp)
    np.testing.assert_array_equal(u32(d_off), wo)
    turn, nro, run, start, wperm, woff = want
    np.testing.assert_array_equal(d_turn.cpu().numpy(), turn)
    np.testing.assert_array_equal(u32(d_nro), nro)
    np.testing.assert_array_equal(u32(d_run), run)
    ns = int(u32(d_nstart)[0])
    assert ns == len(start)
    np.testing.assert_array_equal(u32(d_start)[:ns], start)
    np.testing.assert_array_equal(u32(d_wperm), wperm)
    np.testing.assert_array_equal(u32(d_woff), woff)
    assert {tr.TURN_START, tr.TURN_WAIT, tr.TURN_NONE} <= set(turn.tolist())
    e.close()
