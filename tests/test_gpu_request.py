"""GPU parity for the request writer (gd_request_*): CreateMessage + SendRequestMessage +
SetTargetPlacement + Message.Serialize for a batch, bit for bit against the reference (_request_ref.py): the status
of every message, out_off, and every output byte; and no byte outside the output is written.

Every device run goes into a buffer pre-filled with 0xA5 that has 64 spare bytes: the bytes before the output and
at or past out_off[n] must still be 0xA5 (_dev)."""
import numpy as np
import pytest

import _request_ref as R
import _respond_ref as RSP
import _sendq_ref as SQ

pytestmark = pytest.mark.gpu

TILE = 16384                                     # k_req_write's output bytes a workgroup (gd_frameout.h)
T = R.tables()
ROUTE_NAMES = ("silo", "act", "status", "placed", "new_type")


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


def _configure(e, t=T):
    e.encode_configure(R.SILO_TUPLES, t.types)
    e.request_configure(t.strings)
    e.activation_ids_set(np.arange(len(t.act_ids)), t.act_ids)


@pytest.fixture(scope="module")
def eng(gd):
    e = gd.GrainDispatch(device=0, table_capacity=1 << 12, my_silo=T.my_silo)
    _configure(e)
    yield e
    e.close()


class _DevBatch:
    """A reference batch on the device: the dict request_frames_device takes, and the tensors it points at."""

    def __init__(self, gd, b, drop=()):
        import torch
        dev = torch.device("cuda:0")
        self.keep = []

        def up(a, dt, tt):
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt)).view(tt).copy()).to(dev)
            self.keep.append(t)
            return t.data_ptr()

        n = len(b["target"])
        d = {"id_base": int(b["id_base"]), "ttl_ticks": int(b["ttl_ticks"])}
        d["target"] = up(b["target"] if n else np.zeros((1, 3)), np.uint64, np.int64)
        d["sender_grain"] = up(b["sender_grain"] if n else np.zeros((1, 3)), np.uint64, np.int64)
        d["sender_act"] = up(b["sender_act"] if n else [0], np.uint32, np.int32)
        for k, dt, tt in (("options", np.uint8, np.uint8), ("generic", np.uint32, np.int32), ("debug", np.uint32, np.int32)):
            if b.get(k) is not None and k not in drop:
                d[k] = up(b[k] if n else [0], dt, tt)
        for k in ("target_ext", "sender_ext"):
            if b.get(k) is not None and k not in drop:
                x = gd.KeyExtBatch(b[k])
                d[k] = (up(x.blob, np.uint8, np.uint8), up(x.offset if n else [0], np.uint64, np.int64),
                        up(x.length if n else [0], np.int32, np.int32), int(x.struct.bytes_len))
        if b.get("body") is not None and "body" not in drop:
            d["body"] = up(np.frombuffer(b["body"] or b"\0", np.uint8), np.uint8, np.uint8)
            d["body_off"] = up(b["body_off"], np.uint64, np.int64)
        self.d, self.n, self.up = d, n, up


def _without(b, drop):
    return {k: v for k, v in b.items() if k not in drop and not (k == "body_off" and "body" in drop)}


def _dev(gd, e, b, route=None, order=None, lead=0, out_cap=None, drop=()):
    """gd_request_frames_device on torch buffers.  Returns (out bytes, out_off, req_status)."""
    import torch
    dev = torch.device("cuda:0")
    db = _DevBatch(gd, b, drop)
    n = db.n
    r = {}
    if route is not None:
        dts = {"silo": (np.uint32, np.int32), "act": (np.uint32, np.int32), "status": (np.uint8, np.uint8),
               "placed": (np.uint8, np.uint8), "new_type": (np.uint32, np.int32)}
        r = {k: db.up(route[k] if n else [0], *dts[k]) for k in ROUTE_NAMES if route.get(k) is not None}
    d_od = None if order is None else db.up(order, np.uint32, np.int32)
    nbody = len(b["body"]) if b.get("body") is not None else 0
    cap = nbody + n * 1400 if out_cap is None else out_cap
    room = torch.full((lead + cap + 64 + 16,), 0xA5, dtype=torch.uint8, device=dev)
    base = (-room.data_ptr()) % 16 + lead                          # out pointer = 16-B boundary + lead
    d_out_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    e.request_frames_device(db.d, n, r.get("silo"), r.get("act"), r.get("status"), r.get("placed"), r.get("new_type"),
                            d_od, room.data_ptr() + base, cap, d_out_off.data_ptr(), d_st.data_ptr())
    err = None
    try:
        e.synchronize()
    except Exception as ex:                                        # GD_EFULL surfaces here; the caller checks
        err = ex
    whole = room.cpu().numpy()
    out_off = d_out_off.cpu().numpy().view(np.uint64)
    total = int(out_off[n])
    assert (whole[:base] == 0xA5).all(), "bytes before the output were written"
    keep = base + (total if err is None else 0)
    assert (whole[keep:] == 0xA5).all(), "bytes at or past out_off[n] were written"
    if err is not None:
        err.out_off = out_off
        raise err
    return whole[base:base + total].tobytes(), out_off, d_st.cpu().numpy()[:n]


def _same(got, want):
    out, off, st = got[:3]
    wout, woff, wst = want
    np.testing.assert_array_equal(st, wst, err_msg="req_status")
    np.testing.assert_array_equal(off, woff, err_msg="out_off")
    if out != wout:
        a, b = np.frombuffer(out, np.uint8), np.frombuffer(wout, np.uint8)
        k = int(np.flatnonzero(a != b)[0])
        j = int(np.searchsorted(woff, k, side="right")) - 1
        raise AssertionError(f"first differing byte {k} (output frame {j}, byte {k - int(woff[j])} of it): "
                             f"{a[k]:#x} != {b[k]:#x}")


def _check(gd, e, b, route=None, order=None, lead=0, t=T):
    want = R.request_batch(b, route, order, t)
    _same(_dev(gd, e, b, route, order, lead), want)
    return want


def _plain(n, bodies, rng=None, ext=None):
    """n addressed messages with the given bodies and no options, strings or KeyExt (182-B headers)."""
    rng = rng or np.random.default_rng(1)
    boff = np.zeros(n + 1, np.uint64)
    boff[1:] = np.cumsum([len(x) for x in bodies])
    b = {"target": np.array([R.grain_key(rng) for _ in range(n)], np.uint64).reshape(n, 3),
         "sender_grain": np.array([R.grain_key(rng) for _ in range(n)], np.uint64).reshape(n, 3),
         "sender_act": np.full(n, 3, np.uint32), "id_base": 1000, "ttl_ticks": R.TTL_NONE,
         "body": b"".join(bodies), "body_off": boff}
    if ext is not None:
        b["target_ext"] = ext
    route = {"silo": np.arange(n, dtype=np.uint32) % 5, "act": np.full(n, 7, np.uint32), "status": np.zeros(n, np.uint8)}
    return b, route


# ----------------------------------------------------------------------------- batches
def test_mixed_batch(gd, eng):
    rng = np.random.default_rng(31)
    n = 3000
    b, route = R.random_batch(n, rng, T)
    want = _check(gd, eng, b, route)
    assert (want[2] != R.ST_OK).sum() < n // 2 and set(want[2].tolist()) == {0, 1, 2, 3, 4}
    _check(gd, eng, b, route, order=rng.permutation(n).astype(np.uint32), lead=5)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_batch_sizes(gd, eng, n):
    rng = np.random.default_rng(300 + n)
    b, route = R.random_batch(n, rng, T)
    for lead in (0, 1, 7, 15):
        _check(gd, eng, b, route, lead=lead)


def test_every_frame_phase_and_tile_edges(gd, eng):
    rng = np.random.default_rng(32)
    # 182-B headers: body lengths 0..15 in turn move the frame starts through every 16-B phase
    bodies = [bytes(rng.integers(0, 256, size=k % 16, dtype=np.uint8)) for k in range(200)]
    b, route = _plain(200, bodies, rng)
    want = _check(gd, eng, b, route)
    assert (want[2] == R.ST_OK).all() and len(set(int(o) % 16 for o in want[1][:-1])) == 16
    assert len(want[0]) > 2 * TILE                                  # frames straddle two tile edges
    for lead in (3, 15):
        _check(gd, eng, b, route, lead=lead)
    # one body of 40,000 B spans three tiles; its neighbours are short
    bodies = [bytes(rng.integers(0, 256, size=k % 9, dtype=np.uint8)) for k in range(40)]
    bodies[17] = bytes(rng.integers(0, 256, size=40000, dtype=np.uint8))
    b, route = _plain(40, bodies, rng)
    for lead in (0, 9):
        want = _check(gd, eng, b, route, lead=lead)
    assert len(want[0]) > 40000 + TILE // 4
    # a total of exactly one tile: 64 frames of 256 B (182-B header + 74-B body)
    b, route = _plain(64, [bytes([k]) * 74 for k in range(64)], rng)
    want = _check(gd, eng, b, route)
    assert len(want[0]) == TILE
    _check(gd, eng, b, route, lead=8)


def test_long_strings_cross_tiles(gd, eng):
    """KeyExt strings of 300 B and a 300-B DebugContext on every message: strings that straddle tile edges."""
    rng = np.random.default_rng(33)
    n = 150
    b, route = _plain(n, [b"b" * (k % 5) for k in range(n)], rng, ext=["e" * (300 if k % 3 else 63) for k in range(n)])
    b["sender_ext"] = [None if k % 2 else "s" * 300 for k in range(n)]
    b["debug"] = np.full(n, 4, np.uint32)
    b["generic"] = np.full(n, 2, np.uint32)
    route["new_type"] = np.full(n, 2, np.uint32)
    want = _check(gd, eng, b, route, lead=11)
    assert len(want[0]) > 5 * TILE and (want[2] == R.ST_OK).all()


def test_optional_pointers_null(gd, eng):
    rng = np.random.default_rng(34)
    b, route = R.random_batch(400, rng, T)
    optional = ("target_ext", "sender_ext", "options", "generic", "debug", "body")
    for drop in [(k,) for k in optional] + [optional]:
        _same(_dev(gd, eng, b, route, drop=drop), R.request_batch(_without(b, drop), route, None, T))
    for k in ("placed", "new_type"):
        r = dict(route, **{k: None})
        _same(_dev(gd, eng, b, r), R.request_batch(b, r, None, T))
    got = _dev(gd, eng, b, None)                                    # no route arrays: nothing is addressed
    _same(got, R.request_batch(b, None, None, T))
    assert set(got[2].tolist()) <= {R.ST_UNADDRESSED, R.ST_FALLBACK, R.ST_NO_ID} and (got[2] == R.ST_UNADDRESSED).sum() > 300
    out, off, st, total = eng.request_frames(_without(b, optional))  # the host form, everything absent
    _same((out[:total].tobytes(), off, st), R.request_batch(_without(b, optional), None, None, T))


def test_order_of_the_sender_queues(gd, eng):
    rng = np.random.default_rng(35)
    n, nq = 2000, 5
    b, route = R.random_batch(n, rng, T)
    sh = SQ.hashes_with_edges(rng, len(T.silos))
    eng.send_configure(sh, nq)
    ttl = R.send_ttl(b)
    sst, q, perm, qoff = eng.send_queues(route["silo"], route["status"], None, ttl)
    wperm, wqoff = SQ.send_queues_loop(route["silo"], route["status"], None, ttl, sh, nq, T.my_silo)[2:4]
    np.testing.assert_array_equal(perm, wperm)
    got = _dev(gd, eng, b, route, order=perm)
    _same(got, R.request_batch(b, route, wperm, T))
    single = R.request_batch(b, route, None, T)
    fr = lambda i: single[0][int(single[1][i]):int(single[1][i + 1])]
    for k in range(len(qoff) - 1):                                  # each queue's bytes: one contiguous run
        run = got[0][int(got[1][qoff[k]]):int(got[1][qoff[k + 1]])]
        assert run == b"".join(fr(int(i)) for i in perm[qoff[k]:qoff[k + 1]])


def test_capacity(gd, eng):
    rng = np.random.default_rng(36)
    b, route = R.random_batch(300, rng, T)
    want = R.request_batch(b, route, None, T)
    total = len(want[0])
    with pytest.raises(gd.GrainDispatchError) as ei:               # at the next synchronisation: out_off complete,
        _dev(gd, eng, b, route, out_cap=total - 1)                  # nothing written (_dev)
    assert ei.value.code == gd.GD_EFULL
    np.testing.assert_array_equal(ei.value.out_off, want[1])
    out = np.full(total - 1, 0xA5, np.uint8)
    with pytest.raises(gd.GrainDispatchError) as ei:
        eng.request_frames(b, out=out, **route)
    assert ei.value.code == gd.GD_EFULL and (out == 0xA5).all()
    _same(_dev(gd, eng, b, route, out_cap=total), want)            # exactly enough; the handle still works
    out = np.full(total + 64, 0xA5, np.uint8)
    o2, off, st, tot = eng.request_frames(b, out=out, **route)
    assert tot == total and (out[total:] == 0xA5).all()
    _same((out[:total].tobytes(), off, st), want)


def test_round_trip_on_the_device(gd, eng):
    rng = np.random.default_rng(37)
    n = 600
    b, route = R.random_batch(n, rng, T)
    out, off, st = _dev(gd, eng, b, route)
    live = np.flatnonzero((st == R.ST_OK) | (st == R.ST_UNADDRESSED))
    f, tf = eng.decode_frames_turn(out, off[:-1][live])
    opt = b["options"][live]
    np.testing.assert_array_equal(f["target_grain"], b["target"][live])
    np.testing.assert_array_equal(f["sending_grain"], b["sender_grain"][live])
    np.testing.assert_array_equal(f["correlation_id"], (np.int64(b["id_base"]) + live).astype(np.int64))
    np.testing.assert_array_equal(f["direction"], np.where(opt & R.OPT_ONE_WAY, 2, 0))
    np.testing.assert_array_equal(tf["ttl"], np.where(opt & (R.OPT_ONE_WAY | R.OPT_NO_TTL), R.TTL_NONE, b["ttl_ticks"]))
    flags = np.where(opt & R.OPT_READ_ONLY, gd.MSG_READ_ONLY, 0) | np.where(opt & R.OPT_ALWAYS_INTERLEAVE,
                                                                           gd.MSG_ALWAYS_INTERLEAVE, 0)
    np.testing.assert_array_equal(tf["msg_flags"], flags)
    # the addressed requests answered on the device == the reference's answer to the reference's request bytes
    ok = np.flatnonzero(st == R.ST_OK)
    want_req = R.request_batch(b, route, None, T)
    eng.respond_configure(RSP.INFOS)
    kind = rng.choice([RSP.RSP_RESPONSE, RSP.RSP_REJECTION], size=len(ok)).astype(np.uint8)
    args = (kind, rng.integers(0, 2, size=len(ok)).astype(np.uint8), rng.integers(0, 4, size=len(ok)).astype(np.uint8),
            rng.integers(0, 5, size=len(ok)).astype(np.uint32), b"", np.zeros(len(ok) + 1, np.uint64))
    o2, off2, st2, tot2 = eng.respond_frames(out, off[:-1][ok], *args)
    want = RSP.respond_batch(want_req[0], want_req[1][:-1][ok], *args, None, RSP.INFOS)
    assert (want[2] == RSP.ST_OK).sum() > len(ok) // 2              # one-way requests are discarded, the rest answered
    _same((o2[:tot2].tobytes(), off2, st2), want)


def _chain_engine(gd, nq, rng):
    """A handle with a ring, a directory and every table of the chain; (engine, tables, send hashes, registered keys)."""
    import oracle as o
    silos = o.bench_silos(5)
    tuples = [(s.ip, s.port, s.gen) for s in silos]
    wire = [(bytes(gd.silo_addr(*t).ip), t[1], t[2]) for t in tuples]
    G = 512
    ids = np.zeros((G, 3), np.uint64)
    ids[:, 0], ids[:, 1], ids[:, 2] = np.arange(G) + 77, 5, 0x0400000000000000
    ids[9::50] = 0                                                  # some activations without an id
    t = R.Tables(wire, 1, ids, R.TYPES, R.STRINGS)
    spec = o.ring_spec(silos, "D")
    tc = o.grain_type_code(o.PING_GRAIN_CLASS)
    reg = o.grain_keys(tc, np.arange(G))
    owner = o.ring_owner_np(spec, o.jenkins_u64x3_np(reg[:, 2], reg[:, 0], reg[:, 1])).astype(np.uint32)
    e = gd.GrainDispatch(device=0, table_capacity=4 * G, my_silo=1)
    e.ring_set_silos("D", tuples)
    e.register(reg, np.arange(G), owner)
    e.encode_configure(tuples, t.types)
    e.request_configure(t.strings)
    e.activation_ids_set(np.arange(G), ids)
    sh = SQ.hashes_with_edges(rng, len(tuples))
    e.send_configure(sh, nq)
    return e, t, sh, o.grain_keys(tc, rng.integers(0, G + 60, size=1500))


def test_chain(gd):
    import torch
    rng = np.random.default_rng(38)
    nq = 4
    e, t, sh, targets = _chain_engine(gd, nq, rng)
    n = len(targets)
    with e:
        b, _ = R.random_batch(n, rng, t)
        b["target"] = targets
        b["ttl_ticks"] = 5000
        # the three stages called separately ...
        rst, silo, act = e.route(b["target"])
        sst, q, perm, qoff = e.send_queues(silo, rst, None, R.send_ttl(b))
        route = {"silo": silo, "act": act, "status": rst}
        out, off, st, total = e.request_frames(b, order=perm, **route)
        assert (rst == 0).sum() > n // 2 and (rst != 0).any() and (st == R.ST_OK).sum() > n // 3
        _same((out[:total].tobytes(), off, st), R.request_batch(b, route, perm, t))
        # ... the host chain ...
        c = e.request_send(b)
        for k, w in (("status", rst), ("silo", silo), ("act", act), ("send_status", sst), ("queue", q), ("perm", perm),
                     ("offsets", qoff), ("out_off", off), ("req_status", st)):
            np.testing.assert_array_equal(c[k], w, err_msg=k)
        assert c["total"] == total and c["out"][:total].tobytes() == out[:total].tobytes()
        # ... and the device chain
        dev = torch.device("cuda:0")
        db = _DevBatch(gd, b)
        i32 = lambda k: torch.full((k,), -1, dtype=torch.int32, device=dev)
        u8 = lambda k: torch.full((k,), 0xEE, dtype=torch.uint8, device=dev)
        d_silo, d_act, d_perm, d_q, d_qoff = i32(n), i32(n), i32(n), i32(n), i32(nq + 5)
        d_rst, d_sst, d_st = u8(n), u8(n), u8(n)
        d_out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=dev)
        d_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        e.request_send_device(db.d, n, d_silo.data_ptr(), d_act.data_ptr(), d_rst.data_ptr(), d_sst.data_ptr(),
                              d_q.data_ptr(), d_perm.data_ptr(), d_qoff.data_ptr(), d_out.data_ptr(), total,
                              d_off.data_ptr(), d_st.data_ptr())
        e.synchronize()
        h32 = lambda x: x.cpu().numpy().view(np.uint32)
        for got, w, name in ((h32(d_silo), silo, "silo"), (h32(d_act), act, "act"), (d_rst.cpu().numpy(), rst, "status"),
                             (d_sst.cpu().numpy(), sst, "send_status"), (h32(d_q), q, "queue"), (h32(d_perm), perm, "perm"),
                             (h32(d_qoff), qoff, "offsets"), (d_off.cpu().numpy().view(np.uint64), off, "out_off"),
                             (d_st.cpu().numpy(), st, "req_status")):
            np.testing.assert_array_equal(got, w, err_msg=name)
        whole = d_out.cpu().numpy()
        assert whole[:total].tobytes() == out[:total].tobytes() and (whole[total:] == 0xA5).all()
        # the callbacks need no device result: ids are id_base + i, the caller knows the one-way calls
        e.callbacks_configure(4 * n)
        two_way = np.flatnonzero((b["options"] & R.OPT_ONE_WAY) == 0)
        ids = (np.int64(b["id_base"]) + two_way).astype(np.int64)
        assert e.callbacks_add(ids, two_way.astype(np.uint32), np.full(len(ids), 1 << 40, np.int64)).all()
        hd, _, _, found = e.callbacks_lookup(ids)
        assert found.all() and (hd == two_way).all()
        one_way = np.flatnonzero(b["options"] & R.OPT_ONE_WAY)
        assert not e.callbacks_lookup((np.int64(b["id_base"]) + one_way).astype(np.int64))[3].any()


def test_state_errors(gd, eng):
    rng = np.random.default_rng(39)
    b, route = R.random_batch(3, rng, T)
    with gd.GrainDispatch(device=0, table_capacity=1 << 10, my_silo=1) as e:
        for step in (lambda: None, lambda: e.encode_configure(R.SILO_TUPLES, T.types)):
            step()                                                  # before either configure, then before the second
            with pytest.raises(gd.GrainDispatchError) as ei:
                e.request_frames(b, **route)
            assert ei.value.code == gd.GD_ESTATE
            with pytest.raises(gd.GrainDispatchError) as ei:
                e.request_frames_device({"target": 8, "sender_grain": 8, "sender_act": 8}, 0, None, None, None, None,
                                        None, None, 0, 0, 8, 0)
            assert ei.value.code == gd.GD_ESTATE
        e.request_configure([])                                     # no strings: every index names none
        e.activation_ids_set(np.arange(len(T.act_ids)), T.act_ids)
        out, off, st, total = e.request_frames(b, **route)
        _same((out[:total].tobytes(), off, st), R.request_batch(b, route, None, R.Tables(R.SILOS, 1, T.act_ids, T.types, [])))
        with pytest.raises(gd.GrainDispatchError) as ei:           # the chain needs the sender queues too
            e.request_send(b)
        assert ei.value.code == gd.GD_ESTATE
    with gd.GrainDispatch(device=0, table_capacity=1 << 10, my_silo=7) as e:   # my_silo outside the silo table
        _configure(e)
        with pytest.raises(gd.GrainDispatchError) as ei:
            e.request_frames(b, **route)
        assert ei.value.code == gd.GD_ESTATE
    empty = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in _without(b, ("target_ext", "sender_ext", "body")).items()}
    out, off, st, total = eng.request_frames(empty, out_cap=16)
    assert total == 0 and off.tolist() == [0] and len(st) == 0
    with pytest.raises(gd.GrainDispatchError) as ei:               # totals are 32-bit: the bound is refused
        eng.request_frames_device({"target": 8, "sender_grain": 8, "sender_act": 8}, 1 << 25, None, None, None, None,
                                  None, None, 8, 0, 8, 8)
    assert ei.value.code == gd.GD_EINVAL
    with pytest.raises(gd.GrainDispatchError) as ei:               # silo without act and status
        eng.request_frames(b, silo=route["silo"])
    assert ei.value.code == gd.GD_EINVAL
