"""GPU parity for the turn headers out of the frame decoder and the frame-fed chain:
gd_decode_frames_turn* and gd_receive_turns_frames* through the C ABI against tests/_frame_turns_ref.py (the literal
walk of HeadersContainer.Deserializer, composed with oracle/receive.py and _turns_ref.turns_loop).  Every output is
compared bit for bit, dtype included."""
import ctypes as C
import struct

import numpy as np
import pytest

import headers as H
import oracle as o
import _frame_turns_ref as F
import _turns_ref as T
from _callbacks_ref import Options, Table

pytestmark = pytest.mark.gpu

FRAME_WIN = 192                  # gd_frames.h: the bytes of a frame staged in LDS; past them the walk reads global memory
TILE = 4096                      # gd_turns.h TN_TILE
TC = o.grain_type_code(o.PING_GRAIN_CLASS)
TURN_NAMES = ("turn", "num_running_out", "running_idx", "start_idx", "wait_perm", "wait_offsets")
RECV_NAMES = ("status", "ctx", "perm", "offsets")


@pytest.fixture(scope="module")
def gd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as g
    return g


@pytest.fixture(scope="module")
def eng(gd):
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        yield e


def _same(got, want, name):
    assert got.dtype == want.dtype, name
    np.testing.assert_array_equal(got, want, err_msg=name)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _zeros(count, width):
    import torch
    return torch.zeros(max(count, 1) * width + 16, dtype=torch.uint8, device="cuda")


def _host(t, dt, count):
    return t.cpu().numpy()[:count * np.dtype(dt).itemsize].view(dt).copy()


def _decode(gd, eng, buf, off, form, turn_fields=tuple(F.TURN_FIELDS), fields=None):
    """(frame fields, turn fields) by the host or the device entry point."""
    if form == "host":
        return eng.decode_frames_turn(buf, off, fields, turn_fields)
    n = len(off)
    want = list(gd.FRAME_FIELDS) if fields is None else ["flags", "target_grain", *fields]
    d_buf, d_off = _dev(np.frombuffer(buf, np.uint8)), _dev(np.asarray(off, np.uint64))
    width = lambda k: int(np.prod(gd.FRAME_FIELDS[k][1], dtype=np.int64)) * np.dtype(gd.FRAME_FIELDS[k][0]).itemsize
    d_f = {k: _zeros(n, width(k)) for k in want}
    d_t = None if turn_fields is None else {k: _zeros(n, np.dtype(F.TURN_FIELDS[k]).itemsize) for k in turn_fields}
    eng.decode_frames_turn_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n, {k: v.data_ptr() for k, v in d_f.items()},
                                  None if d_t is None else {k: v.data_ptr() for k, v in d_t.items()})
    eng.synchronize()
    fr = {k: _host(v, gd.FRAME_FIELDS[k][0], n * max(1, int(np.prod(gd.FRAME_FIELDS[k][1], dtype=np.int64))))
          .reshape((n,) + gd.FRAME_FIELDS[k][1]) for k, v in d_f.items()}
    tr = {} if d_t is None else {k: _host(v, F.TURN_FIELDS[k], n) for k, v in d_t.items()}
    return fr, tr


def _check_decode(gd, eng, buf, off, form="host"):
    fr, tr = _decode(gd, eng, buf, off, form)
    want_f, want_t = H.decode_frames(buf, off), F.walk_frames(buf, off)
    for k in gd.FRAME_FIELDS:
        _same(fr[k], want_f[k], k)
    for k in F.TURN_FIELDS:
        _same(tr[k], want_t[k], k)
    return want_f, want_t


def _random_frames(rng, n):
    """Frames with every turn header drawn at random, some fallback / malformed, long DebugContexts among them."""
    tg = o.grain_keys(TC, rng.integers(0, 1000, size=n))
    ta = rng.integers(1, 1 << 62, size=(n, 3), dtype=np.int64).astype(np.uint64)
    return F.chain_frames(rng, tg, ta, ta, rng.choice(np.array([0, 1, 2, 0xFF], np.uint8), size=n))


# ---- decode ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_decode_batch_sizes(gd, eng, n):
    buf, off = _random_frames(np.random.default_rng(100 + n), n)
    for form in ("host", "device"):
        _, t = _check_decode(gd, eng, buf, off, form)
    if n >= 255:
        assert (t["ttl"] != F.TTL_NONE).any() and t["msg_flags"].any() and t["result"].any() and t["resend_count"].any()


@pytest.mark.parametrize("form", ["host", "device"])
def test_decode_output_selection(gd, eng, form):
    buf, off = _random_frames(np.random.default_rng(7), 700)
    want_f, want_t = H.decode_frames(buf, off), F.walk_frames(buf, off)
    for sel in [[k] for k in F.TURN_FIELDS] + [list(F.TURN_FIELDS), ["ttl", "result"]]:
        fr, tr = _decode(gd, eng, buf, off, form, sel, fields=["mask"])
        assert set(tr) == set(sel)
        for k in sel:
            _same(tr[k], want_t[k], k)
        _same(fr["flags"], want_f["flags"], "flags")
        _same(fr["mask"], want_f["mask"], "mask")
    # a NULL struct, and a struct of NULLs: gd_decode_frames itself
    plain = eng.decode_frames(buf, off)
    for sel in (None, []):
        fr, tr = _decode(gd, eng, buf, off, form, sel)
        assert tr == {}
        for k in gd.FRAME_FIELDS:
            _same(fr[k], plain[k], k)
            _same(fr[k], want_f[k], k)


def _edge_frame(kind, pos, pad_to4=True):
    """A frame whose `kind` header's first byte is at frame-relative position pos: lengths 8 + mask 4 + category 1 +
    DebugContext (4 + L) + direction 1 = 18 + L bytes come first."""
    L = pos - 18
    h = {"category": 2, "debug_context": "d" * L, "direction": 0, "target_grain": ((0, pos, 0x0300000000000001), None),
         "target_activation": ((pos, 1, 0), None), "target_silo": F.SILO}
    if kind == "ttl":
        h["time_to_live"] = 0x1122334455667788 + pos
    elif kind == "forward_count":
        h["forward_count"] = 1 + pos % 200
    elif kind == "read_only":
        h["read_only"] = True
    else:                                                   # every header, the ttl at pos
        h.update(time_to_live=-pos, forward_count=3, always_interleave=True, is_new_placement=False, read_only=True,
                 is_unordered=True, rejection_type=2, resend_count=0x01020304 + pos, result=1, correlation_id=pos)
    fr = H.encode_frame(h)
    return fr + bytes(-len(fr) % 4) if pad_to4 else fr      # filler after the frame: the next one keeps its alignment


@pytest.mark.parametrize("sh", [0, 1, 2, 3])
def test_decode_window_edge(gd, eng, sh):
    """The header's first byte from 12 bytes before the staged window's last byte to 4 past it, for every alignment of
    the frame start: fields wholly inside, straddling the limit (FRAME_WIN - (frame_start & 3)) and wholly past it."""
    frames = []
    for kind in ("ttl", "forward_count", "read_only", "all"):
        for pos in range(FRAME_WIN - 12, FRAME_WIN + 5):
            frames.append(_edge_frame(kind, pos))
    buf, off = F.join_frames(frames, lead=4 + sh)
    assert ((off & np.uint64(3)) == sh).all()
    for form in ("host", "device"):
        _, t = _check_decode(gd, eng, buf, off, form)
    k = FRAME_WIN + 5 - (FRAME_WIN - 12)
    pos = np.arange(FRAME_WIN - 12, FRAME_WIN + 5)
    np.testing.assert_array_equal(t["ttl"][:k], 0x1122334455667788 + pos)
    np.testing.assert_array_equal(t["forward_count"][k:2 * k], 1 + pos % 200)
    assert (t["msg_flags"][2 * k:3 * k] == T.MSG_READ_ONLY).all() and (t["msg_flags"][3 * k:] == 3).all()
    np.testing.assert_array_equal(t["resend_count"][3 * k:], 0x01020304 + pos)


@pytest.mark.parametrize("mod", [(4, 1), (4, 2), (4, 3), (16, 4), (16, 8), (16, 12)])
def test_decode_header_ends_at_the_last_byte_of_the_buffer(gd, eng, mod):
    """The last frame has no body and no target: its Result byte is the buffer's last byte, with the buffer's length
    not a multiple of 4 / of 16 (the bytes past the last whole dword / 16 B are never staged)."""
    m, r = mod
    first = _edge_frame("all", 100)
    last = None
    for L in range(150, 190):
        h = {"debug_context": "d" * L, "time_to_live": 77, "forward_count": 2, "read_only": True, "resend_count": 5,
             "result": 2}
        fr = H.encode_frame(h)
        if (len(first) + len(fr)) % m == r and ((len(first) + len(fr)) % 4 != 0 or m == 16):
            last = fr
            break
    buf, off = F.join_frames([first, last])
    assert len(buf) % m == r and off[1] + len(last) == len(buf)
    for form in ("host", "device"):
        f, t = _check_decode(gd, eng, buf, off, form)
    assert f["flags"][1] == 0 and t["result"][1] == 2 and t["resend_count"][1] == 5 and t["ttl"][1] == 77
    # and a buffer too short for one staged chunk: every byte by the global path
    tiny = H.encode_frame({"result": 1, "read_only": True})
    assert len(tiny) < 16
    for form in ("host", "device"):
        _, t = _check_decode(gd, eng, tiny, np.zeros(1, np.uint64), form)
    assert t["result"][0] == 1 and t["msg_flags"][0] == T.MSG_READ_ONLY


def test_decode_malformed_reads_absent(gd, eng):
    """Header lengths that end inside the ttl, inside the forward count, and on the two bool bytes."""
    h = {"category": 2, "direction": 0, "time_to_live": 5, "forward_count": 1, "correlation_id": 3,
         "always_interleave": True, "read_only": True, "rejection_type": 1, "resend_count": 2, "result": 1,
         "target_grain": ((0, 1, 0x0300000000000001), None), "target_activation": ((1, 1, 0), None), "target_silo": F.SILO}
    good = H.encode_frame(h, bytes(9))
    # frame-relative: category 12, direction 13, ttl 14-21, forward count 22-25, correlation id 26-33, bools 34, 35
    ends = list(range(15, 22)) + [23, 24, 25] + [34, 35]
    frames = [good]
    for end in ends:
        fr = bytearray(good)
        struct.pack_into("<i", fr, 0, end - 8)
        frames.append(bytes(fr))
    buf, off = F.join_frames(frames + [good], lead=1)
    f, t = _check_decode(gd, eng, buf, off)
    bad = slice(1, 1 + len(ends))
    assert (f["flags"][bad] == H.F_MALFORMED).all() and f["flags"][0] == f["flags"][-1] == 3
    for k, v in F.ABSENT.items():
        assert (t[k][bad] == v).all(), k
    assert t["ttl"][0] == 5 and t["msg_flags"][-1] == 3


def test_decode_fallback(gd, eng):
    """RequestContext and CacheInvalidationHeader frames read absent; TargetObserver frames read decoded."""
    rng = np.random.default_rng(3)
    frames, kinds = [], []
    for i in range(300):
        h = F.turn_frame(rng, (0, i, 0x0300000000000001), (i + 1, 2, 0), p=0.8)
        kind = i % 4
        if kind == 1:
            h["request_context"] = b"\x01\x00\x00\x00" + bytes(12)
        elif kind == 2:
            h["cache_invalidation"] = struct.pack("<i", 0)
        elif kind == 3:
            h["target_observer"] = bytes(rng.integers(0, 256, size=20, dtype=np.uint8))
        frames.append(H.encode_frame(h, bytes(int(rng.integers(0, 9)))))
        kinds.append(kind)
    kinds = np.array(kinds)
    buf, off = F.join_frames(frames, lead=3)
    f, t = _check_decode(gd, eng, buf, off)
    assert ((f["flags"] & H.F_FALLBACK) != 0).tolist() == (kinds != 0).tolist()
    for k, v in F.ABSENT.items():
        assert (t[k][(kinds == 1) | (kinds == 2)] == v).all(), k
    obs = kinds == 3
    assert (t["ttl"][obs] != F.TTL_NONE).sum() > 30 and t["msg_flags"][obs].any() and t["result"][obs].any()


# ---- the frame-fed chain ----------------------------------------------------------------------------

N_POOL = 1025                    # activation ids the frames target; context = pool index % n_ctx


class World:
    """One batch of frames (shared by the n_ctx variants of a shape) and its decoded reference."""

    def __init__(self, n):
        rng = np.random.default_rng(1000 + n)
        self.n = n
        self.aid = np.zeros((N_POOL, 3), np.uint64)
        self.aid[:, 0] = rng.integers(1, 1 << 62, size=N_POOL, dtype=np.int64).astype(np.uint64)
        self.aid[:, 1] = np.arange(N_POOL)
        which = rng.integers(0, N_POOL + 40, size=n)            # a few activations the directory does not know
        which[rng.random(n) < 0.3] = 0                          # one hot activation
        known = which < N_POOL
        ta = np.zeros((n, 3), np.uint64)
        ta[known] = self.aid[which[known]]
        ta[~known, 0] = 7
        ta[~known, 1] = which[~known]
        sa = rng.integers(1, 1 << 62, size=(n, 3), dtype=np.int64).astype(np.uint64)
        same = (which == 0) & (rng.random(n) < 0.5)             # call-chain messages on the hot one
        sa[same] = ta[same]
        tg = o.grain_keys(TC, rng.integers(0, 1000, size=n))
        direction = rng.choice(np.array([0, 0, 0, 1, 2, 0xFF], np.uint8), size=n)
        self.buf, self.off = F.chain_frames(rng, tg, ta, sa, direction)
        self.mor = (rng.random(n) < 0.2).astype(np.uint8) * T.MSG_MAY_INTERLEAVE | \
                   (rng.random(n) < 0.1).astype(np.uint8) * T.MSG_READ_ONLY
        self.d_buf, self.d_off, self.d_mor = _dev(np.frombuffer(self.buf, np.uint8)), _dev(self.off), _dev(self.mor)
        self.decoded = None                                     # the reference decode, computed once

    def case(self, n_ctx, limits, seed=0):
        rng = np.random.default_rng(n_ctx * 7 + seed)
        ctxs = (np.arange(N_POOL) % n_ctx).astype(np.uint32)
        keep = np.arange(N_POOL) < max(n_ctx, 64)               # distinct contexts need not all be there
        adf = np.where(rng.random(N_POOL) < 0.9, 1, 0) | np.where(rng.random(N_POOL) < 0.3, 4, 0)
        adf[0] = 1
        fl, nr = T.context_state(rng, n_ctx)
        fl[0] = T.CTX_VALID                                     # the hot one: idle, so call chains interleave
        per = max(1, self.n // n_ctx)
        rc0 = rng.integers(0, per + 4, n_ctx).astype(np.uint32)
        return dict(keys=self.aid[keep], ctxs=ctxs[keep], adf=adf[keep].astype(np.uint8), n_ctx=n_ctx, fl=fl, nr=nr,
                    rc0=rc0, recv_lim=(per + 6, per // 2 + 3) if limits else (0, 0),
                    turn_lim=(per + 3, per // 2 + 2) if limits else (0, 0))


_WORLDS = {}


def world(n):
    if n not in _WORLDS:
        _WORLDS[n] = World(n)
    return _WORLDS[n]


def _reference(w, c, age, use_or):
    """The composed reference; the turn stage's request_count is the receive stage's start value plus what it
    enqueued (tests/_turns_ref.py request_count_after_receive)."""
    if w.decoded is None:
        w.decoded = (H.decode_frames(w.buf, w.off), F.walk_frames(w.buf, w.off))
    f = w.decoded[0]
    lim = c["recv_lim"]
    st, ctx, perm, offs = F.receive_frames_ref(f, c["keys"], c["ctxs"], c["adf"], c["n_ctx"],
                                               c["rc0"] if lim[0] else None, lim[0], lim[1])
    rc = T.request_count_after_receive(c["rc0"], offs, c["n_ctx"])
    out = F.chain_ref(w.buf, w.off, c["keys"], c["ctxs"], c["adf"], c["n_ctx"], c["fl"], c["nr"], rc,
                      c["rc0"] if lim[0] else None, lim[0], lim[1], age, w.mor if use_or else None, c["turn_lim"][0],
                      c["turn_lim"][1], 2, True, decoded=w.decoded)
    return rc, out


class DeviceOut:
    def __init__(self, n, n_ctx):
        self.n, self.n_ctx = n, n_ctx
        self.ctx, self.st, self.perm, self.offs = _zeros(n, 4), _zeros(n, 1), _zeros(n, 4), _zeros(n_ctx + 3, 4)
        self.turn, self.nro, self.run = _zeros(n, 1), _zeros(n_ctx, 4), _zeros(n_ctx, 4)
        self.start, self.ns, self.wp, self.wo = _zeros(n, 4), _zeros(1, 4), _zeros(n, 4), _zeros(n_ctx + 2, 4)

    def recv(self):
        n, n_ctx = self.n, self.n_ctx
        return (_host(self.st, np.uint8, n), _host(self.ctx, np.uint32, n), _host(self.perm, np.uint32, n),
                _host(self.offs, np.uint32, n_ctx + 3))

    def turns(self):
        n, n_ctx = self.n, self.n_ctx
        ns = int(_host(self.ns, np.uint32, 1)[0])
        return (_host(self.turn, np.uint8, n), _host(self.nro, np.uint32, n_ctx), _host(self.run, np.uint32, n_ctx),
                _host(self.start, np.uint32, n)[:ns], _host(self.wp, np.uint32, n), _host(self.wo, np.uint32, n_ctx + 2))


def _fused_device(eng, w, c, rc, age, use_or, d_fields=None, d_turn_fields=None):
    n, n_ctx = w.n, c["n_ctx"]
    out = DeviceOut(n, n_ctx)
    keep = (_dev(c["fl"]), _dev(c["nr"]), _dev(rc), _dev(c["rc0"]))
    state = eng.turn_state_device(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), c["turn_lim"][0],
                                  c["turn_lim"][1], 2, True)
    lim = c["recv_lim"]
    eng.receive_turns_frames_device(w.d_buf.data_ptr(), len(w.buf), w.d_off.data_ptr(), n, n_ctx, d_fields, d_turn_fields,
                                    out.ctx.data_ptr(), out.st.data_ptr(), out.perm.data_ptr(), out.offs.data_ptr(), age,
                                    w.d_mor.data_ptr() if use_or else None, state, out.turn.data_ptr(),
                                    out.nro.data_ptr(), out.run.data_ptr(), out.start.data_ptr(), out.ns.data_ptr(),
                                    out.wp.data_ptr(), out.wo.data_ptr(), keep[3].data_ptr() if lim[0] else None,
                                    lim[0], lim[1])
    eng.synchronize()
    return out


def _fill_directory(eng, c):
    eng.actdir_clear()
    assert eng.actdir_add(c["keys"], c["ctxs"], c["adf"]).all()


CHAIN_N = [1, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]
CHAIN_CTX = [1, 7, 1025]
# limits, a ttl age and the flag merge each on and off for every n and every n_ctx
CHAIN = [(n, n_ctx, (i + j) % 2 == 0, (0, 51)[(i + 2 * j + (i + j) // 2) % 2], (i // 2 + j) % 2 == 0)
         for i, n in enumerate(CHAIN_N) for j, n_ctx in enumerate(CHAIN_CTX)]


@pytest.mark.parametrize("n,n_ctx,limits,age,use_or", CHAIN)
def test_fused_chain_device(eng, n, n_ctx, limits, age, use_or):
    w = world(n)
    c = w.case(n_ctx, limits)
    _fill_directory(eng, c)
    rc, want = _reference(w, c, age, use_or)
    out = _fused_device(eng, w, c, rc, age, use_or)
    for name, a, b in zip(RECV_NAMES, out.recv(), want[2:6]):
        _same(a, b, name)
    for name, a, b in zip(TURN_NAMES, out.turns(), want[6:]):
        _same(a, b, name)
    st, turn = want[2], want[6]
    assert not turn[st != 0].any()                           # UNDECODED (and not enqueued) frames: GD_TURN_NONE
    if n >= TILE - 1:
        assert (st == F.RECV_UNDECODED).sum() > 100
        if not limits:
            assert (st == 0).sum() > 1000 and len(set(np.unique(turn).tolist())) >= 4
            hot = (want[3] == 0) & (st == 0)
            assert (turn[hot] == T.TURN_START).sum() > 100   # the hot context's call chains interleave


def test_fused_chain_covers_every_switch():
    for col, values in ((0, CHAIN_N), (1, CHAIN_CTX)):
        for v in values:
            rows = [c for c in CHAIN if c[col] == v]
            assert all(len({c[k] for c in rows}) == 2 for k in (2, 3, 4)), (col, v)


@pytest.mark.parametrize("n,n_ctx,limits,age,use_or", [(65, 7, True, 51, True), (3 * TILE + 17, 1025, True, 51, True),
                                                       (TILE + 1, 1, False, 0, False)])
def test_fused_chain_host_form_equals_device_form(eng, n, n_ctx, limits, age, use_or):
    w = world(n)
    c = w.case(n_ctx, limits)
    _fill_directory(eng, c)
    rc, want = _reference(w, c, age, use_or)
    out = _fused_device(eng, w, c, rc, age, use_or)
    lim = c["recv_lim"]
    got = eng.receive_turns_frames(w.buf, w.off, n_ctx, c["fl"], c["nr"], rc, c["rc0"] if lim[0] else None, lim[0], lim[1],
                                   age, w.mor if use_or else None, c["turn_lim"][0], c["turn_lim"][1], 2, True,
                                   fields=["target_activation", "direction"], turn_fields=list(F.TURN_FIELDS))
    dec, tdec = got[0], got[1]
    d_st, d_ctx, d_perm, d_offs = out.recv()
    for name, a, b in zip(("ctx", "status", "perm", "offsets"), got[2:6], (d_ctx, d_st, d_perm, d_offs)):
        _same(a, b, name)
    for name, a, b in zip(TURN_NAMES, got[6:], out.turns()):
        _same(a, b, name)
    for name, a, b in zip(TURN_NAMES, got[6:], want[6:]):
        _same(a, b, name)
    for k in ("flags", "target_grain", "target_activation", "direction"):
        _same(dec[k], want[0][k], k)
    for k in F.TURN_FIELDS:                                  # as the wire has them: before the age and the merge
        _same(tdec[k], want[1][k], k)


def test_fused_equals_receive_frames_then_turns(eng):
    """The parent's path: gd_receive_frames_device, then gd_turns_device fed with side arrays the host computed by
    the reference walk (the ttl aged, the flags merged).  Every output equals the fused call's."""
    n, n_ctx, age = 3 * TILE + 17, 7, 51
    w = world(n)
    c = w.case(n_ctx, True)
    _fill_directory(eng, c)
    rc, want = _reference(w, c, age, True)
    d_tf = {k: _zeros(n, np.dtype(dt).itemsize) for k, dt in F.TURN_FIELDS.items()}
    fused = _fused_device(eng, w, c, rc, age, True, None, {k: v.data_ptr() for k, v in d_tf.items()})
    for k, dt in F.TURN_FIELDS.items():
        _same(_host(d_tf[k], dt, n), want[1][k], k)
    t = want[1]
    d_ttl, d_fwd = _dev(F.aged_ttl(t["ttl"], age)), _dev(t["forward_count"])
    d_mf = _dev(t["msg_flags"] | w.mor)
    two = DeviceOut(n, n_ctx)
    d_f = {"flags": _zeros(n, 4), "target_grain": _zeros(n, 24), "target_activation": _zeros(n, 24),
           "sending_activation": _zeros(n, 24), "direction": _zeros(n, 1)}
    ff = eng_frame_fields(eng, d_f)
    keep = (_dev(c["fl"]), _dev(c["nr"]), _dev(rc), _dev(c["rc0"]))
    from orleans_amd import graindispatch as g
    lim = g.gd_recv_limits(keep[3].data_ptr(), c["recv_lim"][0], c["recv_lim"][1])
    V = lambda x: C.c_void_p(x.data_ptr())
    eng._c(g.lib.gd_receive_frames_device(eng.h, V(w.d_buf), len(w.buf), V(w.d_off), n, n_ctx, C.byref(lim), C.byref(ff),
                                          V(two.ctx), V(two.st), V(two.perm), V(two.offs)))
    state = eng.turn_state_device(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), c["turn_lim"][0],
                                  c["turn_lim"][1], 2, True)
    eng.turns_device(two.ctx.data_ptr(), two.st.data_ptr(), d_f["direction"].data_ptr(), d_ttl.data_ptr(),
                     d_fwd.data_ptr(), d_mf.data_ptr(), d_f["target_activation"].data_ptr(),
                     d_f["sending_activation"].data_ptr(), n, n_ctx, state, two.turn.data_ptr(), two.nro.data_ptr(),
                     two.run.data_ptr(), two.start.data_ptr(), two.ns.data_ptr(), two.wp.data_ptr(), two.wo.data_ptr())
    eng.synchronize()
    for name, a, b in zip(RECV_NAMES, fused.recv(), two.recv()):
        _same(a, b, name)
    for name, a, b in zip(TURN_NAMES, fused.turns(), two.turns()):
        _same(a, b, name)
    for name, a, b in zip(TURN_NAMES, fused.turns(), want[6:]):
        _same(a, b, name)


def eng_frame_fields(eng, d_f):
    from orleans_amd import graindispatch as g
    return g.gd_frame_fields(**{k: C.c_void_p(v.data_ptr()) for k, v in d_f.items()})


def test_chain_into_callbacks(gd):
    """Result and RejectionType decoded on the device go, with the fused call's d_turn and the decoded correlation
    ids, straight into gd_callbacks_respond_device."""
    import torch
    rng = np.random.default_rng(12)
    n, n_ctx = 900, 5
    aid = np.zeros((n_ctx, 3), np.uint64)
    aid[:, 0] = np.arange(1, n_ctx + 1)
    which = rng.integers(0, n_ctx, n)
    ids = np.arange(1, n + 1, dtype=np.int64)
    rng.shuffle(ids)
    frames = []
    for i in range(n):
        h = {"category": 2, "direction": int(rng.choice([0, 1, 1])), "correlation_id": int(ids[i]),
             "target_grain": ((0, i, 0x0300000000000001), None), "target_activation": (tuple(int(x) for x in aid[which[i]]), None),
             "target_silo": F.SILO}
        if rng.random() < 0.7:
            h["result"] = int(rng.choice([0, 2]))
        if rng.random() < 0.5:
            h["rejection_type"] = int(rng.choice([0, 1]))
        if rng.random() < 0.1:
            h["debug_context"] = "d" * int(rng.integers(150, 200))
        frames.append(H.encode_frame(h, bytes(int(rng.integers(0, 20)))))
    buf, off = F.join_frames(frames, lead=2)
    fl = rng.choice(np.array([0, 2], np.uint8), n_ctx, p=[0.7, 0.3])             # VALID / INVALID
    fl[0], fl[1] = 0, 2
    nr, rc = np.zeros(n_ctx, np.uint32), np.zeros(n_ctx, np.uint32)
    want = F.chain_ref(buf, off, aid, np.arange(n_ctx, dtype=np.uint32), np.ones(n_ctx, np.uint8), n_ctx, fl, nr, rc)
    t, turn = want[1], want[6]
    assert (turn == T.TURN_RESPONSE).sum() > 100 and (turn == T.TURN_RESPONSE_DROPPED).sum() > 20
    table = Table(Options(1, False, 0))
    handles, dl = np.arange(n, dtype=np.uint32), rng.integers(0, 1000, n, dtype=np.int64)
    with gd.GrainDispatch(device=0, table_capacity=1024) as e:
        e.callbacks_configure(4096, 1, False, 0)
        _same(e.callbacks_add(ids, handles, dl), table.add(ids, handles, dl), "added")
        assert e.actdir_add(aid, np.arange(n_ctx, dtype=np.uint32), np.ones(n_ctx, np.uint8)).all()
        d_buf, d_off = _dev(np.frombuffer(buf, np.uint8)), _dev(off)
        d_f = {"flags": _zeros(n, 4), "target_grain": _zeros(n, 24), "correlation_id": _zeros(n, 8)}
        d_t = {"result": _zeros(n, 1), "rejection_type": _zeros(n, 1)}
        out = DeviceOut(n, n_ctx)
        keep = (_dev(fl), _dev(nr), _dev(rc))
        state = e.turn_state_device(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr())
        d_oc, d_of, d_oh, d_fi, d_nf = _zeros(n, 1), _zeros(n, 1), _zeros(n, 4), _zeros(n, 4), _zeros(1, 4)
        torch.cuda.synchronize()
        e.receive_turns_frames_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n, n_ctx,
                                      {k: v.data_ptr() for k, v in d_f.items()}, {k: v.data_ptr() for k, v in d_t.items()},
                                      out.ctx.data_ptr(), out.st.data_ptr(), None, None, 0, None, state,
                                      out.turn.data_ptr(), out.nro.data_ptr(), out.run.data_ptr())
        e.callbacks_respond_device(d_f["correlation_id"].data_ptr(), d_t["result"].data_ptr(),
                                   d_t["rejection_type"].data_ptr(), None, out.turn.data_ptr(), n, d_oc.data_ptr(),
                                   d_of.data_ptr(), d_oh.data_ptr(), d_fi.data_ptr(), d_nf.data_ptr())
        e.synchronize()
        _same(_host(out.turn, np.uint8, n), turn, "turn")
        _same(_host(d_t["result"], np.uint8, n), t["result"], "result")
        _same(_host(d_t["rejection_type"], np.uint8, n), t["rejection_type"], "rejection_type")
        _same(_host(d_f["correlation_id"], np.int64, n), ids, "correlation_id")
        w = table.respond(ids, t["result"], t["rejection_type"], None, turn)
        nf = int(_host(d_nf, np.uint32, 1)[0])
        got = (_host(d_oc, np.uint8, n), _host(d_of, np.uint8, n), _host(d_oh, np.uint32, n), _host(d_fi, np.uint32, n)[:nf])
        for name, a, b in zip(("outcome", "flags", "handle", "fire_idx"), got, w):
            _same(a, b, name)
        assert len(w[3]) > 50


def test_argument_errors_and_capture_refusal(gd, eng):
    import torch
    lib, h = gd.lib, eng.h
    n, n_ctx = 4, 2
    eng.actdir_clear()
    buf, off = _random_frames(np.random.default_rng(1), n)
    P = lambda a: C.c_void_p(a.ctypes.data)
    b = np.frombuffer(buf, np.uint8)
    flags, tg, ttl = np.zeros(n, np.uint32), np.zeros((n, 3), np.uint64), np.zeros(n, np.int64)
    tf = gd.gd_frame_turn_fields(ttl=ttl.ctypes.data)
    dec = lambda ff: lib.gd_decode_frames_turn(h, P(b), len(buf), P(off), n, C.byref(ff), C.byref(tf))
    assert dec(gd.gd_frame_fields(flags=flags.ctypes.data, target_grain=tg.ctypes.data)) == gd.GD_OK
    assert dec(gd.gd_frame_fields(target_grain=tg.ctypes.data)) == gd.GD_EINVAL          # flags missing
    assert dec(gd.gd_frame_fields(flags=flags.ctypes.data)) == gd.GD_EINVAL              # target_grain missing
    assert lib.gd_decode_frames_turn(h, P(b), len(buf), P(off), n, None, C.byref(tf)) == gd.GD_EINVAL
    assert lib.gd_decode_frames_turn_device(h, P(b), len(buf), P(off), n, None, C.byref(tf)) == gd.GD_EINVAL
    fl, nr = np.zeros(n_ctx, np.uint8), np.zeros(n_ctx, np.uint32)
    st = gd.gd_turn_state(fl.ctypes.data, nr.ctypes.data, None, 0, 0, 2, 0)
    ctx, rs, turn = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    nro, run = np.zeros(n_ctx, np.uint32), np.zeros(n_ctx, np.uint32)

    def fused(age=0, ff=None, turn_p=P(turn), state=st):
        return lib.gd_receive_turns_frames(h, P(b), len(buf), P(off), n, n_ctx, None, None if ff is None else C.byref(ff),
                                           None, P(ctx), P(rs), None, None, age, None,
                                           None if state is None else C.byref(state), turn_p, P(nro), P(run), None, None,
                                           None, None)
    assert fused() == gd.GD_OK
    assert fused(age=-1) == gd.GD_EINVAL and fused(age=-(1 << 63)) == gd.GD_EINVAL
    assert fused(ff=gd.gd_frame_fields(target_grain=tg.ctypes.data)) == gd.GD_EINVAL
    assert fused(ff=gd.gd_frame_fields(flags=flags.ctypes.data)) == gd.GD_EINVAL
    assert fused(turn_p=None) == gd.GD_EINVAL and fused(state=None) == gd.GD_EINVAL
    assert lib.gd_receive_turns_frames(None, P(b), len(buf), P(off), n, n_ctx, None, None, None, P(ctx), P(rs), None, None,
                                       0, None, C.byref(st), P(turn), P(nro), P(run), None, None, None, None) == gd.GD_EINVAL
    # under a stream capture both forms are refused before anything is launched
    w = world(65)
    c = w.case(7, False)
    out = DeviceOut(65, 7)
    keep = (_dev(c["fl"]), _dev(c["nr"]), _dev(c["rc0"]))
    state = eng.turn_state_device(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr())
    mine = torch.zeros(4, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.set_stream(s.cuda_stream)
    eng.set_kernel_timing(True)
    eng.kernel_times_reset()
    graph = torch.cuda.CUDAGraph()
    codes = []
    with torch.cuda.graph(graph, stream=s):
        mine.add_(1)                                         # the capture holds one node of the test's own
        for call in (lambda: eng.receive_turns_frames_device(
                         w.d_buf.data_ptr(), len(w.buf), w.d_off.data_ptr(), 65, 7, None, None, out.ctx.data_ptr(),
                         out.st.data_ptr(), None, None, 0, None, state, out.turn.data_ptr(), out.nro.data_ptr(),
                         out.run.data_ptr()),
                     lambda: eng.receive_turns_frames(w.buf, w.off, 7, c["fl"], c["nr"], c["rc0"])):
            with pytest.raises(gd.GrainDispatchError) as ei:
                call()
            codes.append(ei.value.code)
    eng.set_stream(None)
    assert codes == [gd.GD_ESTATE] * 2
    assert not any(k.startswith("k_") for k in eng.kernel_times())
    eng.set_kernel_timing(False)
