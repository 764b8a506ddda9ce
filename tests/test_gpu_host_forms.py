"""The host-pointer forms of the six batched stages share one staging pool in the handle.  One
handle, configured for all six, takes their calls interleaved, in two orders, at n = 65 and n = a stage tile + 1
(the encoder, whose tile is 16 KiB of output: 65 and 257 frames), so every pool slot is used small then large and
large then small, by arrays of different element widths; the optional arrays (route_status, category, ttl;
strategy, given_silo; start_idx, wait_perm; n_started_by, start_pos; the old list, msg_id, the keys; result,
rejection, flags, fire_idx; placed, new_type, order) change between consecutive calls of a stage, so a slot is
skipped in one call and taken in the next.  Every output is compared bit for bit with the per-stage references.

test_reference_inputs_agree_on_the_cpu runs the same cases through the references' two forms without a GPU."""
import copy
import ctypes as C

import numpy as np
import pytest

import _callbacks_ref as CR
import _encode_ref as ER
import _place_ref as PR
import _pump_ref as PP
import _sendq_ref as SQ
import _turns_ref as TR
import test_gpu_callbacks as TCB
import test_gpu_encode as TE
import test_gpu_place as TP
import test_gpu_pump as TPU

T = 4096                          # SQ_TILE = PL_TILE = TN_TILE, the bucketing's tile, the fire list's tile
SIZES = {"send": (65, T + 1), "place": (65, T + 1), "turns": (65, T + 1), "pump": (65, T + 1),
         "callbacks": (65, T + 1), "encode": (65, 257)}
STAGES = tuple(SIZES)
N_SILOS, NQ = 8, 7
SH = SQ.hashes_with_edges(np.random.default_rng(5), N_SILOS)


def _rng(stage, n, k):
    return np.random.default_rng(1000 * STAGES.index(stage) + 10 * n + k)


def _pick(k, *arrays):
    """Call k of a stage passes array j when bit j of (all, none, even ones, odd ones)[k] is set."""
    mask = (0xFF, 0x00, 0x55, 0xAA)[k]
    return tuple(a if mask >> j & 1 else None for j, a in enumerate(arrays))


def send_case(n, k):
    silo, rs, cat, ttl = SQ.mixed_batch(_rng("send", n, k), n, N_SILOS, TP.MY)
    return (silo,) + _pick(k, rs, cat, ttl)


def place_case(n, k):
    keys, strat, given = TP._mixed(_rng("place", n, k), n)
    strat, given = _pick(k, strat, given)
    return keys, PR.PLACE_HASH if strat is None else strat, given


def turns_case(n, k):
    b = TR.mixed_batch(_rng("turns", n, k), n, (7, 1025)[k % 2], limits=k < 2)
    b.recv_status, b.direction, b.ttl, b.forward_count, b.msg_flags, ta = _pick(
        k, b.recv_status, b.direction, b.ttl, b.forward_count, b.msg_flags, b.target_activation)
    if ta is None:
        b.target_activation = b.sending_activation = None
        b.chain = False
    return b, b.hard_limit > 0 or k == 2      # request_count: needed with a limit, unread (passed or not) without


def pump_case(n, k):
    return PP.mixed_pump(_rng("pump", n, k), n, (7, 1025)[k % 2], ("uniform", "zipf")[k // 2], flags=k not in (1, 2))


def merge_case(n, k):
    return TPU._merge_case(_rng("pump", n, 4 + k), (7, 1025)[k % 2], n, old=k != 1, keys=k in (0, 3), ids=k in (0, 2))


def respond_case(table, n, k):
    ids, res, rej, fl = CR.mixed_batch(_rng("callbacks", n, k), table, n)
    return (ids,) + _pick(k, res, rej, fl)


def encode_case(n, k):
    rng = _rng("encode", n, k)
    buf, offs, silo, act, status, placed, new_type = ER.random_batch(n, rng, TE.CFG)
    return (buf, offs, silo, act, status) + _pick(k, placed, new_type, rng.permutation(n).astype(np.uint32))


def _script():
    """(stage, n, call number of the stage): the stages in order, small then large; then reversed, large then small."""
    steps = [(s, SIZES[s][j]) for j in (0, 1) for s in STAGES] + [(s, SIZES[s][j]) for j in (1, 0) for s in STAGES[::-1]]
    seen = {}
    for s, n in steps:
        k = seen.get(s, 0)
        seen[s] = k + 1
        yield s, n, k


def _eq(got, want, names):
    assert len(got) == len(want) == len(names), names
    for name, a, b in zip(names, got, want):
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a, b, err_msg=name)


TURN_NAMES = ("turn", "num_running_out", "running_idx", "start_idx", "wait_perm", "wait_offsets")


def _turns(gd, e, b, with_rc, starts, waits):
    """gd_turns with the start list and the wait lists asked for separately (the binding asks for both or neither)."""
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    n, n_ctx = b.n, b.n_ctx
    st = gd.gd_turn_state(b.ctx_flags.ctypes.data, b.num_running.ctypes.data,
                          b.request_count.ctypes.data if with_rc else None, b.hard_limit, b.hard_limit_sw,
                          b.max_forward_count, int(b.chain))
    turn, nro, run = np.zeros(n, np.uint8), np.zeros(n_ctx, np.uint32), np.zeros(n_ctx, np.uint32)
    start, n_start = (np.zeros(n, np.uint32), np.zeros(1, np.uint32)) if starts else (None, None)
    perm, off = (np.zeros(n, np.uint32), np.zeros(n_ctx + 2, np.uint32)) if waits else (None, None)
    rc = gd.lib.gd_turns(e.h, p(b.ctx), p(b.recv_status), p(b.direction), p(b.ttl), p(b.forward_count), p(b.msg_flags),
                         p(b.target_activation), p(b.sending_activation), n, n_ctx, C.byref(st), p(turn), p(nro), p(run),
                         p(start), p(n_start), p(perm), p(off))
    assert rc == gd.GD_OK, gd.lib.gd_last_error(e.h)
    return turn, nro, run, None if start is None else start[:int(n_start[0])], perm, off


@pytest.mark.gpu
def test_interleaved_host_forms_share_the_pool():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from orleans_amd import graindispatch as gd
    with TP.World(gd) as w:
        e = w.e
        e.send_configure(SH, NQ)
        TE._configure(e)
        cb = TCB.Mirror(e, 4 * T, max_resend=1)
        act_base, next_id = 1000, 1
        for stage, n, k in _script():
            if stage == "send":
                args = send_case(n, k)
                bucket = k in (0, 3)
                want = SQ.send_queues_loop(*args, SH, NQ, TP.MY)
                _eq(e.send_queues(*args, bucket=bucket), want if bucket else want[:2],
                    ("send_status", "queue", "perm", "offsets")[:4 if bucket else 2])
            elif stage == "place":
                keys, strat, given = place_case(n, k)
                got = w.run(keys, strat, given, act_base=act_base, n_act=(None, 3000)[k // 2])
                act_base += got[5]
            elif stage == "turns":
                b, with_rc = turns_case(n, k)
                starts, waits = k in (0, 2), k in (0, 3)
                want = TR.turns_loop(b)
                got = _turns(gd, e, b, with_rc, starts, waits)
                keep = [j for j in range(6) if j < 3 or (starts if j == 3 else waits)]
                _eq([got[j] for j in keep], [want[j] for j in keep], [TURN_NAMES[j] for j in keep])
            elif stage == "pump":
                b = pump_case(n, k)
                started_by, starts = k in (0, 2), k in (0, 3)
                want = PP.pump_loop(b)
                keep = [j for j in range(7) if j < 5 or (started_by if j == 5 else starts)]
                _eq(TPU._call(e, b, started_by=started_by, starts=starts), [want[j] for j in keep],
                    [PP.NAMES[j] for j in keep])
                TPU._merge_check(e, *merge_case(n, k))
            elif stage == "callbacks":
                rng = _rng("callbacks", n, 8 + k)
                ids = TCB.fresh_ids(rng, n, lo=next_id)
                next_id += n
                cb.add(ids, rng.integers(0, 1 << 32, n, dtype=np.uint32), rng.integers(-5, 1 << 40, n, dtype=np.int64))
                cb.set_target(ids[: n // 2], rng.integers(0, N_SILOS, n // 2).astype(np.uint32))
                args = respond_case(cb.t, n, k)
                fire = k in (0, 2)
                cb.seen |= set(int(x) for x in args[0])
                want = cb.t.respond(*args)
                _eq(e.callbacks_respond(*args, fire=fire), want if fire else want[:3],
                    ("outcome", "flags", "handle", "fire_idx")[:4 if fire else 3])
                cb.verify()
                cb.scan("expire", 1 << 30)
            else:
                buf, offs, silo, act, status, placed, new_type, order = encode_case(n, k)
                want = ER.encode_batch(buf, offs, silo, act, status, placed, new_type, order, TE.CFG)
                out = np.full(len(buf) + n * 300 + 64, 0xA5, np.uint8)
                _, off, est, total = e.encode_frames(buf, offs, silo, act, status, placed, new_type, order, out=out)
                assert total == len(want[0]) and (out[total:] == 0xA5).all()
                TE._same((out[:total].tobytes(), off, est), want)


def test_reference_inputs_agree_on_the_cpu():
    """The cases above through both forms of every reference: the inputs are good before they meet the GPU."""
    same = lambda a, b: [np.testing.assert_array_equal(x, y) for x, y in zip(a, b, strict=True)]
    table = CR.Table(CR.Options(1))
    silos = TP.o.bench_silos(8)                # the directory and the configuration TP.World starts from
    directory, cfg, spec = TP.DirectoryState(), PR.PlaceConfig(silos, my_silo=TP.MY), TP.o.ring_spec(silos, "D")
    acts = np.arange(300, dtype=np.uint32)
    acts[::17] = TP.o.ACT_MULTI
    directory.upsert(TP.o.grain_keys(TP.TC, np.arange(300)), acts, (np.arange(300) % 8).astype(np.uint32))
    act_base, next_id = 1000, 1
    for stage, n, k in _script():
        if stage == "send":
            args = send_case(n, k)
            same(SQ.send_queues_np(*args, SH, NQ, TP.MY), SQ.send_queues_loop(*args, SH, NQ, TP.MY))
        elif stage == "place":
            keys, strat, given = place_case(n, k)
            route = PR.route_of(keys, spec, directory, TP.MY, TP.SEED)
            other = copy.deepcopy(directory)
            want = PR.place_loop(keys, route, strat, given, act_base, cfg, directory)
            got = PR.place_np(keys, route, strat, given, act_base, cfg, other)
            same(got[:5], want[:5])
            assert got[5] == want[5] and other.entries == directory.entries
            act_base += want[5]
        elif stage == "turns":
            b, _ = turns_case(n, k)
            same(TR.turns_np(b), TR.turns_loop(b))
        elif stage == "pump":
            b = pump_case(n, k)
            same(PP.pump_np(b), PP.pump_loop(b))
            args, kw = merge_case(n, k)
            off, msg, fl, total = PP.merge_loop(*args, **kw)       # one form only: it runs, and is consistent
            assert total == len(msg) == len(fl) == int(off[-1])
        elif stage == "callbacks":
            rng = _rng("callbacks", n, 8 + k)
            ids = TCB.fresh_ids(rng, n, lo=next_id)
            next_id += n
            table.add(ids, rng.integers(0, 1 << 32, n, dtype=np.uint32), rng.integers(-5, 1 << 40, n, dtype=np.int64))
            table.set_target(ids[: n // 2], rng.integers(0, N_SILOS, n // 2).astype(np.uint32))
            args = respond_case(table, n, k)
            other = copy.deepcopy(table)
            same(CR.respond_np(other, *args), table.respond(*args))
            table.expire(1 << 30)
        else:
            buf, offs, silo, act, status, placed, new_type, order = encode_case(n, k)
            a = ER.encode_batch(buf, offs, silo, act, status, placed, new_type, order, TE.CFG)
            b = ER.encode_batch(buf, offs, silo, act, status, placed, new_type, order, TE.CFG, form=ER.encode_reparse)
            assert a[0] == b[0]
            same(a[1:], b[1:])
