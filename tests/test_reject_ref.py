"""CPU checks of the forward-rejection reference (tests/_reject_ref.py): its two forms -- the field
form and the composition of the forward splice with the responder's reference -- agree on the batches the GPU tests
use, every status is reached, the frozen vectors of tests/golden/reject.json still come out, and the answers decode
as the reference's rule says."""
import json
import os
import struct

import numpy as np
import pytest

import _cih_ref as C
import _forward_ref as F
import _reject_ref as J
import _respond_ref as R
import headers as H

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reject.json")


@pytest.fixture(scope="module")
def cfg():
    return F.make_config(np.random.default_rng(9))


@pytest.mark.parametrize("max_fc", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_forms_agree(cfg, n, max_fc):
    rng = np.random.default_rng(1000 + 10 * n + max_fc)
    batch = J.random_batch(n, rng, cfg, max_fc)
    order = rng.permutation(n).astype(np.uint32)
    a = J.reject_batch(*batch, order, max_fc, F.LOCAL_SILO, cfg, form=J.reject_fields)
    b = J.reject_batch(*batch, order, max_fc, F.LOCAL_SILO, cfg, form=J.reject_compose)
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[0] == b[0]


def test_every_status_and_the_partition(cfg):
    rng = np.random.default_rng(77)
    n = 900
    batch = J.random_batch(n, rng, cfg)
    buf, offs, kind, old_act = batch[:4]
    for local in (F.LOCAL_SILO, 9):
        out, off, st = J.reject_batch(*batch, None, F.MAX_FC, local, cfg)
        fst = F.forward_batch(buf, offs, kind, old_act, None, None, None, None, F.MAX_FC, local, cfg)[2]
        np.testing.assert_array_equal(np.isin(st, J.FWD_REJECT_SET), fst == F.ST_REJECT)
        for mine, theirs in ((J.ST_SKIPPED, F.ST_SKIPPED), (J.ST_MALFORMED, F.ST_MALFORMED), (J.ST_FALLBACK, F.ST_FALLBACK)):
            np.testing.assert_array_equal(st == mine, fst == theirs)
        if local == F.LOCAL_SILO:
            assert set(np.unique(st).tolist()) == set(range(8)) - {J.ST_NO_SILO}
        else:
            assert (st == J.ST_NO_SILO).sum() > n // 10
    assert (st == J.ST_OK).sum() > n // 10


def test_without_an_old_address_it_is_the_responder(cfg):
    """old_act absent: the bytes are respond_walk's (kind REJECTION, type 0) wherever that is OK; its one FALLBACK
    frame (entries, a default-valued Category byte, a DebugContext) is written here."""
    rng = np.random.default_rng(78)
    buf, offs, kind, _, info, body, body_off = J.random_batch(400, rng, cfg, max_fc=0)
    kind[:] = F.FWD_FORWARD
    out, off, st = J.reject_batch(buf, offs, kind, None, info, body, body_off, None, 0, F.LOCAL_SILO, cfg)
    seen_ok = seen_split = 0
    for i in range(len(offs)):
        b = body[int(body_off[i]):int(body_off[i + 1])]
        rst, want = C.respond_walk(buf, int(offs[i]), R.RSP_REJECTION, None, 0, int(info[i]), b, J.INFOS)
        got = out[int(off[i]):int(off[i + 1])]
        if st[i] == J.ST_OK:
            assert rst in (R.ST_OK, R.ST_FALLBACK)
        if rst == R.ST_OK:
            # the forward writer's FALLBACK set is the wider one: no TargetGrain, any system target
            assert st[i] in (J.ST_OK, J.ST_MAY_FORWARD, J.ST_FALLBACK)
        if rst == R.ST_OK and st[i] == J.ST_OK:
            assert got == want
            seen_ok += 1
        elif rst == R.ST_FALLBACK and st[i] == J.ST_OK:
            h = F.parse_fields(got, struct.unpack_from("<i", got, 0)[0])[0]
            assert "category" not in h and h["debug_context"] and h["invalidation"]
            seen_split += 1
    assert seen_ok > 100 and seen_split >= 1


def test_the_answer_decodes(cfg):
    """The appended entry is the last one, behind the old ones in order; Direction Response, Result Rejection, the
    addresses exchanged."""
    rng = np.random.default_rng(79)
    frames = [C.request(rng, count=c, tg_ext=x, forward_count=2, time_to_live=5, target_silo=F.SILOS[3],
                        target_activation=((4, 5, 0), None))
              for c in (None, 0, 1, 3) for x in (None, "", "ext")]
    buf, offs = F.pack_frames(frames)
    n = len(offs)
    old = np.flatnonzero(cfg.act_ids.any(axis=1))[:n].astype(np.uint32)
    out, off, st = J.reject_batch(buf, offs, np.ones(n, np.uint8), old, np.zeros(n, np.uint32), None, None, None,
                                  F.MAX_FC, F.LOCAL_SILO, cfg)
    assert (st == J.ST_OK).all()
    for i in range(n):
        fr = out[int(off[i]):int(off[i + 1])]
        req = F.parse_fields(frames[i], struct.unpack_from("<i", frames[i], 0)[0])[0]
        h = F.parse_fields(fr, struct.unpack_from("<i", fr, 0)[0])[0]
        assert h["invalidation"][:-1] == req.get("invalidation", [])
        assert h["invalidation"][-1] == (H.w_silo(*F.SILOS[F.LOCAL_SILO]), req["target_grain"],
                                         (cfg.act_id(int(old[i])), None))
        assert h["direction"] == 1 and h["result"] == 2 and "rejection_type" not in h and "forward_count" not in h
        assert h["rejection_info"] == J.INFOS[0] and h["correlation_id"] == req["correlation_id"]
        assert h["target_grain"] == req["sending_grain"] and h["sending_grain"] == req["target_grain"]
        assert h["sending_silo"] == req["target_silo"] and h["target_silo"] == req["sending_silo"]
        assert h["sending_activation"] == req["target_activation"]


def test_golden(cfg):
    with open(GOLDEN) as f:
        g = json.load(f)
    gcfg = F.Config([bytes.fromhex(s) for s in g["silos"]], [], np.array(g["act_ids"], dtype=np.uint64))
    assert len(g["cases"]) >= 6
    for c in g["cases"]:
        frame = bytes.fromhex(c["frame"])
        for form in (J.reject_fields, J.reject_compose):
            st, out = form(frame, 0, c["kind"], c["old_act"], c["info"], bytes.fromhex(c["body"]), c["max_fc"],
                           c["local_silo"], gcfg, g["infos"])
            assert st == c["status"], c["name"]
            assert out.hex() == c["out"], c["name"]
