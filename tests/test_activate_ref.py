"""The two forms of the activation stage's reference (tests/_activate_ref.py) agree, its scenes contain every case
the GPU tests rely on, and the chained model is the turn stage run on the resolved arrays."""
import numpy as np
import pytest

import _activate_ref as A
import _turns_ref as T


def _same(a, b):
    for k in A.OUT_NAMES:
        if k == "n_proposed":
            assert a[k] == b[k]
        else:
            assert a[k].dtype == b[k].dtype, k
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["entries"] == b["entries"] and a["err_range"] == b["err_range"]


def _both(b):
    lo, cl = A.activate_loop(b), A.activate_closed(b)
    _same(lo, cl)
    return lo


@pytest.mark.parametrize("n", [0, 1, 7, 63, 64, 65, 257, 1500])
@pytest.mark.parametrize("given", [True, False])
def test_forms_agree(n, given):
    b, scripted, _ = A.scene(np.random.default_rng(n + 17 * given), n, given=given)
    r = _both(b)
    assert r["n_proposed"] <= b.cap_new and not r["err_range"]
    if n >= 257:
        A.assert_scene_cases(b, r, scripted)


def test_hot_id_scene():
    hot = [10, 30, 63, 64, 70, 200, 255, 256, 300, 4095, 4096, 4100, 4999]
    b, scripted, hot_id = A.scene(np.random.default_rng(5), 5000, hot=hot)
    A.assert_scene_cases(b, _both(b), scripted, hot_id)


def test_optional_arrays_and_no_participants():
    b, _, _ = A.scene(np.random.default_rng(3), 300)
    b.direction = b.ttl = b.new_placement = None
    r = _both(b)
    assert r["n_proposed"] == 0 and len(r["new_idx"]) == 0 and A.ACTV_NONEXISTENT in r["kind"]
    b, _, _ = A.scene(np.random.default_rng(4), 300, p_part=0.0)
    b.recv_status[:7] = 0
    r = _both(b)
    assert not r["kind"].any() and r["entries"] == b.entries
    np.testing.assert_array_equal(r["ctx"], b.ctx)
    np.testing.assert_array_equal(r["status"], b.recv_status)


def test_terminating_creates_nothing():
    b, _, _ = A.scene(np.random.default_rng(8), 400, terminating=True)
    r = _both(b)
    assert r["n_proposed"] == 0 and r["entries"] == b.entries and A.ACTV_CREATED not in r["kind"]
    assert A.ACTV_FOUND in r["kind"] and A.ACTV_NONEXISTENT in r["kind"]


def test_refusal_is_whole():
    b, _, _ = A.scene(np.random.default_rng(9), 400)
    want = _both(b)
    b.cap_new = want["n_proposed"]                         # n_proposed == cap_new: accepted, the same outputs
    b.new_ctx = b.new_ctx[:b.cap_new]
    _same(_both(b), want)
    b.cap_new -= 1
    b.new_ctx = b.new_ctx[:-1]
    r = _both(b)
    assert r["n_proposed"] == b.cap_new + 1 and r["entries"] == b.entries
    assert len(r["new_idx"]) == 0 and len(r["gone_idx"]) == 0
    assert not np.isin(r["kind"], (A.ACTV_CREATED, A.ACTV_NONEXISTENT, A.ACTV_NONEXISTENT_RESPONSE)).any()
    # rules 1-3 still decide
    decided = np.isin(want["kind"], (A.ACTV_NONE, A.ACTV_EXPIRED)) | \
        np.array([k in b.entries for k in b.keys()])
    np.testing.assert_array_equal(r["kind"][decided], want["kind"][decided])
    assert (r["kind"][~decided] == A.ACTV_HOST).all()


def test_proposal_out_of_range_refuses():
    b, _, _ = A.scene(np.random.default_rng(10), 300)
    b.new_ctx[b.cap_new // 2] = b.n_ctx
    r = _both(b)
    assert r["err_range"] and r["entries"] == b.entries and A.ACTV_CREATED not in r["kind"]
    # a FOUND entry whose context is out of range: HOST and the error, the rest of the batch goes on
    b, _, _ = A.scene(np.random.default_rng(11), 300)
    k = next(k for k, v in b.entries.items() if not v[1] & A.AD_SYSTEM_TARGET)
    b.entries[k] = (b.n_ctx + 3, 0)
    r = _both(b)
    assert r["err_range"] and A.ACTV_CREATED in r["kind"]


def test_chain_is_turns_on_the_resolved_arrays():
    rng = np.random.default_rng(12)
    b, _, _ = A.scene(rng, 600)
    fl, nr = T.context_state(rng, b.n_ctx)
    for k in range(b.ctx_base, b.n_ctx):                     # the contexts offered to new activations
        fl[k], nr[k] = T.CTX_NOT_READY, 0
    rc = np.zeros(b.n_ctx, np.uint32)
    fwd = rng.integers(0, 4, b.n).astype(np.uint8)
    mf = rng.integers(0, 8, b.n).astype(np.uint8)
    m = A.chain_model(b, fl, nr, rc, fwd, mf)
    m2 = A.chain_model(b, fl, nr, rc, fwd, mf, form=A.activate_closed, turns=T.turns_np)
    for k in ("ctx", "status", "perm", "offsets", "turn", "num_running_out", "running_idx", "start_idx", "wait_perm",
              "wait_offsets"):
        np.testing.assert_array_equal(m[k], m2[k], err_msg=k)
    # a created activation's requests wait in order on its list; bucket c of perm holds the resolved messages
    created = m["new_idx"]
    assert len(created)
    for i in created:
        c = int(m["ctx"][i])
        lo, hi = int(m["offsets"][c]), int(m["offsets"][c + 1])
        members = m["perm"][lo:hi]
        assert members[0] == i and (np.diff(members.astype(np.int64)) > 0).all()
        assert (m["ctx"][members] == c).all()
        req = [j for j in members if m["turn"][j] not in (T.TURN_EXPIRED, T.TURN_RESPONSE)]
        assert all(m["turn"][j] == T.TURN_WAIT for j in req)
        wl = m["wait_perm"][int(m["wait_offsets"][c]):int(m["wait_offsets"][c + 1])]
        np.testing.assert_array_equal(wl, np.array(req, np.uint32))
    # the null bucket keeps only what was not resolved
    null = m["perm"][int(m["offsets"][b.n_ctx]):int(m["offsets"][b.n_ctx + 1])]
    assert np.isin(m["kind"][null], (A.ACTV_EXPIRED, A.ACTV_HOST, A.ACTV_NONEXISTENT, A.ACTV_NONEXISTENT_RESPONSE)).all()
