// eng_activate.hip -- libgraindispatch: the activation stage of a received batch (gd_activate.h):
// Catalog.GetOrCreateActivation for the messages gd_receive left on the null context, alone; the chained forms
// (receive -> activate -> turns) are in eng_turns.hip.  Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_activate.h"

namespace gdx {

int check_activate_args(gd_handle* h, const ActivateArgs& a, const char* call) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (a.n && (!a.ctx || !a.recv_status || !a.target_activation || !a.kind || !a.ctx_out || !a.status_out))
        return set_err(h, GD_EINVAL, "%s: null argument", call);
    if (!a.n_proposed) return set_err(h, GD_EINVAL, "%s: null n_proposed", call);
    if ((a.new_idx != nullptr) != (a.n_new != nullptr)) return set_err(h, GD_EINVAL, "%s: new_idx and n_new go together", call);
    if ((a.gone_idx != nullptr) != (a.n_gone != nullptr))
        return set_err(h, GD_EINVAL, "%s: gone_idx and n_gone go together", call);
    if (a.n > (1u << 31)) return set_err(h, GD_EINVAL, "%s: n > 2^31", call);
    if (a.n_ctx >= 0xFFFFFFFDu) return set_err(h, GD_EINVAL, "%s: n_ctx too large", call);
    if (a.ttl_age < 0) return set_err(h, GD_EINVAL, "%s: ttl_age_ticks < 0", call);
    if (!a.new_ctx && (uint64_t)a.ctx_base + a.cap_new > a.n_ctx)
        return set_err(h, GD_EINVAL, "%s: ctx_base %u + cap_new %u is past n_ctx %u", call, a.ctx_base, a.cap_new, a.n_ctx);
    return GD_OK;
}

// The stage on device arrays; the words (n_new, n_gone, n_proposed) are device words.  host_form: the claim passes
// are driven by read-backs, and *refused says whether the batch was refused whole (the stream is idle then).
int activate_device(gd_handle* h, const ActivateArgs& a, bool host_form, bool* refused, const char* call) {
    if (refused) *refused = false;
    const uint32_t n = a.n;
    if (n == 0) {
        GD_TRY(launch(h, "k_fill", dim3(1), dim3(BLOCK), 0, k_fill_u32, a.n_proposed, 1u, 0u));
        if (a.n_new) GD_TRY(launch(h, "k_fill", dim3(1), dim3(BLOCK), 0, k_fill_u32, a.n_new, 1u, 0u));
        if (a.n_gone) GD_TRY(launch(h, "k_fill", dim3(1), dim3(BLOCK), 0, k_fill_u32, a.n_gone, 1u, 0u));
        return GD_OK;
    }
    if (!h->ad_slots) GD_TRY(ad_rehash(h, 1024));
    // room for every entry the batch can create, before anything is claimed: at most one a message, cap_new in all
    const uint32_t m_cap = a.terminating ? 0u : std::min(n, a.cap_new);
    if (m_cap)
        GD_TRY(table_reserve(
            h, h->ad_used_ub, h->ad_cap, m_cap, call,
            [&](uint64_t& live, uint64_t& tomb) {
                GD_TRY(ad_pull(h));
                live = h->ad_host.live;
                tomb = h->ad_host.tomb;
                return (int)GD_OK;
            },
            [&](unsigned long long cap, uint64_t) { return ad_rehash(h, cap); }));
    StageTime stage(h, "stage:activate");
    DevBuf* S = h->actv_scr;
    const uint32_t tiles = blocks_for(n, PL_TILE);
    for (int k = 0; k < 3; ++k) GD_TRY(ensure(h, S[k], ((size_t)tiles + 1) * 4));
    GD_TRY(ensure(h, S[3], (size_t)m_cap * 4 + 4));
    GD_TRY(ensure(h, S[4], (size_t)m_cap * sizeof(gd_key) + 8));
    GD_TRY(ensure(h, S[5], (size_t)m_cap * 4 + 4));
    GD_TRY(ensure(h, S[6], (size_t)m_cap * 4 + 4));
    GD_TRY(ensure(h, S[7], (size_t)m_cap + 16));
    GD_TRY(ensure(h, S[8], sizeof(ActvWords)));
    uint32_t *tile_cand = (uint32_t*)S[0].p, *tile_new = (uint32_t*)S[1].p, *tile_gone = (uint32_t*)S[2].p;
    uint32_t* idx = (uint32_t*)S[3].p;
    gd_key* ckeys = (gd_key*)S[4].p;
    uint32_t *prop = (uint32_t*)S[5].p, *slot_of = (uint32_t*)S[6].p;
    uint8_t* is_new = (uint8_t*)S[7].p;
    ActvWords* w = (ActvWords*)S[8].p;
    uint32_t* last = (uint32_t*)h->ad_last.p;
    uint32_t* err = &h->ctr->err;
    HIP_TRY(h, hipMemsetAsync(w, 0, sizeof(ActvWords), h->stream));

    const ActvIn in{a.ctx, a.recv_status, a.target_activation, a.direction, a.ttl, a.new_placement, a.ttl_age, n,
                    a.n_ctx, a.terminating ? 1u : 0u};
    const uint32_t wide =
        ((((uintptr_t)a.recv_status | (uintptr_t)a.kind | (uintptr_t)a.status_out) & 15u) == 0 ? AV_WIDE_BYTES : 0u) |
        ((((uintptr_t)a.ctx | (uintptr_t)a.ctx_out) & 15u) == 0 ? AV_WIDE_CTX : 0u);
    const dim3 gt(tiles), bt(PL_NT);
    GD_TRY(launch(h, "k_actv_classify", gt, bt, 0, k_actv_classify, in, ad_args(h), wide, a.kind, a.ctx_out, a.status_out,
                  tile_cand, tiles, err));
    GD_TRY(scan_device<OpAdd>(h, tile_cand, tiles + 1, false, false, "actv_cand"));
    if (m_cap)
        GD_TRY(launch(h, "k_actv_gather", gt, bt, 0, k_actv_gather, (const uint8_t*)a.kind, a.target_activation, n,
                      a.n_ctx, wide, (const uint32_t*)tile_cand, a.new_ctx, a.ctx_base, m_cap, idx, ckeys, prop, w));
    GD_TRY(launch(h, "k_actv_gate", dim3(1), dim3(WAVE), 0, k_actv_gate, (const uint32_t*)(tile_cand + tiles), a.cap_new,
                  w, a.n_proposed, err));
    // the candidates the claims run over: the device's count in the device form, read back in the host form
    uint32_t m = m_cap;
    if (host_form) {
        uint32_t hw[3] = {0, 0, 0};
        GD_TRY(read_back(h, w, hw, 3));
        if (refused) *refused = hw[0] == 0;
        m = hw[0] ? hw[2] : 0u;
    }
    if (m) {
        const dim3 gc(blocks_for(m, BLOCK)), bc(BLOCK);
        const uint32_t* unsettled = nullptr;
        const int rc = claim_pass_driver(
            h, w->retry, m <= (1u << 16) ? REG_PASSES_SMALL : REG_PASSES, host_form, call, &unsettled,
            [&](uint32_t p, const uint32_t* gate, uint32_t* word) {
                return launch(h, "k_actv_claim", gc, bc, 0, k_actv_claim, (const gd_key*)ckeys, (const ActvWords*)w,
                              h->ad_slots, h->ad_cap - 1ull, h->ad_ctr, err, slot_of, is_new, p, gate, word, last);
            });
        // unsettled read-back passes: the claims made so far keep their words (pass 0 wrote every slot_of)
        if (rc == GD_ETIMEOUT)
            (void)launch(h, "k_actv_clear", gc, bc, 0, k_actv_clear, (const ActvWords*)w, (const uint32_t*)slot_of, last);
        if (rc != GD_OK) return rc;
        GD_TRY(launch(h, "k_actv_commit", gc, bc, 0, k_actv_commit, (const ActvWords*)w, (const uint32_t*)slot_of,
                      (const uint8_t*)is_new, (const uint32_t*)prop, h->ad_slots, h->ad_ctr, (const uint32_t*)last,
                      unsettled, err));
    }
    GD_TRY(launch(h, "k_actv_resolve", gt, bt, 0, k_actv_resolve, a.target_activation, n, wide, ad_args(h),
                  (const ActvWords*)w, (const uint32_t*)last, (const uint32_t*)idx, a.kind, a.ctx_out, a.status_out,
                  tile_new, tile_gone, tiles));
    if (m)
        GD_TRY(launch(h, "k_actv_clear", dim3(blocks_for(m, BLOCK)), dim3(BLOCK), 0, k_actv_clear, (const ActvWords*)w,
                      (const uint32_t*)slot_of, last));
    if (a.new_idx) {
        GD_TRY(scan_device<OpAdd>(h, tile_new, tiles + 1, false, false, "actv_new"));
        GD_TRY(launch(h, "k_actv_list", gt, bt, 0, k_actv_list, (const uint8_t*)a.kind, n, wide, (const uint32_t*)tile_new,
                      tiles, (uint32_t)ACTV_CREATED, a.new_idx, n, a.n_new));
    }
    if (a.gone_idx) {
        GD_TRY(scan_device<OpAdd>(h, tile_gone, tiles + 1, false, false, "actv_gone"));
        GD_TRY(launch(h, "k_actv_list", gt, bt, 0, k_actv_list, (const uint8_t*)a.kind, n, wide,
                      (const uint32_t*)tile_gone, tiles, (uint32_t)ACTV_NONEXISTENT, a.gone_idx, n, a.n_gone));
    }
    return GD_OK;
}

// Message.IsNewPlacement of the NULL_CONTEXT frames into the handle's scratch (*out).
int frame_new_placement_device(gd_handle* h, const uint8_t* buf, uint64_t len, const uint64_t* off, const uint8_t* st,
                               uint32_t n, const uint8_t** out) {
    *out = nullptr;
    if (n == 0) return GD_OK;
    GD_TRY(ensure(h, h->actv_scr[9], (size_t)n + 16));
    uint8_t* newp = (uint8_t*)h->actv_scr[9].p;
    if (h->walk_cih)                    // GD_OPT_WALK_INVALIDATION
        GD_TRY(launch(h, "k_actv_newp_cih", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_actv_newp<true>, buf, len, off,
                      st, n, newp));
    else
        GD_TRY(launch(h, "k_actv_newp", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_actv_newp<false>, buf, len, off,
                      st, n, newp));
    *out = newp;
    return GD_OK;
}

}  // namespace gdx

extern "C" {

int gd_activate_device(gd_handle* h, const uint32_t* d_ctx, const uint8_t* d_recv_status, const gd_key* d_target_grain,
                       const gd_key* d_target_activation, const uint8_t* d_direction, const int64_t* d_ttl,
                       const uint8_t* d_new_placement, uint32_t n, uint32_t n_ctx, int terminating, uint32_t ctx_base,
                       const uint32_t* d_new_ctx, uint32_t cap_new, uint8_t* d_kind, uint32_t* d_ctx_out,
                       uint8_t* d_status_out, uint32_t* d_new_idx, uint32_t* d_n_new, uint32_t* d_gone_idx,
                       uint32_t* d_n_gone, uint32_t* d_n_proposed) {
    (void)d_target_grain;
    const ActivateArgs a{d_ctx, d_recv_status, d_target_activation, d_direction, d_ttl, d_new_placement, 0, n, n_ctx,
                         terminating, ctx_base, d_new_ctx, cap_new, d_kind, d_ctx_out, d_status_out, d_new_idx, d_n_new,
                         d_gone_idx, d_n_gone, d_n_proposed};
    GD_TRY(check_activate_args(h, a, "gd_activate_device"));
    HIP_TRY(h, hipSetDevice(h->device));
    return activate_device(h, a, false, nullptr, "gd_activate_device");
}

int gd_activate(gd_handle* h, const uint32_t* ctx, const uint8_t* recv_status, const gd_key* target_grain,
                const gd_key* target_activation, const uint8_t* direction, const int64_t* ttl,
                const uint8_t* new_placement, uint32_t n, uint32_t n_ctx, int terminating, uint32_t ctx_base,
                const uint32_t* new_ctx, uint32_t cap_new, uint8_t* out_kind, uint32_t* out_ctx, uint8_t* out_status,
                uint32_t* out_new_idx, uint32_t* out_n_new, uint32_t* out_gone_idx, uint32_t* out_n_gone,
                uint32_t* out_n_proposed) {
    (void)target_grain;
    ActivateArgs a{ctx, recv_status, target_activation, direction, ttl, new_placement, 0, n, n_ctx, terminating,
                   ctx_base, new_ctx, cap_new, out_kind, out_ctx, out_status, out_new_idx, out_n_new, out_gone_idx,
                   out_n_gone, out_n_proposed};
    GD_TRY(check_activate_args(h, a, "gd_activate"));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_activate"));
    HostStage io(h);
    a.ctx = io.in(ctx, n);
    a.recv_status = io.in(recv_status, n);
    a.target_activation = io.in(target_activation, n);
    a.direction = io.in(direction, n);
    a.ttl = io.in(ttl, n);
    a.new_placement = io.in(new_placement, n);
    a.new_ctx = io.in(new_ctx, cap_new);
    a.kind = io.out(out_kind, n, 16);
    a.ctx_out = io.out(out_ctx, n, 4);
    a.status_out = io.out(out_status, n, 16);
    // the whole lists come down (n entries at most); the host reads the first *out_n_new / *out_n_gone
    a.new_idx = io.out_if(out_new_idx, n, 4);
    a.n_new = io.out_if(out_n_new, 1);
    a.gone_idx = io.out_if(out_gone_idx, n, 4);
    a.n_gone = io.out_if(out_n_gone, 1);
    a.n_proposed = io.out(out_n_proposed, 1);
    GD_TRY(io.status());
    bool refused = false;
    GD_TRY(activate_device(h, a, true, &refused, "gd_activate"));
    GD_TRY(io.fetch());
    GD_TRY(sync_checked(h));
    if (refused)
        return set_err(h, GD_EINVAL, "gd_activate: %u proposals, cap_new %u: the batch is refused (nothing created)",
                       *out_n_proposed, cap_new);
    return GD_OK;
}

}  // extern "C"
