// eng_turns.hip -- libgraindispatch: the turn admission of a received batch: Dispatcher.ReceiveMessage
// -> ReceiveRequest per message (gd_turns.h), alone or after the receive stage.
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_turns.h"

namespace {

struct TurnOut {
    uint8_t* turn;
    uint32_t *num_running, *running_idx, *start_idx, *n_start, *wait_perm, *wait_offsets;
};

// The argument checks that need no handle state (so a caller's mistake is reported the same everywhere).
int check_turn_args(gd_handle* h, const void* ta, const void* sa, bool fused, uint32_t n, uint32_t n_ctx,
                    const gd_turn_state* s, const TurnOut& o) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (fused ? false : (ta != nullptr) != (sa != nullptr))
        return set_err(h, GD_EINVAL, "target and sending activation keys go together");
    if ((o.start_idx != nullptr) != (o.n_start != nullptr)) return set_err(h, GD_EINVAL, "start_idx and n_start go together");
    if ((o.wait_perm != nullptr) != (o.wait_offsets != nullptr))
        return set_err(h, GD_EINVAL, "wait_perm and wait_offsets go together");
    if (!s) return set_err(h, GD_EINVAL, "null turn state");
    if (n_ctx && (!s->ctx_flags || !s->num_running || !o.num_running || !o.running_idx))
        return set_err(h, GD_EINVAL, "null context array");
    if ((s->hard_limit > 0 || s->hard_limit_stateless_worker > 0) && n_ctx && !s->request_count)
        return set_err(h, GD_EINVAL, "a hard limit without request_count");
    if (n && !o.turn) return set_err(h, GD_EINVAL, "null argument");
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "turns: n > 2^31");
    if (n_ctx >= 0xFFFFFFFDu) return set_err(h, GD_EINVAL, "n_ctx too large");
    return GD_OK;
}

// The turn stage on device arrays (state's arrays device memory).  adj: the frame-fed chain's ttl age and flag
// merge, applied in the stage's own loads; the kernels without them run when there is nothing to apply.
int turns_device(gd_handle* h, const uint32_t* ctx, const uint8_t* rs, const uint8_t* dir, const int64_t* ttl,
                 const uint8_t* fwd, const uint8_t* mf, const gd_key* ta, const gd_key* sa, uint32_t n, uint32_t n_ctx,
                 const gd_turn_state* s, const TurnOut& o, TurnFrameAdj adj = TurnFrameAdj{0, nullptr, nullptr}) {
    StageTime stage(h, "stage:turns");
    const dim3 gc(blocks_for(n_ctx, BLOCK)), bc(BLOCK);
    GD_TRY(launch(h, "k_turn_init", gc, bc, 0, k_turn_init, s->num_running, n_ctx, o.num_running, o.running_idx));
    if (n == 0) {
        if (o.n_start) GD_TRY(launch(h, "k_fill", dim3(1), dim3(BLOCK), 0, k_fill_u32, o.n_start, 1u, 0u));
        if (o.wait_offsets)
            GD_TRY(launch(h, "k_fill", dim3(blocks_for(n_ctx + 2, BLOCK)), dim3(BLOCK), 0, k_fill_u32, o.wait_offsets,
                          n_ctx + 2, 0u));
        return GD_OK;
    }
    const bool limits = s->request_count && (s->hard_limit > 0 || s->hard_limit_stateless_worker > 0);
    const bool chain = s->allow_call_chain_reentrancy && ta && sa;
    const TurnArgs a{s->ctx_flags, s->num_running, limits ? s->request_count : nullptr, s->hard_limit,
                     s->hard_limit_stateless_worker, s->max_forward_count, chain ? 1u : 0u};
    const uint32_t tiles = blocks_for(n, TN_TILE);
    GD_TRY(ensure(h, h->turn_scr[0], ((size_t)tiles + 1) * 4));
    uint32_t* tile_cnt = (uint32_t*)h->turn_scr[0].p;
    uint32_t *pkey = nullptr, *rank = nullptr, *roff = nullptr, *wkey = nullptr;
    if (limits) {
        GD_TRY(ensure(h, h->turn_scr[1], (size_t)n * 4));
        GD_TRY(ensure(h, h->turn_scr[2], (size_t)n * 4 + 4));
        GD_TRY(ensure(h, h->turn_scr[3], ((size_t)n_ctx + 2) * 4));
        GD_TRY(ensure(h, h->turn_scr[4], (size_t)n * 4));
        pkey = (uint32_t*)h->turn_scr[1].p;
        roff = (uint32_t*)h->turn_scr[3].p;
        rank = (uint32_t*)h->turn_scr[4].p;
    }
    if (o.wait_perm) {
        GD_TRY(ensure(h, h->turn_scr[5], (size_t)n * 4));
        wkey = (uint32_t*)h->turn_scr[5].p;
    }
    const bool adjust = adj.ttl_age != 0 || adj.flags_or;
    const uint8_t* mf_in = mf;      // what k_turn_classify loads
    if (adj.flags_or) {             // k_turn_decide reads the Running message's flags: the merged ones, written once
        GD_TRY(ensure(h, h->turn_scr[6], (size_t)n));
        adj.flags_out = (uint8_t*)h->turn_scr[6].p;
        mf = adj.flags_out;
    }
    GD_TRY(launch(h, "k_turn_classify", dim3(tiles), dim3(TN_NT), 0,
                  adjust ? k_turn_classify<true> : k_turn_classify<false>, ctx, rs, dir, ttl, fwd, mf_in,
                  chain ? ta : nullptr, chain ? sa : nullptr, n, n_ctx, a, o.turn, o.running_idx, pkey, adj));
    // each message's place among its context's participating messages: CheckOverloaded's count (gd_turns.h)
    if (limits) GD_TRY(bucket_device(h, pkey, n, n_ctx, (uint32_t*)h->turn_scr[2].p, roff, rank));
    GD_TRY(launch(h, "k_turn_decide", dim3(tiles), dim3(TN_NT), 0, k_turn_decide, ctx, mf, n, n_ctx, a,
                  (const uint32_t*)o.running_idx, (const uint32_t*)rank, (const uint32_t*)roff, o.turn, o.num_running,
                  wkey, tile_cnt, tiles));
    GD_TRY(launch(h, "k_turn_finish", gc, bc, 0, k_turn_finish, s->ctx_flags, n_ctx, o.running_idx));
    if (o.start_idx) {
        GD_TRY(scan_device<OpAdd>(h, tile_cnt, tiles + 1, false, false, "turns"));
        const uint32_t wide = ((uintptr_t)o.turn & 15u) == 0 ? 1u : 0u;
        GD_TRY(launch(h, "k_turn_starts", dim3(tiles), dim3(TN_NT), 0, k_turn_starts, (const uint8_t*)o.turn, n, wide,
                      (const uint32_t*)tile_cnt, tiles, o.start_idx, n, o.n_start));
    }
    if (o.wait_perm) GD_TRY(bucket_device(h, wkey, n, n_ctx, o.wait_perm, o.wait_offsets));
    return GD_OK;
}

// What the caller of a frame-fed chain did not ask back is decoded into the handle's scratch; SendingActivation only
// when the call-chain test reads it.
int turn_frame_scratch(gd_handle* h, uint32_t n, bool chain, gd_frame_fields& f, gd_frame_turn_fields& t) {
    auto scratch = [&](auto*& p, int k, size_t elem) -> int {
        if (p) return GD_OK;
        GD_TRY(ensure(h, h->frt_scr[k], (size_t)n * elem + 8));
        p = (std::remove_reference_t<decltype(p)>)h->frt_scr[k].p;
        return GD_OK;
    };
    GD_TRY(scratch(f.flags, 0, 4));
    GD_TRY(scratch(f.target_grain, 1, sizeof(gd_key)));
    GD_TRY(scratch(f.target_activation, 2, sizeof(gd_key)));
    if (chain) GD_TRY(scratch(f.sending_activation, 3, sizeof(gd_key)));
    GD_TRY(scratch(f.direction, 4, 1));
    GD_TRY(scratch(t.ttl, 5, 8));
    GD_TRY(scratch(t.forward_count, 6, 1));
    GD_TRY(scratch(t.msg_flags, 7, 1));
    return GD_OK;
}

// Frames -> decode (turn headers included) -> ReceiveMessage -> ReceiveRequest, all on the handle's stream.  What
// the caller did not ask back is decoded into the handle's scratch; SendingActivation only when the call-chain
// test reads it.
int receive_turns_frames_device(gd_handle* h, const uint8_t* buf, uint64_t len, const uint64_t* off, uint32_t n,
                                uint32_t n_ctx, const gd_recv_limits* lim, const gd_frame_fields* out,
                                const gd_frame_turn_fields* turn_out, uint32_t* ctx, uint8_t* st, uint32_t* perm,
                                uint32_t* offsets, int64_t ttl_age, const uint8_t* flags_or, const gd_turn_state* s,
                                const TurnOut& o) {
    gd_frame_fields f = out ? *out : gd_frame_fields{};
    gd_frame_turn_fields t = turn_out ? *turn_out : gd_frame_turn_fields{};
    const bool chain = s->allow_call_chain_reentrancy != 0;
    if (n) GD_TRY(turn_frame_scratch(h, n, chain, f, t));
    GD_TRY(receive_frames_device(h, buf, len, off, n, n_ctx, lim, &f, ctx, st, perm, offsets, &t));
    return turns_device(h, ctx, st, f.direction, t.ttl, t.forward_count, t.msg_flags, f.target_activation,
                        chain ? f.sending_activation : nullptr, n, n_ctx, s, o, TurnFrameAdj{ttl_age, flags_or, nullptr});
}

int check_turn_frames_args(gd_handle* h, const void* buf, const void* off, uint32_t n, uint32_t n_ctx,
                           const gd_frame_fields* out, const gd_frame_turn_fields* turn_out, const void* ctx,
                           const void* st, const void* perm, const void* offsets, int64_t ttl_age,
                           const gd_turn_state* s, const TurnOut& o) {
    GD_TRY(check_turn_args(h, nullptr, nullptr, true, n, n_ctx, s, o));
    if (n && (!buf || !off || !ctx || !st)) return set_err(h, GD_EINVAL, "null argument");
    if (out && n && (!out->flags || !out->target_grain))
        return set_err(h, GD_EINVAL, "a frame-field struct needs flags and target_grain");
    if (out && (((uintptr_t)out->target_silo | (uintptr_t)out->sending_silo) & 3))
        return set_err(h, GD_EINVAL, "silo outputs must be 4-byte aligned");
    if (turn_out && (((uintptr_t)turn_out->ttl & 7) || ((uintptr_t)turn_out->resend_count & 3)))
        return set_err(h, GD_EINVAL, "ttl / resend_count outputs must be 8- / 4-byte aligned");
    if ((perm != nullptr) != (offsets != nullptr)) return set_err(h, GD_EINVAL, "perm and offsets go together");
    if (ttl_age < 0) return set_err(h, GD_EINVAL, "ttl_age_ticks < 0");
    return GD_OK;
}

// ---- the chains with the activation stage between the receive and the turn stage
// A null-context closure is enqueued with a null target: IncrementEnqueuedOnDispatcherCount never counted it
// (IncomingMessageAgent.cs:172-190), and the turn stage's closed form for EnqueueRequest's hard limit takes every
// participating message as counted.  With a limit on, the caller runs gd_activate* alone.
int check_activate_chain(gd_handle* h, const gd_turn_state* s, const gd_activate_io* act, uint32_t n, const char* call) {
    if (!act) return set_err(h, GD_EINVAL, "%s: null gd_activate_io", call);
    if (s->hard_limit > 0 || s->hard_limit_stateless_worker > 0)
        return set_err(h, GD_EINVAL, "%s: a hard limit is set (the resolved messages were never counted); use gd_activate",
                       call);
    if (n && !act->kind) return set_err(h, GD_EINVAL, "%s: null kind", call);
    return GD_OK;
}

ActivateArgs activate_chain_args(const gd_activate_io* act, uint32_t* ctx, uint8_t* st, const gd_key* ta,
                                 const uint8_t* dir, const int64_t* ttl, int64_t ttl_age, const uint8_t* newp, uint32_t n,
                                 uint32_t n_ctx) {
    return ActivateArgs{ctx, st, ta, dir, ttl, newp, ttl_age, n, n_ctx, act->terminating, act->ctx_base, act->new_ctx,
                        act->cap_new, act->kind, ctx, st, act->new_idx, act->n_new, act->gone_idx, act->n_gone,
                        act->n_proposed};
}

// receive -> activate (in place on ctx / st) -> the bucketing of the resolved contexts -> turns.
int receive_activate_turns_device(gd_handle* h, const gd_key* tg, const gd_key* ta, const uint8_t* dir, uint32_t n,
                                  uint32_t n_ctx, const gd_recv_limits* lim, uint32_t* ctx, uint8_t* st, uint32_t* perm,
                                  uint32_t* offsets, const int64_t* ttl, const uint8_t* fwd, const uint8_t* mf,
                                  const gd_key* sa, const gd_turn_state* s, const TurnOut& o, const gd_activate_io* act,
                                  bool host_form, bool* refused, const char* call) {
    GD_TRY(receive_device(h, tg, ta, dir, nullptr, n, n_ctx, lim, ctx, st, nullptr, nullptr));
    const ActivateArgs a = activate_chain_args(act, ctx, st, ta, dir, ttl, 0, act->new_placement, n, n_ctx);
    GD_TRY(check_activate_args(h, a, call));
    GD_TRY(activate_device(h, a, host_form, refused, call));
    if (perm) GD_TRY(bucket_device(h, ctx, n, n_ctx + 1, perm, offsets));
    return turns_device(h, ctx, st, dir, ttl, fwd, mf, ta, sa, n, n_ctx, s, o);
}

int receive_activate_turns_frames_device(gd_handle* h, const uint8_t* buf, uint64_t len, const uint64_t* off, uint32_t n,
                                         uint32_t n_ctx, const gd_recv_limits* lim, const gd_frame_fields* out,
                                         const gd_frame_turn_fields* turn_out, uint32_t* ctx, uint8_t* st, uint32_t* perm,
                                         uint32_t* offsets, int64_t ttl_age, const uint8_t* flags_or,
                                         const gd_turn_state* s, const TurnOut& o, const gd_activate_io* act,
                                         bool host_form, bool* refused, const char* call) {
    gd_frame_fields f = out ? *out : gd_frame_fields{};
    gd_frame_turn_fields t = turn_out ? *turn_out : gd_frame_turn_fields{};
    const bool chain = s->allow_call_chain_reentrancy != 0;
    if (n) GD_TRY(turn_frame_scratch(h, n, chain, f, t));
    GD_TRY(receive_frames_device(h, buf, len, off, n, n_ctx, lim, &f, ctx, st, nullptr, nullptr, &t));
    const uint8_t* newp = nullptr;
    GD_TRY(frame_new_placement_device(h, buf, len, off, st, n, &newp));
    const ActivateArgs a = activate_chain_args(act, ctx, st, f.target_activation, f.direction, t.ttl, ttl_age, newp, n, n_ctx);
    GD_TRY(check_activate_args(h, a, call));
    GD_TRY(activate_device(h, a, host_form, refused, call));
    if (perm) GD_TRY(bucket_device(h, ctx, n, n_ctx + 1, perm, offsets));
    return turns_device(h, ctx, st, f.direction, t.ttl, t.forward_count, t.msg_flags, f.target_activation,
                        chain ? f.sending_activation : nullptr, n, n_ctx, s, o, TurnFrameAdj{ttl_age, flags_or, nullptr});
}

// The activation stage's arrays of a host-form chain: inputs up, room for the outputs.
gd_activate_io stage_activate_io(HostStage& io, const gd_activate_io* act, uint32_t n) {
    gd_activate_io d = *act;
    d.new_placement = io.in(act->new_placement, n);
    d.new_ctx = io.in(act->new_ctx, act->cap_new);
    d.kind = io.out(act->kind, n, 16);
    d.new_idx = io.out_if(act->new_idx, n, 4);
    d.n_new = io.out_if(act->n_new, 1);
    d.gone_idx = io.out_if(act->gone_idx, n, 4);
    d.n_gone = io.out_if(act->n_gone, 1);
    d.n_proposed = io.out(act->n_proposed, 1);
    return d;
}

int activate_chain_end(gd_handle* h, HostStage& io, bool refused, const gd_activate_io* act, const char* call) {
    GD_TRY(io.fetch());
    GD_TRY(sync_checked(h));
    if (refused)
        return set_err(h, GD_EINVAL, "%s: %u proposals, cap_new %u: the batch is refused (nothing created)", call,
                       *act->n_proposed, act->cap_new);
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_turns_device(gd_handle* h, const uint32_t* d_ctx, const uint8_t* d_recv_status, const uint8_t* d_direction,
                    const int64_t* d_ttl, const uint8_t* d_forward_count, const uint8_t* d_msg_flags,
                    const gd_key* d_target_activation, const gd_key* d_sending_activation, uint32_t n, uint32_t n_ctx,
                    const gd_turn_state* state, uint8_t* d_turn, uint32_t* d_num_running_out, uint32_t* d_running_idx,
                    uint32_t* d_start_idx, uint32_t* d_n_start, uint32_t* d_wait_perm, uint32_t* d_wait_offsets) {
    const TurnOut o{d_turn, d_num_running_out, d_running_idx, d_start_idx, d_n_start, d_wait_perm, d_wait_offsets};
    GD_TRY(check_turn_args(h, d_target_activation, d_sending_activation, false, n, n_ctx, state, o));
    if (n && !d_ctx) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_turns_device"));
    return turns_device(h, d_ctx, d_recv_status, d_direction, d_ttl, d_forward_count, d_msg_flags, d_target_activation,
                        d_sending_activation, n, n_ctx, state, o);
}

int gd_turns(gd_handle* h, const uint32_t* ctx, const uint8_t* recv_status, const uint8_t* direction,
             const int64_t* ttl, const uint8_t* forward_count, const uint8_t* msg_flags,
             const gd_key* target_activation, const gd_key* sending_activation, uint32_t n, uint32_t n_ctx,
             const gd_turn_state* state, uint8_t* out_turn, uint32_t* out_num_running, uint32_t* out_running_idx,
             uint32_t* out_start_idx, uint32_t* out_n_start, uint32_t* out_wait_perm, uint32_t* out_wait_offsets) {
    const TurnOut ho{out_turn, out_num_running, out_running_idx, out_start_idx, out_n_start, out_wait_perm,
                     out_wait_offsets};
    GD_TRY(check_turn_args(h, target_activation, sending_activation, false, n, n_ctx, state, ho));
    if (n && !ctx) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_turns"));
    HostStage io(h);
    const uint32_t* dctx = io.in(ctx, n);
    const uint8_t* drs = io.in(recv_status, n);
    const uint8_t* ddir = io.in(direction, n);
    const int64_t* dttl = io.in(ttl, n);
    const uint8_t* dfwd = io.in(forward_count, n);
    const uint8_t* dmf = io.in(msg_flags, n);
    const gd_key* dta = io.in(target_activation, n);
    const gd_key* dsa = io.in(sending_activation, n);
    gd_turn_state ds = *state;
    ds.ctx_flags = io.in(state->ctx_flags, n_ctx);
    ds.num_running = io.in(state->num_running, n_ctx);
    ds.request_count = io.in(state->request_count, n_ctx);
    TurnOut o;
    o.turn = io.out(out_turn, n, 16);
    o.num_running = io.out(out_num_running, n_ctx, 4);
    o.running_idx = io.out(out_running_idx, n_ctx, 4);
    // the whole start list comes down (n entries at most); the host reads the first *out_n_start
    o.start_idx = io.out_if(out_start_idx, n, 4);
    o.n_start = io.out_if(out_n_start, 1);
    o.wait_perm = io.out_if(out_wait_perm, n, 4);
    o.wait_offsets = io.out_if(out_wait_offsets, (size_t)n_ctx + 2);
    GD_TRY(io.status());
    GD_TRY(turns_device(h, dctx, drs, ddir, dttl, dfwd, dmf, dta, dsa, n, n_ctx, &ds, o));
    GD_TRY(io.fetch());
    return sync_checked(h);
}

int gd_receive_turns_device(gd_handle* h, const gd_key* d_target_grain, const gd_key* d_target_activation,
                            const uint8_t* d_direction, uint32_t n, uint32_t n_ctx, const gd_recv_limits* recv_limits,
                            uint32_t* d_ctx, uint8_t* d_status, uint32_t* d_perm, uint32_t* d_offsets,
                            const int64_t* d_ttl, const uint8_t* d_forward_count, const uint8_t* d_msg_flags,
                            const gd_key* d_sending_activation, const gd_turn_state* state, uint8_t* d_turn,
                            uint32_t* d_num_running_out, uint32_t* d_running_idx, uint32_t* d_start_idx,
                            uint32_t* d_n_start, uint32_t* d_wait_perm, uint32_t* d_wait_offsets) {
    const TurnOut o{d_turn, d_num_running_out, d_running_idx, d_start_idx, d_n_start, d_wait_perm, d_wait_offsets};
    GD_TRY(check_turn_args(h, d_target_activation, d_sending_activation, true, n, n_ctx, state, o));
    if (n && (!d_target_grain || !d_target_activation || !d_ctx || !d_status))
        return set_err(h, GD_EINVAL, "null argument");
    if ((d_perm != nullptr) != (d_offsets != nullptr)) return set_err(h, GD_EINVAL, "perm and offsets go together");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_receive_turns_device"));
    GD_TRY(receive_device(h, d_target_grain, d_target_activation, d_direction, nullptr, n, n_ctx, recv_limits, d_ctx,
                          d_status, d_perm, d_offsets));
    return turns_device(h, d_ctx, d_status, d_direction, d_ttl, d_forward_count, d_msg_flags, d_target_activation,
                        d_sending_activation, n, n_ctx, state, o);
}

int gd_receive_turns_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                                   uint32_t n, uint32_t n_ctx, const gd_recv_limits* recv_limits,
                                   const gd_frame_fields* d_out, const gd_frame_turn_fields* d_turn_out,
                                   uint32_t* d_ctx, uint8_t* d_status, uint32_t* d_perm, uint32_t* d_offsets,
                                   int64_t ttl_age_ticks, const uint8_t* d_msg_flags_or, const gd_turn_state* state,
                                   uint8_t* d_turn, uint32_t* d_num_running_out, uint32_t* d_running_idx,
                                   uint32_t* d_start_idx, uint32_t* d_n_start, uint32_t* d_wait_perm,
                                   uint32_t* d_wait_offsets) {
    const TurnOut o{d_turn, d_num_running_out, d_running_idx, d_start_idx, d_n_start, d_wait_perm, d_wait_offsets};
    GD_TRY(check_turn_frames_args(h, d_buf, d_frame_off, n, n_ctx, d_out, d_turn_out, d_ctx, d_status, d_perm,
                                  d_offsets, ttl_age_ticks, state, o));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_receive_turns_frames_device"));
    return receive_turns_frames_device(h, d_buf, buf_len, d_frame_off, n, n_ctx, recv_limits, d_out, d_turn_out, d_ctx,
                                       d_status, d_perm, d_offsets, ttl_age_ticks, d_msg_flags_or, state, o);
}

int gd_receive_turns_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                            uint32_t n_ctx, const gd_recv_limits* recv_limits, const gd_frame_fields* out,
                            const gd_frame_turn_fields* turn_out, uint32_t* out_ctx, uint8_t* out_status,
                            uint32_t* out_perm, uint32_t* out_offsets, int64_t ttl_age_ticks,
                            const uint8_t* msg_flags_or, const gd_turn_state* state, uint8_t* out_turn,
                            uint32_t* out_num_running, uint32_t* out_running_idx, uint32_t* out_start_idx,
                            uint32_t* out_n_start, uint32_t* out_wait_perm, uint32_t* out_wait_offsets) {
    const TurnOut ho{out_turn, out_num_running, out_running_idx, out_start_idx, out_n_start, out_wait_perm,
                     out_wait_offsets};
    GD_TRY(check_turn_frames_args(h, buf, frame_off, n, n_ctx, out, turn_out, out_ctx, out_status, out_perm, out_offsets,
                                  ttl_age_ticks, state, ho));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_receive_turns_frames"));
    HostStage io(h);
    const uint8_t* dbuf = io.in(buf, n ? (size_t)buf_len : 0);
    const uint64_t* doff = io.in(frame_off, n);
    gd_recv_limits dl{};
    const gd_recv_limits* pl = nullptr;
    const uint32_t* drc = io.in(recv_limits ? recv_limits->request_count : nullptr, n_ctx);
    if (drc) {
        dl = *recv_limits;
        dl.request_count = drc;
        pl = &dl;
    }
    gd_frame_fields dev{};
    gd_frame_turn_fields tdev{};
    stage_frame_outputs(io, n, out, turn_out, &dev, &tdev);
    uint32_t* dctx = io.out(out_ctx, n, 8);
    uint8_t* dst = io.out(out_status, n, 8);
    uint32_t* dperm = io.out_if(out_perm, n, 8);
    uint32_t* doffs = io.out_if(out_offsets, (size_t)n_ctx + 3);
    const uint8_t* dmor = io.in(msg_flags_or, n);
    gd_turn_state ds = *state;
    ds.ctx_flags = io.in(state->ctx_flags, n_ctx);
    ds.num_running = io.in(state->num_running, n_ctx);
    ds.request_count = io.in(state->request_count, n_ctx);
    TurnOut o;
    o.turn = io.out(out_turn, n, 16);
    o.num_running = io.out(out_num_running, n_ctx, 4);
    o.running_idx = io.out(out_running_idx, n_ctx, 4);
    o.start_idx = io.out_if(out_start_idx, n, 4);
    o.n_start = io.out_if(out_n_start, 1);
    o.wait_perm = io.out_if(out_wait_perm, n, 4);
    o.wait_offsets = io.out_if(out_wait_offsets, (size_t)n_ctx + 2);
    GD_TRY(io.status());
    GD_TRY(receive_turns_frames_device(h, dbuf, buf_len, doff, n, n_ctx, pl, &dev, &tdev, dctx, dst, dperm, doffs,
                                       ttl_age_ticks, dmor, &ds, o));
    GD_TRY(io.fetch());
    return sync_checked(h);
}

int gd_receive_activate_turns_device(gd_handle* h, const gd_key* d_target_grain, const gd_key* d_target_activation,
                                     const uint8_t* d_direction, uint32_t n, uint32_t n_ctx,
                                     const gd_recv_limits* recv_limits, uint32_t* d_ctx, uint8_t* d_status,
                                     uint32_t* d_perm, uint32_t* d_offsets, const int64_t* d_ttl,
                                     const uint8_t* d_forward_count, const uint8_t* d_msg_flags,
                                     const gd_key* d_sending_activation, const gd_turn_state* state, uint8_t* d_turn,
                                     uint32_t* d_num_running_out, uint32_t* d_running_idx, uint32_t* d_start_idx,
                                     uint32_t* d_n_start, uint32_t* d_wait_perm, uint32_t* d_wait_offsets,
                                     const gd_activate_io* d_act) {
    const TurnOut o{d_turn, d_num_running_out, d_running_idx, d_start_idx, d_n_start, d_wait_perm, d_wait_offsets};
    GD_TRY(check_turn_args(h, d_target_activation, d_sending_activation, true, n, n_ctx, state, o));
    GD_TRY(check_activate_chain(h, state, d_act, n, "gd_receive_activate_turns_device"));
    if (n && (!d_target_grain || !d_target_activation || !d_ctx || !d_status))
        return set_err(h, GD_EINVAL, "null argument");
    if ((d_perm != nullptr) != (d_offsets != nullptr)) return set_err(h, GD_EINVAL, "perm and offsets go together");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_receive_activate_turns_device"));
    return receive_activate_turns_device(h, d_target_grain, d_target_activation, d_direction, n, n_ctx, recv_limits, d_ctx,
                                         d_status, d_perm, d_offsets, d_ttl, d_forward_count, d_msg_flags,
                                         d_sending_activation, state, o, d_act, false, nullptr,
                                         "gd_receive_activate_turns_device");
}

int gd_receive_activate_turns(gd_handle* h, const gd_key* target_grain, const gd_key* target_activation,
                              const uint8_t* direction, uint32_t n, uint32_t n_ctx, const gd_recv_limits* recv_limits,
                              uint32_t* out_ctx, uint8_t* out_status, uint32_t* out_perm, uint32_t* out_offsets,
                              const int64_t* ttl, const uint8_t* forward_count, const uint8_t* msg_flags,
                              const gd_key* sending_activation, const gd_turn_state* state, uint8_t* out_turn,
                              uint32_t* out_num_running, uint32_t* out_running_idx, uint32_t* out_start_idx,
                              uint32_t* out_n_start, uint32_t* out_wait_perm, uint32_t* out_wait_offsets,
                              const gd_activate_io* act) {
    const TurnOut ho{out_turn, out_num_running, out_running_idx, out_start_idx, out_n_start, out_wait_perm,
                     out_wait_offsets};
    GD_TRY(check_turn_args(h, target_activation, sending_activation, true, n, n_ctx, state, ho));
    GD_TRY(check_activate_chain(h, state, act, n, "gd_receive_activate_turns"));
    if (n && (!target_grain || !target_activation || !out_ctx || !out_status)) return set_err(h, GD_EINVAL, "null argument");
    if ((out_perm != nullptr) != (out_offsets != nullptr)) return set_err(h, GD_EINVAL, "perm and offsets go together");
    if (!act->n_proposed) return set_err(h, GD_EINVAL, "gd_receive_activate_turns: null n_proposed");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_receive_activate_turns"));
    HostStage io(h);
    const gd_key* dtg = io.in(target_grain, n);
    const gd_key* dta = io.in(target_activation, n);
    const uint8_t* ddir = io.in(direction, n);
    gd_recv_limits dl{};
    const gd_recv_limits* pl = nullptr;
    const uint32_t* drc = io.in(recv_limits ? recv_limits->request_count : nullptr, n_ctx);
    if (drc) {
        dl = *recv_limits;
        dl.request_count = drc;
        pl = &dl;
    }
    uint32_t* dctx = io.out(out_ctx, n, 8);
    uint8_t* dst = io.out(out_status, n, 16);
    uint32_t* dperm = io.out_if(out_perm, n, 8);
    uint32_t* doffs = io.out_if(out_offsets, (size_t)n_ctx + 3);
    const int64_t* dttl = io.in(ttl, n);
    const uint8_t* dfwd = io.in(forward_count, n);
    const uint8_t* dmf = io.in(msg_flags, n);
    const gd_key* dsa = io.in(sending_activation, n);
    gd_turn_state ds = *state;
    ds.ctx_flags = io.in(state->ctx_flags, n_ctx);
    ds.num_running = io.in(state->num_running, n_ctx);
    ds.request_count = io.in(state->request_count, n_ctx);
    TurnOut o;
    o.turn = io.out(out_turn, n, 16);
    o.num_running = io.out(out_num_running, n_ctx, 4);
    o.running_idx = io.out(out_running_idx, n_ctx, 4);
    o.start_idx = io.out_if(out_start_idx, n, 4);
    o.n_start = io.out_if(out_n_start, 1);
    o.wait_perm = io.out_if(out_wait_perm, n, 4);
    o.wait_offsets = io.out_if(out_wait_offsets, (size_t)n_ctx + 2);
    const gd_activate_io da = stage_activate_io(io, act, n);
    GD_TRY(io.status());
    bool refused = false;
    GD_TRY(receive_activate_turns_device(h, dtg, dta, ddir, n, n_ctx, pl, dctx, dst, dperm, doffs, dttl, dfwd, dmf, dsa,
                                         &ds, o, &da, true, &refused, "gd_receive_activate_turns"));
    return activate_chain_end(h, io, refused, act, "gd_receive_activate_turns");
}

int gd_receive_activate_turns_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len,
                                            const uint64_t* d_frame_off, uint32_t n, uint32_t n_ctx,
                                            const gd_recv_limits* recv_limits, const gd_frame_fields* d_out,
                                            const gd_frame_turn_fields* d_turn_out, uint32_t* d_ctx, uint8_t* d_status,
                                            uint32_t* d_perm, uint32_t* d_offsets, int64_t ttl_age_ticks,
                                            const uint8_t* d_msg_flags_or, const gd_turn_state* state, uint8_t* d_turn,
                                            uint32_t* d_num_running_out, uint32_t* d_running_idx, uint32_t* d_start_idx,
                                            uint32_t* d_n_start, uint32_t* d_wait_perm, uint32_t* d_wait_offsets,
                                            const gd_activate_io* d_act) {
    const TurnOut o{d_turn, d_num_running_out, d_running_idx, d_start_idx, d_n_start, d_wait_perm, d_wait_offsets};
    GD_TRY(check_turn_frames_args(h, d_buf, d_frame_off, n, n_ctx, d_out, d_turn_out, d_ctx, d_status, d_perm,
                                  d_offsets, ttl_age_ticks, state, o));
    GD_TRY(check_activate_chain(h, state, d_act, n, "gd_receive_activate_turns_frames_device"));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_receive_activate_turns_frames_device"));
    return receive_activate_turns_frames_device(h, d_buf, buf_len, d_frame_off, n, n_ctx, recv_limits, d_out, d_turn_out,
                                                d_ctx, d_status, d_perm, d_offsets, ttl_age_ticks, d_msg_flags_or, state,
                                                o, d_act, false, nullptr, "gd_receive_activate_turns_frames_device");
}

int gd_receive_activate_turns_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off,
                                     uint32_t n, uint32_t n_ctx, const gd_recv_limits* recv_limits,
                                     const gd_frame_fields* out, const gd_frame_turn_fields* turn_out, uint32_t* out_ctx,
                                     uint8_t* out_status, uint32_t* out_perm, uint32_t* out_offsets,
                                     int64_t ttl_age_ticks, const uint8_t* msg_flags_or, const gd_turn_state* state,
                                     uint8_t* out_turn, uint32_t* out_num_running, uint32_t* out_running_idx,
                                     uint32_t* out_start_idx, uint32_t* out_n_start, uint32_t* out_wait_perm,
                                     uint32_t* out_wait_offsets, const gd_activate_io* act) {
    const TurnOut ho{out_turn, out_num_running, out_running_idx, out_start_idx, out_n_start, out_wait_perm,
                     out_wait_offsets};
    GD_TRY(check_turn_frames_args(h, buf, frame_off, n, n_ctx, out, turn_out, out_ctx, out_status, out_perm, out_offsets,
                                  ttl_age_ticks, state, ho));
    GD_TRY(check_activate_chain(h, state, act, n, "gd_receive_activate_turns_frames"));
    if (!act->n_proposed) return set_err(h, GD_EINVAL, "gd_receive_activate_turns_frames: null n_proposed");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_receive_activate_turns_frames"));
    HostStage io(h);
    const uint8_t* dbuf = io.in(buf, n ? (size_t)buf_len : 0);
    const uint64_t* doff = io.in(frame_off, n);
    gd_recv_limits dl{};
    const gd_recv_limits* pl = nullptr;
    const uint32_t* drc = io.in(recv_limits ? recv_limits->request_count : nullptr, n_ctx);
    if (drc) {
        dl = *recv_limits;
        dl.request_count = drc;
        pl = &dl;
    }
    gd_frame_fields dev{};
    gd_frame_turn_fields tdev{};
    stage_frame_outputs(io, n, out, turn_out, &dev, &tdev);
    uint32_t* dctx = io.out(out_ctx, n, 8);
    uint8_t* dst = io.out(out_status, n, 16);
    uint32_t* dperm = io.out_if(out_perm, n, 8);
    uint32_t* doffs = io.out_if(out_offsets, (size_t)n_ctx + 3);
    const uint8_t* dmor = io.in(msg_flags_or, n);
    gd_turn_state ds = *state;
    ds.ctx_flags = io.in(state->ctx_flags, n_ctx);
    ds.num_running = io.in(state->num_running, n_ctx);
    ds.request_count = io.in(state->request_count, n_ctx);
    TurnOut o;
    o.turn = io.out(out_turn, n, 16);
    o.num_running = io.out(out_num_running, n_ctx, 4);
    o.running_idx = io.out(out_running_idx, n_ctx, 4);
    o.start_idx = io.out_if(out_start_idx, n, 4);
    o.n_start = io.out_if(out_n_start, 1);
    o.wait_perm = io.out_if(out_wait_perm, n, 4);
    o.wait_offsets = io.out_if(out_wait_offsets, (size_t)n_ctx + 2);
    const gd_activate_io da = stage_activate_io(io, act, n);
    GD_TRY(io.status());
    bool refused = false;
    GD_TRY(receive_activate_turns_frames_device(h, dbuf, buf_len, doff, n, n_ctx, pl, &dev, &tdev, dctx, dst, dperm,
                                                doffs, ttl_age_ticks, dmor, &ds, o, &da, true, &refused,
                                                "gd_receive_activate_turns_frames"));
    return activate_chain_end(h, io, refused, act, "gd_receive_activate_turns_frames");
}

}  // extern "C"
