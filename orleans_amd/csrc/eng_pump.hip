// eng_pump.hip -- libgraindispatch: the turn completion and message pump of a batch of completions, and the
// wait-list merge that keeps the waiting lists' CSR between steps (gd_pump.h):
// Dispatcher.OnActivationCompletedRequest -> ResetRunning -> RunMessagePump per completed request.
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_pump.h"

namespace {

struct PumpOut {
    uint8_t* ctx_flags;
    uint32_t *num_running, *n_dequeued, *running_pos;
    uint8_t* event;
    uint32_t *n_started_by, *start_pos, *n_start;
};

// The argument checks that need no handle state, as check_turn_args reports them.
int check_complete_args(gd_handle* h, const void* done_ctx, uint32_t n_done, uint32_t n_ctx, const void* ctx_flags,
                        const void* num_running, const gd_wait_list* wait, uint32_t wait_cap, const PumpOut& o) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if ((o.start_pos != nullptr) != (o.n_start != nullptr)) return set_err(h, GD_EINVAL, "start_pos and n_start go together");
    if (!wait) return set_err(h, GD_EINVAL, "null wait list");
    if (n_ctx && (!ctx_flags || !num_running || !wait->offsets || !o.ctx_flags || !o.num_running || !o.n_dequeued ||
                  !o.running_pos || !o.event))
        return set_err(h, GD_EINVAL, "null context array");
    if (n_ctx && wait_cap && !wait->flags) return set_err(h, GD_EINVAL, "null wait-list flags");
    if (n_done && !done_ctx) return set_err(h, GD_EINVAL, "null argument");
    if (n_done > (1u << 31)) return set_err(h, GD_EINVAL, "turns_complete: n_done > 2^31");
    if (n_ctx >= 0xFFFFFFFDu) return set_err(h, GD_EINVAL, "n_ctx too large");
    return GD_OK;
}

int check_merge_args(gd_handle* h, const gd_wait_list* old_list, uint32_t n_ctx, const void* wperm, const void* woff,
                     uint32_t n, const void* ta, const void* sa, uint32_t cap, const void* off_out, const void* msg_out,
                     const void* flags_out, const void* total) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if ((ta != nullptr) != (sa != nullptr)) return set_err(h, GD_EINVAL, "target and sending activation keys go together");
    if (old_list && old_list->offsets && (!old_list->msg || !old_list->flags))
        return set_err(h, GD_EINVAL, "an old list without msg or flags");
    if (!off_out || !total || !woff) return set_err(h, GD_EINVAL, "null argument");
    if (n && !wperm) return set_err(h, GD_EINVAL, "null argument");
    if (cap && (!msg_out || !flags_out)) return set_err(h, GD_EINVAL, "null output list");
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "wait_list_merge: n > 2^31");
    if (n_ctx >= 0xFFFFFFFDu) return set_err(h, GD_EINVAL, "n_ctx too large");
    return GD_OK;
}

// The completion stage on device arrays.
int complete_device(gd_handle* h, const uint32_t* done_ctx, const uint8_t* done_flags, uint32_t n_done, uint32_t n_ctx,
                    const uint8_t* ctx_flags, const uint32_t* num_running, const uint32_t* woff, const uint8_t* wflags,
                    uint32_t wait_cap, const PumpOut& o) {
    StageTime stage(h, "stage:pump");
    DevBuf* S = h->pump_scr;
    const bool starts = o.start_pos != nullptr;
    const bool work = n_done && n_ctx;
    uint32_t *cnt = nullptr, *first = nullptr;
    if (starts) {
        GD_TRY(ensure(h, S[2], ((size_t)n_done + 1) * 4));
        GD_TRY(ensure(h, S[3], ((size_t)n_done + 1) * 4));
        cnt = (uint32_t*)S[2].p;
        first = (uint32_t*)S[3].p;
        HIP_TRY(h, hipMemsetAsync(cnt, 0, ((size_t)n_done + 1) * 4, h->stream));
    } else if (o.n_started_by && n_done) {
        cnt = o.n_started_by;
        HIP_TRY(h, hipMemsetAsync(cnt, 0, (size_t)n_done * 4, h->stream));
    }
    if (n_ctx) {
        PumpArgs a{nullptr, nullptr, done_flags, ctx_flags, num_running, woff, wflags, wait_cap, n_ctx, o.ctx_flags,
                   o.num_running, o.n_dequeued, o.running_pos, o.event, cnt, first};
        // a context on the work list holds at least PUMP_THIN completions + list entries
        const uint32_t work_cap =
            (uint32_t)std::min<uint64_t>(n_ctx, ((uint64_t)n_done + wait_cap) / PUMP_THIN);
        GD_TRY(ensure(h, S[4], ((size_t)work_cap + 1) * 4));
        GD_TRY(ensure(h, S[5], 4));
        uint32_t* wl = (uint32_t*)S[4].p;
        uint32_t* n_work = (uint32_t*)S[5].p;
        if (work) {
            GD_TRY(ensure(h, S[0], (size_t)n_done * 4));
            GD_TRY(ensure(h, S[1], ((size_t)n_ctx + 2) * 4));
            // each context's completions in arrival order (the key is clamped to n_ctx by the bucketing)
            GD_TRY(bucket_device(h, done_ctx, n_done, n_ctx, (uint32_t*)S[0].p, (uint32_t*)S[1].p));
            a.bperm = (const uint32_t*)S[0].p;
            a.boff = (const uint32_t*)S[1].p;
            HIP_TRY(h, hipMemsetAsync(n_work, 0, 4, h->stream));
        }
        GD_TRY(launch(h, "k_pump_ctx", dim3(blocks_for(n_ctx, BLOCK)), dim3(BLOCK), 0, k_pump_ctx, a, wl, n_work, work_cap));
        if (work && work_cap) {
            const uint32_t grid = std::min<uint32_t>(blocks_for(work_cap, PUMP_WAVE_NW), h->n_cu * 8u);
            GD_TRY(launch(h, "k_pump_wave", dim3(grid), dim3(PUMP_WAVE_NT), 0, k_pump_wave, a, (const uint32_t*)wl,
                          (const uint32_t*)n_work, work_cap));
        }
    }
    if (starts) {
        if (o.n_started_by && n_done)
            HIP_TRY(h, hipMemcpyAsync(o.n_started_by, cnt, (size_t)n_done * 4, hipMemcpyDeviceToDevice, h->stream));
        GD_TRY(scan_device<OpAdd>(h, cnt, n_done + 1, false, false, "pump"));
        const uint32_t grid = std::max<uint32_t>(1u, blocks_for(wait_cap, PUMP_START_TILE));
        GD_TRY(launch(h, "k_pump_starts", dim3(grid), dim3(PUMP_START_NT), 0, k_pump_starts, (const uint32_t*)cnt,
                      (const uint32_t*)first, n_done, o.start_pos, wait_cap, o.n_start));
    }
    return GD_OK;
}

int merge_device(gd_handle* h, const MergeArgs& a, uint32_t* off_out, uint32_t* msg_out, uint8_t* flags_out,
                 uint32_t* total) {
    StageTime stage(h, "stage:wait_merge");
    GD_TRY(launch(h, "k_merge_count", dim3(blocks_for((uint64_t)a.n_ctx + 1, BLOCK)), dim3(BLOCK), 0, k_merge_count, a,
                  off_out));
    GD_TRY(scan_device<OpAdd>(h, off_out, a.n_ctx + 1, false, false, "merge"));
    // the total is a device word: a grid that covers the capacity, capped, strides over what there is
    const uint32_t grid = std::max<uint32_t>(1u, std::min<uint32_t>(blocks_for(a.cap, BLOCK), h->n_cu * 16u));
    return launch(h, "k_merge_copy", dim3(grid), dim3(BLOCK), 0, k_merge_copy, a, (const uint32_t*)off_out, msg_out,
                  flags_out, total);
}

}  // namespace

extern "C" {

int gd_turns_complete_device(gd_handle* h, const uint32_t* d_done_ctx, const uint8_t* d_done_flags, uint32_t n_done,
                             uint32_t n_ctx, const uint8_t* d_ctx_flags, const uint32_t* d_num_running,
                             const gd_wait_list* wait, uint32_t wait_cap, uint8_t* d_ctx_flags_out,
                             uint32_t* d_num_running_out, uint32_t* d_n_dequeued, uint32_t* d_running_pos,
                             uint8_t* d_event, uint32_t* d_n_started_by, uint32_t* d_start_pos, uint32_t* d_n_start) {
    const PumpOut o{d_ctx_flags_out, d_num_running_out, d_n_dequeued, d_running_pos,
                    d_event,         d_n_started_by,    d_start_pos,  d_n_start};
    GD_TRY(check_complete_args(h, d_done_ctx, n_done, n_ctx, d_ctx_flags, d_num_running, wait, wait_cap, o));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_turns_complete_device"));
    return complete_device(h, d_done_ctx, d_done_flags, n_done, n_ctx, d_ctx_flags, d_num_running, wait->offsets,
                           wait->flags, wait_cap, o);
}

int gd_turns_complete(gd_handle* h, const uint32_t* done_ctx, const uint8_t* done_flags, uint32_t n_done,
                      uint32_t n_ctx, const uint8_t* ctx_flags, const uint32_t* num_running, const gd_wait_list* wait,
                      uint32_t wait_cap, uint8_t* out_ctx_flags, uint32_t* out_num_running, uint32_t* out_n_dequeued,
                      uint32_t* out_running_pos, uint8_t* out_event, uint32_t* out_n_started_by,
                      uint32_t* out_start_pos, uint32_t* out_n_start) {
    const PumpOut ho{out_ctx_flags,    out_num_running, out_n_dequeued, out_running_pos, out_event,
                     out_n_started_by, out_start_pos,   out_n_start};
    GD_TRY(check_complete_args(h, done_ctx, n_done, n_ctx, ctx_flags, num_running, wait, wait_cap, ho));
    const uint32_t total = n_ctx ? wait->offsets[n_ctx] : 0u;
    if (total > wait_cap) return set_err(h, GD_EINVAL, "wait list longer than wait_cap");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_turns_complete"));
    HostStage io(h);
    const uint32_t* dctx = io.in(done_ctx, n_done);
    const uint8_t* ddf = io.in(done_flags, n_done);
    const uint8_t* dfl = io.in(ctx_flags, n_ctx);
    const uint32_t* dnr = io.in(num_running, n_ctx);
    const uint32_t* dwoff = io.in(n_ctx ? wait->offsets : nullptr, (size_t)n_ctx + 1);
    const uint8_t* dwf = io.in(total ? wait->flags : nullptr, total);
    PumpOut o;
    o.ctx_flags = io.out(out_ctx_flags, n_ctx, 16);
    o.num_running = io.out(out_num_running, n_ctx, 4);
    o.n_dequeued = io.out(out_n_dequeued, n_ctx, 4);
    o.running_pos = io.out(out_running_pos, n_ctx, 4);
    o.event = io.out(out_event, n_ctx, 16);
    o.n_started_by = io.out_if(out_n_started_by, n_done, 4);
    // the whole start list comes down (offsets[n_ctx] entries at most); the host reads the first *out_n_start
    o.start_pos = io.out_if(out_start_pos, total, 4);
    o.n_start = io.out_if(out_n_start, 1);
    GD_TRY(io.status());
    // the list's own length is the device form's capacity: nothing past it can start
    GD_TRY(complete_device(h, dctx, ddf, n_done, n_ctx, dfl, dnr, dwoff, dwf, total, o));
    GD_TRY(io.fetch());
    return sync_checked(h);
}

int gd_wait_list_merge_device(gd_handle* h, const gd_wait_list* old_list, const uint32_t* d_n_dequeued, uint32_t n_ctx,
                              const uint32_t* d_wait_perm, const uint32_t* d_wait_offsets, uint32_t n,
                              const uint32_t* d_msg_id, uint32_t id_base, const uint8_t* d_msg_flags,
                              const gd_key* d_target_activation, const gd_key* d_sending_activation,
                              int allow_call_chain_reentrancy, uint32_t cap, uint32_t* d_offsets_out,
                              uint32_t* d_msg_out, uint8_t* d_flags_out, uint32_t* d_total) {
    GD_TRY(check_merge_args(h, old_list, n_ctx, d_wait_perm, d_wait_offsets, n, d_target_activation,
                            d_sending_activation, cap, d_offsets_out, d_msg_out, d_flags_out, d_total));
    HIP_TRY(h, hipSetDevice(h->device));
    const bool old = old_list && old_list->offsets;
    const bool chain = allow_call_chain_reentrancy && d_target_activation;
    const MergeArgs a{old ? old_list->offsets : nullptr,
                      old ? old_list->msg : nullptr,
                      old ? old_list->flags : nullptr,
                      old ? d_n_dequeued : nullptr,
                      d_wait_perm,
                      d_wait_offsets,
                      d_msg_id,
                      d_msg_flags,
                      chain ? d_target_activation : nullptr,
                      chain ? d_sending_activation : nullptr,
                      n,
                      n_ctx,
                      id_base,
                      cap};
    return merge_device(h, a, d_offsets_out, d_msg_out, d_flags_out, d_total);
}

int gd_wait_list_merge(gd_handle* h, const gd_wait_list* old_list, const uint32_t* n_dequeued, uint32_t n_ctx,
                       const uint32_t* wait_perm, const uint32_t* wait_offsets, uint32_t n, const uint32_t* msg_id,
                       uint32_t id_base, const uint8_t* msg_flags, const gd_key* target_activation,
                       const gd_key* sending_activation, int allow_call_chain_reentrancy, uint32_t cap,
                       uint32_t* out_offsets, uint32_t* out_msg, uint8_t* out_flags, uint32_t* out_total) {
    GD_TRY(check_merge_args(h, old_list, n_ctx, wait_perm, wait_offsets, n, target_activation, sending_activation, cap,
                            out_offsets, out_msg, out_flags, out_total));
    HIP_TRY(h, hipSetDevice(h->device));
    const bool old = old_list && old_list->offsets;
    const uint32_t old_total = old ? old_list->offsets[n_ctx] : 0u;
    // the new list holds at most the old entries and the batch: a device capacity past that changes nothing
    const uint32_t dcap = (uint32_t)std::min<uint64_t>(cap, (uint64_t)old_total + n);
    const bool chain = allow_call_chain_reentrancy && target_activation;
    HostStage io(h);
    MergeArgs a{};
    a.old_off = io.in(old ? old_list->offsets : nullptr, (size_t)n_ctx + 1);
    a.old_msg = io.in(old ? old_list->msg : nullptr, old_total);
    a.old_flags = io.in(old ? old_list->flags : nullptr, old_total);
    a.n_deq = io.in(old ? n_dequeued : nullptr, n_ctx);
    a.wperm = io.in(wait_perm, n);
    a.woff = io.in(wait_offsets, (size_t)n_ctx + 2);
    a.msg_id = io.in(msg_id, n);
    a.msg_flags = io.in(msg_flags, n);
    a.ta = io.in(chain ? target_activation : nullptr, n);
    a.sa = io.in(chain ? sending_activation : nullptr, n);
    a.n = n;
    a.n_ctx = n_ctx;
    a.id_base = id_base;
    a.cap = dcap;
    uint32_t* doff = io.out(out_offsets, (size_t)n_ctx + 1);
    uint32_t* dmsg = io.hold<uint32_t>(dcap, 4);       // the first min(total, dcap) come down, once the total is known
    uint8_t* dflags = io.hold<uint8_t>(dcap, 16);
    uint32_t* dtotal = io.out(out_total, 1);
    GD_TRY(io.status());
    GD_TRY(merge_device(h, a, doff, dmsg, dflags, dtotal));
    GD_TRY(io.fetch());
    GD_TRY(sync_checked(h));
    const uint32_t keep = std::min(*out_total, dcap);
    GD_TRY(io.fetch(out_msg, dmsg, keep));
    GD_TRY(io.fetch(out_flags, dflags, keep));
    return sync_checked(h);
}

}  // extern "C"
