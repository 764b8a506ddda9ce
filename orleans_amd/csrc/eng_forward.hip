// eng_forward.hip -- libgraindispatch: the forward writer: Dispatcher.TryForwardRequest ->
// TryForwardMessage -> ResendMessageImpl -> AddressMessage + Message.Serialize for the frames of a received batch
// that must be forwarded, written in batch order or in a given order (gd_send_queues' perm) as one contiguous byte
// run (gd_forward.h); and the chain: plan, route, sender queues, writer.
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_forward.h"

namespace {

int check_forward_state(gd_handle* h, const char* call) {
    if (!h) return set_err(nullptr, GD_ESTATE, "%s: null handle (no gd_encode_configure)", call);
    if (!h->enc_nsilos) return set_err(h, GD_ESTATE, "%s before gd_encode_configure", call);
    return GD_OK;
}

int check_forward_args(gd_handle* h, const gd_forward_batch* b, uint32_t n, const void* silo, const void* act,
                       const void* status, const void* out, uint64_t out_cap, const void* out_off,
                       const void* fwd_status) {
    if (!b || !out_off) return set_err(h, GD_EINVAL, "null argument");
    if (n && (!b->buf || !b->frame_off || !b->kind || !fwd_status || (!out && out_cap)))
        return set_err(h, GD_EINVAL, "null argument");
    if ((b->fwd_silo != nullptr) != (b->fwd_act != nullptr))
        return set_err(h, GD_EINVAL, "forward frames: fwd_silo and fwd_act go together");
    if ((silo != nullptr) != (act != nullptr) || (silo != nullptr) != (status != nullptr))
        return set_err(h, GD_EINVAL, "forward frames: silo, act and status go together");
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "forward frames: n > 2^31");
    return GD_OK;
}

// The most bytes the call can write.  Frames are disjoint ranges of buf, so the copied bytes are at most buf_len;
// a frame gains at most the invalidation count (4), one entry (24 + TargetGrain + 28 = 80 + its KeyExt bytes),
// ForwardCount (4) and the encoder's 57 + the longest type string.  The TargetGrain KeyExt bytes of all frames lie
// in buf: buf_len bounds their sum.  Totals are 32-bit (gd_forward.h).
int forward_bound(gd_handle* h, uint64_t buf_len, uint32_t n, uint64_t* bound) {
    *bound = 2 * buf_len + (uint64_t)n * (4ull + 80 + 4 + 57 + h->enc_maxtype);
    if (buf_len >= (1ull << 32) || *bound >= (1ull << 32))
        return set_err(h, GD_EINVAL, "forward frames: 2 * buf_len + n * (145 + longest type string) reaches 2^32");
    return GD_OK;
}

struct FwdScratch {
    FwdPlan* plan;
    uint32_t* lens;
    uint32_t* offs;
};

int forward_scratch(gd_handle* h, uint32_t n, FwdScratch* s) {
    GD_TRY(frameout_scratch(h, h->fwd_scr, n, sizeof(FwdPlan)));
    s->plan = (FwdPlan*)h->fwd_scr[0].p;
    s->lens = (uint32_t*)h->fwd_scr[1].p;
    s->offs = (uint32_t*)h->fwd_scr[2].p;
    return GD_OK;
}

FwdIn fwd_in(const gd_forward_batch* b, const uint8_t* kind, const uint32_t* old_act, const uint32_t* fwd_silo,
             const uint32_t* fwd_act, const uint32_t* silo, const uint32_t* act, const uint8_t* status,
             const uint8_t* placed, const uint32_t* new_type) {
    FwdIn in{};
    in.kind = kind, in.old_act = old_act, in.fwd_silo = fwd_silo, in.fwd_act = fwd_act;
    in.silo = silo, in.act = act, in.status = status, in.placed = placed, in.new_type = new_type;
    in.max_forward = b->max_forward_count, in.local_silo = b->local_silo;
    return in;
}

// Offsets, capacity check and the write, from finished plans; enqueue only.
int forward_write(gd_handle* h, const uint8_t* buf, const uint64_t* frame_off, uint32_t n, uint32_t local_silo,
                  const FwdScratch& s, const uint32_t* order, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                  uint64_t write_bound) {
    GD_TRY(frameout_offsets(h, s.lens, order, n, s.offs, out_cap, out_off, "forward"));
    const FwdArgs a{buf, frame_off, order, s.plan, s.offs, (const uint8_t*)h->act_ids.p,
                    (const uint8_t*)h->enc_tab[0].p, (const uint8_t*)h->enc_tab[1].p, local_silo, n, out_cap};
    return launch(h, "k_fwd_write", dim3(blocks_for(write_bound + 16, ENC_TILE_CHUNKS * 16)), dim3(BLOCK), 0,
                  k_run_write<FwdArgs>, a, out);
}

// The stage on device arrays; enqueue only.
int forward_device(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                   const FwdIn& in, const uint32_t* order, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                   uint8_t* fwd_status, gd_key* target, uint64_t write_bound) {
    if (n == 0) {
        HIP_TRY(h, hipMemsetAsync(out_off, 0, sizeof(uint64_t), h->stream));
        return GD_OK;
    }
    StageTime stage(h, "stage:forward");
    FwdScratch s;
    GD_TRY(forward_scratch(h, n, &s));
    GD_TRY(launch(h, "k_fwd_plan", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_fwd_plan, buf, buf_len, frame_off, n,
                  in, enc_tab(h), s.plan, s.lens, fwd_status, (uint64_t*)target));
    return forward_write(h, buf, frame_off, n, in.local_silo, s, order, out, out_cap, out_off, write_bound);
}

// The chain on device arrays; enqueue only: plan (no route yet), route on the TargetGrain keys, merge, finish the
// plans the route hit, sender queues (with each frame's own Category and TimeToLive), write with order = perm.
int forward_send_device(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                        FwdIn in, uint32_t* silo, uint32_t* act, uint8_t* status, uint8_t* send_status,
                        uint32_t* queue, uint32_t* perm, uint32_t* offsets, uint8_t* out, uint64_t out_cap,
                        uint64_t* out_off, uint8_t* fwd_status, gd_key* target, uint64_t write_bound) {
    if (n == 0) {
        HIP_TRY(h, hipMemsetAsync(out_off, 0, sizeof(uint64_t), h->stream));
        return gd_send_queues_device(h, silo, status, nullptr, nullptr, 0, send_status, queue, perm, offsets);
    }
    StageTime stage(h, "stage:forward_send");
    FwdScratch s;
    GD_TRY(forward_scratch(h, n, &s));
    GD_TRY(ensure(h, h->fwd_scr[3], (size_t)n * 8));
    GD_TRY(ensure(h, h->fwd_scr[4], (size_t)n));
    in.silo = nullptr, in.act = nullptr, in.status = nullptr, in.placed = nullptr, in.new_type = nullptr;
    in.ttl = (long long*)h->fwd_scr[3].p;
    in.category = (uint8_t*)h->fwd_scr[4].p;
    const EncTab t = enc_tab(h);
    GD_TRY(launch(h, "k_fwd_plan", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_fwd_plan, buf, buf_len, frame_off, n,
                  in, t, s.plan, s.lens, fwd_status, (uint64_t*)target));
    GD_TRY(route_device(h, target, n, silo, act, status));
    GD_TRY(launch(h, "k_fwd_merge", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_fwd_merge,
                  (const uint8_t*)fwd_status, (const FwdPlan*)s.plan, n, silo, act, status));
    GD_TRY(launch(h, "k_fwd_finish", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_fwd_finish, (const uint32_t*)silo,
                  (const uint32_t*)act, (const uint8_t*)status, n, t, s.plan, s.lens, fwd_status));
    GD_TRY(gd_send_queues_device(h, silo, status, in.category, (const int64_t*)in.ttl, n, send_status, queue, perm,
                                 offsets));
    return forward_write(h, buf, frame_off, n, in.local_silo, s, perm, out, out_cap, out_off, write_bound);
}

int kinds_device(gd_handle* h, const uint8_t* turn, uint32_t n, uint8_t* kind) {
    if (n == 0) return GD_OK;
    return launch(h, "k_fwd_kinds", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_fwd_kinds, turn, n, kind);
}

}  // namespace

extern "C" {

int gd_forward_kinds_device(gd_handle* h, const uint8_t* d_turn, uint32_t n, uint8_t* d_kind) {
    GD_TRY(check_forward_state(h, "gd_forward_kinds_device"));
    if (n && (!d_turn || !d_kind)) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_forward_kinds_device"));
    return kinds_device(h, d_turn, n, d_kind);
}

int gd_forward_kinds(gd_handle* h, const uint8_t* turn, uint32_t n, uint8_t* kind) {
    GD_TRY(check_forward_state(h, "gd_forward_kinds"));
    if (n && (!turn || !kind)) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_forward_kinds"));
    if (n == 0) return GD_OK;
    HostStage io(h);
    const uint8_t* dturn = io.in(turn, n);
    uint8_t* dkind = io.out(kind, n);
    GD_TRY(io.status());
    GD_TRY(kinds_device(h, dturn, n, dkind));
    GD_TRY(io.fetch());
    return sync(h);
}

int gd_forward_frames_device(gd_handle* h, const gd_forward_batch* batch, uint32_t n, const uint32_t* d_silo,
                             const uint32_t* d_act, const uint8_t* d_status, const uint8_t* d_placed,
                             const uint32_t* d_new_type, const uint32_t* d_order, uint8_t* d_out_buf, uint64_t out_cap,
                             uint64_t* d_out_off, uint8_t* d_fwd_status, gd_key* d_target) {
    GD_TRY(check_forward_state(h, "gd_forward_frames_device"));
    GD_TRY(check_forward_args(h, batch, n, d_silo, d_act, d_status, d_out_buf, out_cap, d_out_off, d_fwd_status));
    uint64_t bound = 0;
    GD_TRY(forward_bound(h, batch->buf_len, n, &bound));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_forward_frames_device"));
    const FwdIn in = fwd_in(batch, batch->kind, batch->old_act, batch->fwd_silo, batch->fwd_act, d_silo, d_act,
                            d_status, d_placed, d_new_type);
    return forward_device(h, batch->buf, batch->buf_len, batch->frame_off, n, in, d_order, d_out_buf, out_cap,
                          d_out_off, d_fwd_status, d_target, bound);
}

int gd_forward_send_device(gd_handle* h, const gd_forward_batch* batch, uint32_t n, uint32_t* d_silo, uint32_t* d_act,
                           uint8_t* d_status, uint8_t* d_send_status, uint32_t* d_queue, uint32_t* d_perm,
                           uint32_t* d_offsets, uint8_t* d_out_buf, uint64_t out_cap, uint64_t* d_out_off,
                           uint8_t* d_fwd_status, gd_key* d_target) {
    GD_TRY(check_forward_state(h, "gd_forward_send_device"));
    if (!h->send_nq) return set_err(h, GD_ESTATE, "gd_forward_send_device before gd_send_configure");
    GD_TRY(check_forward_args(h, batch, n, d_silo, d_act, d_status, d_out_buf, out_cap, d_out_off, d_fwd_status));
    if (!d_perm || !d_offsets || (n && (!d_silo || !d_send_status || !d_target)))
        return set_err(h, GD_EINVAL, "null argument");
    uint64_t bound = 0;
    GD_TRY(forward_bound(h, batch->buf_len, n, &bound));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_forward_send_device"));
    const FwdIn in = fwd_in(batch, batch->kind, batch->old_act, batch->fwd_silo, batch->fwd_act, nullptr, nullptr,
                            nullptr, nullptr, nullptr);
    return forward_send_device(h, batch->buf, batch->buf_len, batch->frame_off, n, in, d_silo, d_act, d_status,
                               d_send_status, d_queue, d_perm, d_offsets, d_out_buf, out_cap, d_out_off, d_fwd_status,
                               d_target, bound);
}

int gd_forward_frames(gd_handle* h, const gd_forward_batch* batch, uint32_t n, const uint32_t* silo,
                      const uint32_t* act, const uint8_t* status, const uint8_t* placed, const uint32_t* new_type,
                      const uint32_t* order, uint8_t* out_buf, uint64_t out_cap, uint64_t* out_off,
                      uint8_t* fwd_status, gd_key* target, uint64_t* out_total) {
    GD_TRY(check_forward_state(h, "gd_forward_frames"));
    GD_TRY(check_forward_args(h, batch, n, silo, act, status, out_buf, out_cap, out_off, fwd_status));
    uint64_t bound = 0;
    GD_TRY(forward_bound(h, batch->buf_len, n, &bound));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_forward_frames"));
    if (out_total) *out_total = 0;
    if (n == 0) {
        out_off[0] = 0;
        return GD_OK;
    }
    const uint64_t cap = std::min(out_cap, bound);                 // the total never exceeds the bound
    HostStage io(h);
    const uint8_t* dbuf = io.in(batch->buf, (size_t)batch->buf_len);
    const uint64_t* dfoff = io.in(batch->frame_off, n);
    const uint8_t* dkind = io.in(batch->kind, n);
    const uint32_t* dold = io.in(batch->old_act, n);
    const uint32_t* dfs = io.in(batch->fwd_silo, n);
    const uint32_t* dfa = io.in(batch->fwd_act, n);
    const uint32_t* dsilo = io.in(silo, n);
    const uint32_t* dact = io.in(act, n);
    const uint8_t* dstatus = io.in(status, n);
    const uint8_t* dplaced = io.in(placed, n);
    const uint32_t* dtype = io.in(new_type, n);
    const uint32_t* dorder = io.in(order, n);
    uint8_t* dout = io.hold<uint8_t>((size_t)cap, 16);           // out_off[n] bytes come down, once that is known
    uint64_t* dooff = io.out(out_off, (size_t)n + 1);
    uint8_t* dst = io.out(fwd_status, n, 8);
    gd_key* dtg = io.out_if(target, n);
    GD_TRY(io.status());
    const FwdIn in = fwd_in(batch, dkind, dold, dfs, dfa, dsilo, dact, dstatus, dplaced, dtype);
    GD_TRY(forward_device(h, dbuf, batch->buf_len, dfoff, n, in, dorder, dout, cap, dooff, dst, dtg, bound));
    return frameout_fetch(h, io, out_off, n, out_buf, dout, cap, out_total);
}

int gd_forward_send(gd_handle* h, const gd_forward_batch* batch, uint32_t n, uint32_t* out_silo, uint32_t* out_act,
                    uint8_t* out_status, uint8_t* out_send_status, uint32_t* out_queue, uint32_t* out_perm,
                    uint32_t* out_offsets, uint8_t* out_buf, uint64_t out_cap, uint64_t* out_off, uint8_t* fwd_status,
                    gd_key* target, uint64_t* out_total) {
    GD_TRY(check_forward_state(h, "gd_forward_send"));
    if (!h->send_nq) return set_err(h, GD_ESTATE, "gd_forward_send before gd_send_configure");
    GD_TRY(check_forward_args(h, batch, n, out_silo, out_act, out_status, out_buf, out_cap, out_off, fwd_status));
    if (!out_perm || !out_offsets || (n && (!out_silo || !out_send_status || !target)))
        return set_err(h, GD_EINVAL, "null argument");
    uint64_t bound = 0;
    GD_TRY(forward_bound(h, batch->buf_len, n, &bound));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_forward_send"));
    if (out_total) *out_total = 0;
    const uint64_t cap = std::min(out_cap, bound);
    const uint32_t B = h->send_nq + 4;
    HostStage io(h);
    const uint8_t* dbuf = io.in(n ? batch->buf : nullptr, (size_t)batch->buf_len);
    const uint64_t* dfoff = io.in(batch->frame_off, n);
    const uint8_t* dkind = io.in(batch->kind, n);
    const uint32_t* dold = io.in(batch->old_act, n);
    const uint32_t* dfs = io.in(batch->fwd_silo, n);
    const uint32_t* dfa = io.in(batch->fwd_act, n);
    uint32_t* dsilo = io.out(out_silo, n, 16);
    uint32_t* dact = io.out(out_act, n, 16);
    uint8_t* dstatus = io.out(out_status, n, 16);
    uint8_t* dsst = io.out(out_send_status, n, 4);
    uint32_t* dq = io.out_if(out_queue, n, 4);
    uint32_t* dperm = io.out(out_perm, n, 4);
    uint32_t* doffs = io.out(out_offsets, (size_t)B + 1);
    uint8_t* dout = io.hold<uint8_t>((size_t)cap, 16);
    uint64_t* dooff = io.out(out_off, (size_t)n + 1);
    uint8_t* dst = io.out(fwd_status, n, 8);
    gd_key* dtg = io.out(target, n, 8);
    GD_TRY(io.status());
    const FwdIn in = fwd_in(batch, dkind, dold, dfs, dfa, nullptr, nullptr, nullptr, nullptr, nullptr);
    GD_TRY(forward_send_device(h, dbuf, batch->buf_len, dfoff, n, in, dsilo, dact, dstatus, dsst, dq, dperm, doffs,
                               dout, cap, dooff, dst, dtg, bound));
    return frameout_fetch(h, io, out_off, n, out_buf, dout, cap, out_total);
}

}  // extern "C"
