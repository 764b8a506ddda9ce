// eng_reject.hip -- libgraindispatch: the forward rejections: the failure arm of
// Dispatcher.TryForwardRequest -> RejectMessage -> MessageFactory.CreateRejectionResponse + Message.Serialize for
// the frames of a received batch that may not forward, from the forward writer's own batch, written in batch order
// or in a given order (gd_send_queues' perm over gd_silo_index's output) as one contiguous byte run (gd_reject.h).
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_reject.h"

namespace {

int check_reject_state(gd_handle* h, const char* call) {
    if (!h) return set_err(nullptr, GD_ESTATE, "%s: null handle (no gd_encode_configure)", call);
    if (!h->enc_nsilos) return set_err(h, GD_ESTATE, "%s before gd_encode_configure", call);
    if (!h->rsp_configured) return set_err(h, GD_ESTATE, "%s before gd_respond_configure", call);
    return GD_OK;
}

int check_reject_args(gd_handle* h, const gd_forward_batch* b, uint32_t n, const void* out, uint64_t out_cap,
                      const void* out_off, const void* rej_status) {
    if (!b || !out_off) return set_err(h, GD_EINVAL, "null argument");
    if (n && (!b->buf || !b->frame_off || !b->kind || !rej_status || (!out && out_cap)))
        return set_err(h, GD_EINVAL, "null argument");
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "forward reject frames: n > 2^31");
    return GD_OK;
}

// The most bytes the call can write.  Frames are disjoint ranges of buf, so the copied bytes are at most buf_len;
// a frame gains at most the invalidation count (4), one entry (24 + TargetGrain + 28 = 80 + its KeyExt bytes),
// Direction (1), the RejectionInfo length (4), Result (1) and the info string.  The TargetGrain KeyExt bytes of all
// frames lie in buf: buf_len bounds their sum.  Totals are 32-bit (gd_reject.h).
int reject_bound(gd_handle* h, uint64_t buf_len, uint64_t body_bytes, uint32_t n, uint64_t* bound) {
    *bound = 2 * buf_len + body_bytes + (uint64_t)n * (4ull + 80 + 1 + 4 + 1 + h->rsp_maxinfo);
    if (buf_len >= (1ull << 31) || body_bytes >= (1ull << 32) || *bound >= (1ull << 32))
        return set_err(h, GD_EINVAL,
                       "forward reject frames: 2 * buf_len + body bytes + n * (90 + longest info string) reaches 2^32");
    return GD_OK;
}

// The stage on device arrays; enqueue only.  write_bound: the most bytes k_rej_write can have to write.
int reject_device(gd_handle* h, const gd_forward_batch* b, const uint8_t* buf, const uint64_t* frame_off,
                  const uint8_t* kind, const uint32_t* old_act, uint32_t n, const uint32_t* info, const uint8_t* body,
                  const uint64_t* body_off, const uint32_t* order, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                  uint8_t* rej_status, uint64_t write_bound) {
    if (n == 0) {
        HIP_TRY(h, hipMemsetAsync(out_off, 0, sizeof(uint64_t), h->stream));
        return GD_OK;
    }
    StageTime stage(h, "stage:forward_reject");
    // + 16: k_rej_write reads whole dwords around the record bytes it copies
    GD_TRY(frameout_scratch(h, h->rej_scr, n, REJ_PLAN_DW * 4, 16));
    uint32_t* plan = (uint32_t*)h->rej_scr[0].p;
    uint32_t* lens = (uint32_t*)h->rej_scr[1].p;
    uint32_t* offs = (uint32_t*)h->rej_scr[2].p;
    if (!body || !body_off) body = nullptr, body_off = nullptr;
    const RejIn in{kind, old_act, info, body_off, (const uint32_t*)h->rsp_tab[1].p, h->rsp_ninfo,
                   b->max_forward_count, b->local_silo};
    GD_TRY(launch(h, "k_rej_plan", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_rej_plan, buf, b->buf_len, frame_off,
                  n, in, enc_tab(h), plan, lens, rej_status));
    GD_TRY(frameout_offsets(h, lens, order, n, offs, out_cap, out_off, "forward_reject"));
    const RejArgs a{buf, frame_off, body, body_off, order, plan, offs, (const uint8_t*)h->rsp_tab[0].p, n, out_cap};
    return launch(h, "k_rej_write", dim3(blocks_for(write_bound + 16, ENC_TILE_CHUNKS * 16)), dim3(BLOCK), 0,
                  k_run_write<RejArgs>, a, out);
}

}  // namespace

extern "C" {

int gd_forward_reject_frames_device(gd_handle* h, const gd_forward_batch* batch, uint32_t n, const uint32_t* d_info,
                                    const uint8_t* d_body, const uint64_t* d_body_off, const uint32_t* d_order,
                                    uint8_t* d_out_buf, uint64_t out_cap, uint64_t* d_out_off, uint8_t* d_rej_status) {
    GD_TRY(check_reject_state(h, "gd_forward_reject_frames_device"));
    GD_TRY(check_reject_args(h, batch, n, d_out_buf, out_cap, d_out_off, d_rej_status));
    // the body bytes are on the device: the header part of the bound is checked here, and with bodies the
    // writer covers what out_cap allows (nothing is written past it) up to the 32-bit totals
    uint64_t bound = 0;
    GD_TRY(reject_bound(h, batch->buf_len, 0, n, &bound));
    if (d_body && d_body_off) bound = std::max(bound, std::min<uint64_t>(out_cap, 0xFFFFFFFFull));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_forward_reject_frames_device"));
    return reject_device(h, batch, batch->buf, batch->frame_off, batch->kind, batch->old_act, n, d_info, d_body,
                         d_body_off, d_order, d_out_buf, out_cap, d_out_off, d_rej_status, bound);
}

int gd_forward_reject_frames(gd_handle* h, const gd_forward_batch* batch, uint32_t n, const uint32_t* info,
                             const uint8_t* body, const uint64_t* body_off, const uint32_t* order, uint8_t* out_buf,
                             uint64_t out_cap, uint64_t* out_off, uint8_t* rej_status, uint64_t* out_total) {
    GD_TRY(check_reject_state(h, "gd_forward_reject_frames"));
    GD_TRY(check_reject_args(h, batch, n, out_buf, out_cap, out_off, rej_status));
    if (!body || !body_off) body = nullptr, body_off = nullptr;
    uint64_t body_bytes = 0;
    if (body_off && n) {
        for (uint32_t i = 0; i < n; ++i)
            if (body_off[i + 1] < body_off[i])
                return set_err(h, GD_EINVAL, "forward reject frames: body_off decreases at %u", i);
        body_bytes = body_off[n];
    }
    uint64_t bound = 0;
    GD_TRY(reject_bound(h, batch->buf_len, body_bytes, n, &bound));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_forward_reject_frames"));
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
    const uint32_t* dinfo = io.in(info, n);
    const uint8_t* dbody = io.in(body_bytes ? body : nullptr, (size_t)body_bytes);   // no bytes: as no bodies
    const uint64_t* dboff = io.in(body_off, (size_t)n + 1);
    const uint32_t* dorder = io.in(order, n);
    uint8_t* dout = io.hold<uint8_t>((size_t)cap, 16);           // out_off[n] bytes come down, once that is known
    uint64_t* dooff = io.out(out_off, (size_t)n + 1);
    uint8_t* dst = io.out(rej_status, n, 8);
    GD_TRY(io.status());
    GD_TRY(reject_device(h, batch, dbuf, dfoff, dkind, dold, n, dinfo, dbody, dboff, dorder, dout, cap, dooff, dst,
                         bound));
    return frameout_fetch(h, io, out_off, n, out_buf, dout, cap, out_total);
}

}  // extern "C"
