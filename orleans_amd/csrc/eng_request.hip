// eng_request.hip -- libgraindispatch: the request writer: MessageFactory.CreateMessage +
// InsideRuntimeClient.SendRequestMessage + Message.SetTargetPlacement + Message.Serialize for a batch of grain
// calls, written in batch order or in a given order (gd_send_queues' perm) as one contiguous byte run
// (gd_request.h); and the head of the send path as one chain: route, sender queues, writer.
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_request.h"

namespace {

int check_request_state(gd_handle* h, const char* call) {
    if (!h) return set_err(nullptr, GD_ESTATE, "%s: null handle (no gd_request_configure)", call);
    if (!h->enc_nsilos) return set_err(h, GD_ESTATE, "%s before gd_encode_configure", call);
    if (!h->req_configured) return set_err(h, GD_ESTATE, "%s before gd_request_configure", call);
    if (h->cfg.my_silo >= h->enc_nsilos)
        return set_err(h, GD_ESTATE, "%s: my_silo %u is not in gd_encode_configure's table", call, h->cfg.my_silo);
    return GD_OK;
}

int check_request_args(gd_handle* h, const gd_request_batch* b, uint32_t n, const void* silo, const void* act,
                       const void* status, const void* out, uint64_t out_cap, const void* out_off,
                       const void* req_status) {
    if (!b || !out_off) return set_err(h, GD_EINVAL, "null argument");
    if (n && (!b->target || !b->sender_grain || !b->sender_act || !req_status || (!out && out_cap)))
        return set_err(h, GD_EINVAL, "null argument");
    if ((silo != nullptr) != (act != nullptr) || (silo != nullptr) != (status != nullptr))
        return set_err(h, GD_EINVAL, "request frames: silo, act and status go together");
    for (const gd_key_ext* x : {b->target_ext, b->sender_ext})
        if (n && x && (!x->length || !x->offset || (x->bytes_len && !x->bytes)))
            return set_err(h, GD_EINVAL, "request frames: a KeyExt batch without its arrays");
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "request frames: n > 2^31");
    return GD_OK;
}

// The most bytes the call can write besides `extra` (the KeyExt and body bytes, where the host sees them): per
// message REQ_FIXED plus the three strings.  Totals are 32-bit (gd_request.h).
int request_bound(gd_handle* h, uint32_t n, uint64_t extra, uint64_t* bound) {
    *bound = (uint64_t)n * ((uint64_t)REQ_FIXED + 2ull * h->req_maxstr + h->enc_maxtype);
    if (extra >= (1ull << 32) || *bound + extra >= (1ull << 32))
        return set_err(h, GD_EINVAL,
                       "request frames: n * (206 + 2 * longest request string + longest type string) + KeyExt bytes "
                       "+ body bytes reaches 2^32");
    *bound += extra;
    return GD_OK;
}

ReqTab req_tab(gd_handle* h) {
    return ReqTab{enc_tab(h), (const uint8_t*)h->req_tab[0].p, (const uint32_t*)h->req_tab[1].p, h->req_nstr,
                  h->cfg.my_silo};
}

// The batch as the kernels take it, from pointers that are all device pointers (tx / sx: null or the KeyExt arrays).
ReqIn req_in(const gd_request_batch* b, const gd_key_ext* tx, const gd_key_ext* sx, const uint8_t* body,
             const uint64_t* body_off, const uint32_t* silo, const uint32_t* act, const uint8_t* status,
             const uint8_t* placed, const uint32_t* new_type) {
    ReqIn in{};
    in.target = (const uint64_t*)b->target;
    if (tx) in.text = tx->bytes, in.text_off = tx->offset, in.text_len = tx->length, in.text_bytes = tx->bytes_len;
    in.sender = (const uint64_t*)b->sender_grain;
    if (sx) in.sext = sx->bytes, in.sext_off = sx->offset, in.sext_len = sx->length, in.sext_bytes = sx->bytes_len;
    in.sender_act = b->sender_act;
    in.options = b->options;
    in.generic = b->generic;
    in.debug = b->debug;
    if (body && body_off) in.body = body, in.body_off = body_off;
    in.silo = silo, in.act = act, in.status = status;
    in.placed = placed, in.new_type = new_type;
    in.id_base = b->id_base, in.ttl = b->ttl_ticks;
    return in;
}

// The stage on device arrays; enqueue only.  write_bound: the most bytes k_req_write can have to write.
int request_device(gd_handle* h, const ReqIn& in, uint32_t n, const uint32_t* order, uint8_t* out, uint64_t out_cap,
                   uint64_t* out_off, uint8_t* req_status, uint64_t write_bound) {
    if (n == 0) {
        HIP_TRY(h, hipMemsetAsync(out_off, 0, sizeof(uint64_t), h->stream));
        return GD_OK;
    }
    StageTime stage(h, "stage:request");
    GD_TRY(frameout_scratch(h, h->req_scr, n, sizeof(ReqPlan)));
    ReqPlan* plan = (ReqPlan*)h->req_scr[0].p;
    uint32_t* lens = (uint32_t*)h->req_scr[1].p;
    uint32_t* offs = (uint32_t*)h->req_scr[2].p;
    const ReqTab t = req_tab(h);
    GD_TRY(launch(h, "k_req_plan", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_req_plan, in, t, n, plan, lens,
                  req_status));
    GD_TRY(frameout_offsets(h, lens, order, n, offs, out_cap, out_off, "request"));
    const ReqArgs a{in, order, plan, offs, n, out_cap};
    return launch(h, "k_req_write", dim3(blocks_for(write_bound + 16, REQ_TILE)), dim3(BLOCK), 0, k_req_write, a, t,
                  out);
}

// The send stage for the batch: per message the TimeToLive its frame carries.
int request_send_queues(gd_handle* h, const gd_request_batch* b, const uint8_t* d_options, uint32_t n,
                        const uint32_t* d_silo, const uint8_t* d_status, uint8_t* d_send_status, uint32_t* d_queue,
                        uint32_t* d_perm, uint32_t* d_offsets) {
    const int64_t* ttl = nullptr;
    if (n && b->ttl_ticks != GD_TTL_NONE) {
        GD_TRY(ensure(h, h->req_scr[3], (size_t)n * 8));
        GD_TRY(launch(h, "k_req_ttl", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_req_ttl, d_options,
                      (long long)b->ttl_ticks, n, (long long*)h->req_scr[3].p));
        ttl = (const int64_t*)h->req_scr[3].p;
    }
    return gd_send_queues_device(h, d_silo, d_status, nullptr, ttl, n, d_send_status, d_queue, d_perm, d_offsets);
}

// A KeyExt batch of a host-pointer call on the device: its three arrays take three staging slots.
const gd_key_ext* stage_ext(HostStage& io, const gd_key_ext* x, uint32_t n, gd_key_ext* dev) {
    const bool want = x != nullptr && n != 0;
    dev->bytes = io.in(want && x->bytes_len ? x->bytes : nullptr, want ? (size_t)x->bytes_len : 0);
    dev->offset = io.in(want ? x->offset : nullptr, n);
    dev->length = io.in(want ? x->length : nullptr, n);
    dev->bytes_len = want ? x->bytes_len : 0;
    return want ? dev : nullptr;
}

// What a host-pointer call stages of the batch itself, and the bound its lengths give.
struct HostBatch {
    gd_request_batch d{};        // the batch with device pointers
    gd_key_ext tx{}, sx{};
    const gd_key_ext *ptx = nullptr, *psx = nullptr;
    const uint8_t* body = nullptr;
    const uint64_t* body_off = nullptr;
};

int host_extra_bytes(gd_handle* h, const gd_request_batch* b, uint32_t n, uint64_t* extra, uint64_t* body_bytes) {
    *extra = 0, *body_bytes = 0;
    if (!n) return GD_OK;
    for (const gd_key_ext* x : {b->target_ext, b->sender_ext})
        if (x)
            for (uint32_t i = 0; i < n; ++i)
                if (x->length[i] > 0) *extra += (uint64_t)x->length[i];
    if (b->body && b->body_off) {
        for (uint32_t i = 0; i < n; ++i)
            if (b->body_off[i + 1] < b->body_off[i])
                return set_err(h, GD_EINVAL, "request frames: body_off decreases at %u", i);
        *body_bytes = b->body_off[n] - b->body_off[0];
        *extra += *body_bytes;
    }
    return GD_OK;
}

void stage_batch(HostStage& io, const gd_request_batch* b, uint32_t n, uint64_t body_bytes, HostBatch* s) {
    s->d = *b;
    s->d.target = io.in(b->target, n);
    s->ptx = stage_ext(io, b->target_ext, n, &s->tx);
    s->d.sender_grain = io.in(b->sender_grain, n);
    s->psx = stage_ext(io, b->sender_ext, n, &s->sx);
    s->d.sender_act = io.in(b->sender_act, n);
    s->d.options = io.in(b->options, n);
    s->d.generic = io.in(b->generic, n);
    s->d.debug = io.in(b->debug, n);
    const bool bodies = b->body && b->body_off && body_bytes;
    // the bodies as they lie in the caller's buffer, body_off[0] bytes in: the offsets stay as given
    s->body = io.in(bodies ? b->body : nullptr, bodies ? (size_t)b->body_off[n] : 0);
    s->body_off = io.in(bodies ? b->body_off : nullptr, (size_t)n + 1);
}

}  // namespace

extern "C" {

int gd_request_configure(gd_handle* h, const uint8_t* str_utf8, const uint32_t* str_off, uint32_t n_str) {
    if (!h) return set_err(h, GD_EINVAL, "gd_request_configure: null handle");
    if (n_str && (!str_off || (str_off[n_str] && !str_utf8)))
        return set_err(h, GD_EINVAL, "gd_request_configure: null string table");
    if (n_str == 0xFFFFFFFFu) return set_err(h, GD_EINVAL, "gd_request_configure: n_str too large");
    uint32_t longest = 0;
    for (uint32_t k = 0; k < n_str; ++k) {
        if (str_off[k + 1] < str_off[k])
            return set_err(h, GD_EINVAL, "gd_request_configure: str_off decreases at %u", k);
        longest = std::max(longest, str_off[k + 1] - str_off[k]);
    }
    if (n_str && str_off[0] != 0) return set_err(h, GD_EINVAL, "gd_request_configure: str_off[0] is not 0");
    if (longest > REQ_MAX_STR)
        return set_err(h, GD_EINVAL, "gd_request_configure: a string of %u bytes (at most %u)", longest, REQ_MAX_STR);
    HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t zero_off[1] = {0};
    GD_TRY(sync(h));                               // a batch in flight reads the table it was enqueued with
    h->req_configured = false;
    GD_TRY(h2d(h, h->req_tab[0], str_utf8, n_str ? (size_t)str_off[n_str] : 0));
    GD_TRY(h2d(h, h->req_tab[1], n_str ? str_off : zero_off, (size_t)n_str + 1));
    GD_TRY(sync(h));
    h->req_nstr = n_str;
    h->req_maxstr = longest;
    h->req_configured = true;
    return GD_OK;
}

int gd_request_frames_device(gd_handle* h, const gd_request_batch* batch, uint32_t n, const uint32_t* d_silo,
                             const uint32_t* d_act, const uint8_t* d_status, const uint8_t* d_placed,
                             const uint32_t* d_new_type, const uint32_t* d_order, uint8_t* d_out_buf, uint64_t out_cap,
                             uint64_t* d_out_off, uint8_t* d_req_status) {
    GD_TRY(check_request_state(h, "gd_request_frames_device"));
    GD_TRY(check_request_args(h, batch, n, d_silo, d_act, d_status, d_out_buf, out_cap, d_out_off, d_req_status));
    // the KeyExt lengths and body_off are on the device: the rest of the bound is checked here, and with either
    // the writer covers what out_cap allows (nothing is written past it) up to the 32-bit totals
    uint64_t bound = 0;
    GD_TRY(request_bound(h, n, 0, &bound));
    if (batch->target_ext || batch->sender_ext || (batch->body && batch->body_off))
        bound = std::max(bound, std::min<uint64_t>(out_cap, 0xFFFFFFFFull));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_request_frames_device"));
    const ReqIn in = req_in(batch, batch->target_ext, batch->sender_ext, batch->body, batch->body_off, d_silo, d_act,
                            d_status, d_placed, d_new_type);
    return request_device(h, in, n, d_order, d_out_buf, out_cap, d_out_off, d_req_status, bound);
}

int gd_request_send_device(gd_handle* h, const gd_request_batch* batch, uint32_t n, uint32_t* d_silo, uint32_t* d_act,
                           uint8_t* d_status, uint8_t* d_send_status, uint32_t* d_queue, uint32_t* d_perm,
                           uint32_t* d_offsets, uint8_t* d_out_buf, uint64_t out_cap, uint64_t* d_out_off,
                           uint8_t* d_req_status) {
    GD_TRY(check_request_state(h, "gd_request_send_device"));
    if (!h->send_nq) return set_err(h, GD_ESTATE, "gd_request_send_device before gd_send_configure");
    GD_TRY(check_request_args(h, batch, n, d_silo, d_act, d_status, d_out_buf, out_cap, d_out_off, d_req_status));
    if (!d_perm || !d_offsets || (n && (!d_silo || !d_send_status))) return set_err(h, GD_EINVAL, "null argument");
    uint64_t bound = 0;
    GD_TRY(request_bound(h, n, 0, &bound));
    if (batch->target_ext || batch->sender_ext || (batch->body && batch->body_off))
        bound = std::max(bound, std::min<uint64_t>(out_cap, 0xFFFFFFFFull));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_request_send_device"));
    if (n) GD_TRY(route_device(h, batch->target, n, d_silo, d_act, d_status));
    GD_TRY(request_send_queues(h, batch, batch->options, n, d_silo, d_status, d_send_status, d_queue, d_perm,
                               d_offsets));
    const ReqIn in = req_in(batch, batch->target_ext, batch->sender_ext, batch->body, batch->body_off, d_silo, d_act,
                            d_status, nullptr, nullptr);
    return request_device(h, in, n, d_perm, d_out_buf, out_cap, d_out_off, d_req_status, bound);
}

int gd_request_frames(gd_handle* h, const gd_request_batch* batch, uint32_t n, const uint32_t* silo,
                      const uint32_t* act, const uint8_t* status, const uint8_t* placed, const uint32_t* new_type,
                      const uint32_t* order, uint8_t* out_buf, uint64_t out_cap, uint64_t* out_off,
                      uint8_t* req_status, uint64_t* out_total) {
    GD_TRY(check_request_state(h, "gd_request_frames"));
    GD_TRY(check_request_args(h, batch, n, silo, act, status, out_buf, out_cap, out_off, req_status));
    uint64_t extra = 0, body_bytes = 0, bound = 0;
    GD_TRY(host_extra_bytes(h, batch, n, &extra, &body_bytes));
    GD_TRY(request_bound(h, n, extra, &bound));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_request_frames"));
    if (out_total) *out_total = 0;
    if (n == 0) {
        out_off[0] = 0;
        return GD_OK;
    }
    const uint64_t cap = std::min(out_cap, bound);                 // the total never exceeds the bound
    HostStage io(h);
    HostBatch s;
    stage_batch(io, batch, n, body_bytes, &s);
    const uint32_t* dsilo = io.in(silo, n);
    const uint32_t* dact = io.in(act, n);
    const uint8_t* dstatus = io.in(status, n);
    const uint8_t* dplaced = io.in(placed, n);
    const uint32_t* dtype = io.in(new_type, n);
    const uint32_t* dorder = io.in(order, n);
    uint8_t* dout = io.hold<uint8_t>((size_t)cap, 16);           // out_off[n] bytes come down, once that is known
    uint64_t* dooff = io.out(out_off, (size_t)n + 1);
    uint8_t* dst = io.out(req_status, n, 8);
    GD_TRY(io.status());
    const ReqIn in = req_in(&s.d, s.ptx, s.psx, s.body, s.body_off, dsilo, dact, dstatus, dplaced, dtype);
    GD_TRY(request_device(h, in, n, dorder, dout, cap, dooff, dst, bound));
    return frameout_fetch(h, io, out_off, n, out_buf, dout, cap, out_total);
}

int gd_request_send(gd_handle* h, const gd_request_batch* batch, uint32_t n, uint32_t* out_silo, uint32_t* out_act,
                    uint8_t* out_status, uint8_t* out_send_status, uint32_t* out_queue, uint32_t* out_perm,
                    uint32_t* out_offsets, uint8_t* out_buf, uint64_t out_cap, uint64_t* out_off, uint8_t* req_status,
                    uint64_t* out_total) {
    GD_TRY(check_request_state(h, "gd_request_send"));
    if (!h->send_nq) return set_err(h, GD_ESTATE, "gd_request_send before gd_send_configure");
    GD_TRY(check_request_args(h, batch, n, out_silo, out_act, out_status, out_buf, out_cap, out_off, req_status));
    if (!out_perm || !out_offsets || (n && (!out_silo || !out_send_status)))
        return set_err(h, GD_EINVAL, "null argument");
    uint64_t extra = 0, body_bytes = 0, bound = 0;
    GD_TRY(host_extra_bytes(h, batch, n, &extra, &body_bytes));
    GD_TRY(request_bound(h, n, extra, &bound));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_request_send"));
    if (out_total) *out_total = 0;
    const uint64_t cap = std::min(out_cap, bound);
    const uint32_t B = h->send_nq + 4;
    HostStage io(h);
    HostBatch s;
    stage_batch(io, batch, n, body_bytes, &s);
    uint32_t* dsilo = io.out(out_silo, n, 16);
    uint32_t* dact = io.out(out_act, n, 16);
    uint8_t* dstatus = io.out(out_status, n, 16);
    uint8_t* dsst = io.out(out_send_status, n, 4);
    uint32_t* dq = io.out_if(out_queue, n, 4);
    uint32_t* dperm = io.out(out_perm, n, 4);
    uint32_t* doffs = io.out(out_offsets, (size_t)B + 1);
    uint8_t* dout = io.hold<uint8_t>((size_t)cap, 16);
    uint64_t* dooff = io.out(out_off, (size_t)n + 1);
    uint8_t* dst = io.out(req_status, n, 8);
    GD_TRY(io.status());
    if (n) GD_TRY(route_device(h, s.d.target, n, dsilo, dact, dstatus));
    GD_TRY(request_send_queues(h, &s.d, s.d.options, n, dsilo, dstatus, dsst, dq, dperm, doffs));
    const ReqIn in = req_in(&s.d, s.ptx, s.psx, s.body, s.body_off, dsilo, dact, dstatus, nullptr, nullptr);
    GD_TRY(request_device(h, in, n, dperm, dout, cap, dooff, dst, bound));
    return frameout_fetch(h, io, out_off, n, out_buf, dout, cap, out_total);
}

}  // extern "C"
