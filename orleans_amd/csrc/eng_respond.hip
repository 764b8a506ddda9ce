// eng_respond.hip -- libgraindispatch: the response writer: MessageFactory.CreateResponseMessage /
// CreateRejectionResponse + Message.Serialize for the request frames of a received batch, written in batch order
// or in a given order (gd_send_queues' perm over gd_silo_index's output) as one contiguous byte run (gd_respond.h).
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_respond.h"

namespace {

int check_respond_state(gd_handle* h, const char* call) {
    if (!h) return set_err(nullptr, GD_ESTATE, "%s: null handle (no gd_respond_configure)", call);
    if (!h->rsp_configured) return set_err(h, GD_ESTATE, "%s before gd_respond_configure", call);
    return GD_OK;
}

// The most header bytes the call can write: frames are disjoint ranges of buf, and an answer's header is the
// request's fields it keeps plus Direction, Result, RejectionType (a byte each) and RejectionInfo (4 + the
// string): at most 16 + the longest info string more than the request frame.  Totals are 32-bit (gd_respond.h).
int respond_bound(gd_handle* h, uint64_t buf_len, uint64_t body_bytes, uint32_t n, uint64_t* bound) {
    *bound = buf_len + body_bytes + (uint64_t)n * (16ull + h->rsp_maxinfo);
    if (buf_len >= (1ull << 32) || body_bytes >= (1ull << 32) || *bound >= (1ull << 32))
        return set_err(h, GD_EINVAL,
                       "respond frames: buf_len + body bytes + n * (16 + longest info string) reaches 2^32");
    return GD_OK;
}

// The stage on device arrays; enqueue only.  write_bound: the most bytes k_rsp_write can have to write.
int respond_device(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                   const uint8_t* kind, const uint8_t* result, const uint8_t* rejection_type, const uint32_t* info,
                   const uint8_t* body, const uint64_t* body_off, const uint32_t* order, uint8_t* out,
                   uint64_t out_cap, uint64_t* out_off, uint8_t* rsp_status, uint64_t write_bound) {
    if (n == 0) {
        HIP_TRY(h, hipMemsetAsync(out_off, 0, sizeof(uint64_t), h->stream));
        return GD_OK;
    }
    StageTime stage(h, "stage:respond");
    GD_TRY(frameout_scratch(h, h->rsp_scr, n, sizeof(RspPlan)));
    RspPlan* plan = (RspPlan*)h->rsp_scr[0].p;
    uint32_t* lens = (uint32_t*)h->rsp_scr[1].p;
    uint32_t* offs = (uint32_t*)h->rsp_scr[2].p;
    if (!body || !body_off) body = nullptr, body_off = nullptr;
    const RspIn in{kind, result, rejection_type, info, body_off, (const uint32_t*)h->rsp_tab[1].p, h->rsp_ninfo};
    if (h->walk_cih)                    // GD_OPT_WALK_INVALIDATION
        GD_TRY(launch(h, "k_rsp_plan_cih", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_rsp_plan<true>, buf, buf_len,
                      frame_off, n, in, plan, lens, rsp_status));
    else
        GD_TRY(launch(h, "k_rsp_plan", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_rsp_plan<false>, buf, buf_len,
                      frame_off, n, in, plan, lens, rsp_status));
    GD_TRY(frameout_offsets(h, lens, order, n, offs, out_cap, out_off, "respond"));
    const RspArgs a{buf, frame_off, body, body_off, order, plan, offs, (const uint8_t*)h->rsp_tab[0].p, n, out_cap};
    return launch(h, "k_rsp_write", dim3(blocks_for(write_bound + 16, ENC_TILE_CHUNKS * 16)), dim3(BLOCK), 0,
                  k_run_write<RspArgs>, a, out);
}

int check_respond_args(gd_handle* h, const void* buf, const void* off, uint32_t n, const void* kind, const void* out,
                       uint64_t out_cap, const void* out_off, const void* rsp_status) {
    if (!out_off) return set_err(h, GD_EINVAL, "null argument");
    if (n && (!buf || !off || !kind || !rsp_status || (!out && out_cap))) return set_err(h, GD_EINVAL, "null argument");
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "respond frames: n > 2^31");
    return GD_OK;
}

int kinds_device(gd_handle* h, const uint8_t* turn, const uint8_t* recv, uint32_t n, uint8_t* kind, uint8_t* rej) {
    if (n == 0) return GD_OK;
    return launch(h, "k_rsp_kinds", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_rsp_kinds, turn, recv, n, kind, rej);
}

int silo_index_device(gd_handle* h, const uint8_t* wire24, uint32_t n, uint32_t* silo) {
    if (n == 0) return GD_OK;
    return launch(h, "k_silo_index", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_silo_index,
                  (const uint32_t*)wire24, n, (const uint32_t*)h->enc_tab[0].p, h->enc_nsilos, silo);
}

int check_silo_index(gd_handle* h, const void* wire24, uint32_t n, const void* silo, bool device, const char* call) {
    if (!h) return set_err(nullptr, GD_ESTATE, "%s: null handle (no gd_encode_configure)", call);
    if (!h->enc_nsilos) return set_err(h, GD_ESTATE, "%s before gd_encode_configure", call);
    if (n && (!wire24 || !silo)) return set_err(h, GD_EINVAL, "null argument");
    if (device && (reinterpret_cast<uintptr_t>(wire24) & 3u)) return set_err(h, GD_EINVAL, "%s: addresses not 4-byte aligned", call);
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_respond_configure(gd_handle* h, const uint8_t* info_utf8, const uint32_t* info_off, uint32_t n_info) {
    if (!h) return set_err(h, GD_EINVAL, "gd_respond_configure: null handle");
    if (n_info && (!info_off || (info_off[n_info] && !info_utf8)))
        return set_err(h, GD_EINVAL, "gd_respond_configure: null info table");
    if (n_info == 0xFFFFFFFFu) return set_err(h, GD_EINVAL, "gd_respond_configure: n_info too large");
    uint32_t longest = 0;
    for (uint32_t k = 0; k < n_info; ++k) {
        if (info_off[k + 1] < info_off[k])
            return set_err(h, GD_EINVAL, "gd_respond_configure: info_off decreases at %u", k);
        longest = std::max(longest, info_off[k + 1] - info_off[k]);
    }
    if (n_info && info_off[0] != 0) return set_err(h, GD_EINVAL, "gd_respond_configure: info_off[0] is not 0");
    if (longest >= (1u << 31))
        return set_err(h, GD_EINVAL, "gd_respond_configure: an info string of %u bytes (an int32 length)", longest);
    HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t zero_off[1] = {0};
    GD_TRY(sync(h));                               // a batch in flight reads the table it was enqueued with
    h->rsp_configured = false;
    // + 4: k_rsp_write reads whole dwords around the bytes it copies
    GD_TRY(ensure(h, h->rsp_tab[0], (n_info ? (size_t)info_off[n_info] : 0) + 4));
    if (n_info && info_off[n_info])
        HIP_TRY(h, hipMemcpyAsync(h->rsp_tab[0].p, info_utf8, info_off[n_info], hipMemcpyHostToDevice, h->stream));
    GD_TRY(h2d(h, h->rsp_tab[1], n_info ? info_off : zero_off, (size_t)n_info + 1));
    GD_TRY(sync(h));
    h->rsp_ninfo = n_info;
    h->rsp_maxinfo = longest;
    h->rsp_configured = true;
    return GD_OK;
}

int gd_respond_kinds_device(gd_handle* h, const uint8_t* d_turn, const uint8_t* d_recv_status, uint32_t n,
                            uint8_t* d_kind, uint8_t* d_rejection_type) {
    if (!h) return set_err(h, GD_EINVAL, "gd_respond_kinds_device: null handle");
    if (n && (!d_turn || !d_kind || !d_rejection_type)) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return kinds_device(h, d_turn, d_recv_status, n, d_kind, d_rejection_type);
}

int gd_respond_kinds(gd_handle* h, const uint8_t* turn, const uint8_t* recv_status, uint32_t n, uint8_t* kind,
                     uint8_t* rejection_type) {
    if (!h) return set_err(h, GD_EINVAL, "gd_respond_kinds: null handle");
    if (n && (!turn || !kind || !rejection_type)) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_respond_kinds"));
    if (n == 0) return GD_OK;
    HostStage io(h);
    const uint8_t* dturn = io.in(turn, n);
    const uint8_t* drecv = io.in(recv_status, n);
    uint8_t* dkind = io.out(kind, n);
    uint8_t* drej = io.out(rejection_type, n);
    GD_TRY(io.status());
    GD_TRY(kinds_device(h, dturn, drecv, n, dkind, drej));
    GD_TRY(io.fetch());
    return sync(h);
}

int gd_silo_index_device(gd_handle* h, const uint8_t* d_wire24, uint32_t n, uint32_t* d_silo) {
    GD_TRY(check_silo_index(h, d_wire24, n, d_silo, true, "gd_silo_index_device"));
    HIP_TRY(h, hipSetDevice(h->device));
    return silo_index_device(h, d_wire24, n, d_silo);
}

int gd_silo_index(gd_handle* h, const uint8_t* wire24, uint32_t n, uint32_t* silo) {
    GD_TRY(check_silo_index(h, wire24, n, silo, false, "gd_silo_index"));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_silo_index"));
    if (n == 0) return GD_OK;
    HostStage io(h);
    const uint8_t* dwire = io.in(wire24, (size_t)n * 24);
    uint32_t* dsilo = io.out(silo, n);
    GD_TRY(io.status());
    GD_TRY(silo_index_device(h, dwire, n, dsilo));
    GD_TRY(io.fetch());
    return sync(h);
}

int gd_respond_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                             uint32_t n, const uint8_t* d_kind, const uint8_t* d_result,
                             const uint8_t* d_rejection_type, const uint32_t* d_info, const uint8_t* d_body,
                             const uint64_t* d_body_off, const uint32_t* d_order, uint8_t* d_out_buf, uint64_t out_cap,
                             uint64_t* d_out_off, uint8_t* d_rsp_status) {
    GD_TRY(check_respond_state(h, "gd_respond_frames_device"));
    GD_TRY(check_respond_args(h, d_buf, d_frame_off, n, d_kind, d_out_buf, out_cap, d_out_off, d_rsp_status));
    // the body bytes are on the device: the header part of the bound is checked here, and with bodies the
    // writer covers what out_cap allows (nothing is written past it) up to the 32-bit totals
    uint64_t bound = 0;
    GD_TRY(respond_bound(h, buf_len, 0, n, &bound));
    if (d_body && d_body_off) bound = std::max(bound, std::min<uint64_t>(out_cap, 0xFFFFFFFFull));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_respond_frames_device"));
    return respond_device(h, d_buf, buf_len, d_frame_off, n, d_kind, d_result, d_rejection_type, d_info, d_body,
                          d_body_off, d_order, d_out_buf, out_cap, d_out_off, d_rsp_status, bound);
}

int gd_respond_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                      const uint8_t* kind, const uint8_t* result, const uint8_t* rejection_type, const uint32_t* info,
                      const uint8_t* body, const uint64_t* body_off, const uint32_t* order, uint8_t* out_buf,
                      uint64_t out_cap, uint64_t* out_off, uint8_t* rsp_status, uint64_t* out_total) {
    GD_TRY(check_respond_state(h, "gd_respond_frames"));
    GD_TRY(check_respond_args(h, buf, frame_off, n, kind, out_buf, out_cap, out_off, rsp_status));
    if (!body || !body_off) body = nullptr, body_off = nullptr;
    uint64_t body_bytes = 0;
    if (body_off && n) {
        for (uint32_t i = 0; i < n; ++i)
            if (body_off[i + 1] < body_off[i]) return set_err(h, GD_EINVAL, "respond frames: body_off decreases at %u", i);
        body_bytes = body_off[n];
    }
    uint64_t bound = 0;
    GD_TRY(respond_bound(h, buf_len, body_bytes, n, &bound));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_respond_frames"));
    if (out_total) *out_total = 0;
    if (n == 0) {
        out_off[0] = 0;
        return GD_OK;
    }
    const uint64_t cap = std::min(out_cap, bound);                 // the total never exceeds the bound
    HostStage io(h);
    const uint8_t* dbuf = io.in(buf, (size_t)buf_len);
    const uint64_t* dfoff = io.in(frame_off, n);
    const uint8_t* dkind = io.in(kind, n);
    const uint8_t* dres = io.in(result, n);
    const uint8_t* drej = io.in(rejection_type, n);
    const uint32_t* dinfo = io.in(info, n);
    const uint8_t* dbody = io.in(body_bytes ? body : nullptr, (size_t)body_bytes);   // no bytes: as no bodies
    const uint64_t* dboff = io.in(body_off, (size_t)n + 1);
    const uint32_t* dorder = io.in(order, n);
    uint8_t* dout = io.hold<uint8_t>((size_t)cap, 16);           // out_off[n] bytes come down, once that is known
    uint64_t* dooff = io.out(out_off, (size_t)n + 1);
    uint8_t* dst = io.out(rsp_status, n, 8);
    GD_TRY(io.status());
    GD_TRY(respond_device(h, dbuf, buf_len, dfoff, n, dkind, dres, drej, dinfo, dbody, dboff, dorder, dout, cap, dooff,
                          dst, bound));
    return frameout_fetch(h, io, out_off, n, out_buf, dout, cap, out_total);
}

}  // extern "C"
