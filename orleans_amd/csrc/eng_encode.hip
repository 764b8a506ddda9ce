// eng_encode.hip -- libgraindispatch: the frame encoder: Message.SetTargetPlacement + Message.Serialize
// for the frames of a routed batch, written in batch order or in a given order (gd_send_queues' perm) as one
// contiguous byte run (gd_encode.h).
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_encode.h"

namespace {

int check_encode_state(gd_handle* h, const char* call) {
    if (!h) return set_err(nullptr, GD_ESTATE, "%s: null handle (no gd_encode_configure)", call);
    if (!h->enc_nsilos) return set_err(h, GD_ESTATE, "%s before gd_encode_configure", call);
    return GD_OK;
}

// The most bytes the call can write: frames are disjoint ranges of buf, and a frame grows by at most
// 28 (TargetActivation) + 24 (TargetSilo) + 1 (IsNewPlacement) + 4 + the longest type string.  Totals are
// 32-bit (gd_encode.h): a bound of 2^32 or more is refused.
int encode_bound(gd_handle* h, uint64_t buf_len, uint32_t n, uint64_t* bound) {
    *bound = buf_len + (uint64_t)n * (57ull + h->enc_maxtype);
    if (buf_len >= (1ull << 32) || *bound >= (1ull << 32))
        return set_err(h, GD_EINVAL, "encode frames: buf_len + n * (57 + longest type string) reaches 2^32");
    return GD_OK;
}

// The stage on device arrays (placed / new_type / order may be null); enqueue only.
int encode_device(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                  const uint32_t* silo, const uint32_t* act, const uint8_t* status, const uint8_t* placed,
                  const uint32_t* new_type, const uint32_t* order, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                  uint8_t* enc_status, uint64_t bound) {
    if (n == 0) {
        HIP_TRY(h, hipMemsetAsync(out_off, 0, sizeof(uint64_t), h->stream));
        return GD_OK;
    }
    StageTime stage(h, "stage:encode");
    GD_TRY(frameout_scratch(h, h->enc_scr, n, sizeof(EncPlan)));
    EncPlan* plan = (EncPlan*)h->enc_scr[0].p;
    uint32_t* lens = (uint32_t*)h->enc_scr[1].p;
    uint32_t* offs = (uint32_t*)h->enc_scr[2].p;
    const EncTab t = enc_tab(h);
    if (h->walk_cih)                    // GD_OPT_WALK_INVALIDATION
        GD_TRY(launch(h, "k_enc_plan_cih", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_enc_plan<true>, buf, buf_len,
                      frame_off, n, silo, act, status, placed, new_type, t, plan, lens, enc_status));
    else
        GD_TRY(launch(h, "k_enc_plan", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_enc_plan<false>, buf, buf_len,
                      frame_off, n, silo, act, status, placed, new_type, t, plan, lens, enc_status));
    GD_TRY(frameout_offsets(h, lens, order, n, offs, out_cap, out_off, "encode"));
    const EncArgs a{buf, frame_off, silo, act, new_type, order, plan, offs, n, out_cap};
    return launch(h, "k_enc_write", dim3(blocks_for(bound + 16, ENC_TILE_CHUNKS * 16)), dim3(BLOCK), 0, k_enc_write, a, t,
                  out);
}

int check_encode_args(gd_handle* h, const void* buf, const void* off, uint32_t n, const void* silo, const void* act,
                      const void* status, const void* out, uint64_t out_cap, const void* out_off,
                      const void* enc_status) {
    if (!out_off) return set_err(h, GD_EINVAL, "null argument");
    if (n && (!buf || !off || !silo || !act || !status || !enc_status || (!out && out_cap)))
        return set_err(h, GD_EINVAL, "null argument");
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "encode frames: n > 2^31");
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_encode_configure(gd_handle* h, const gd_silo_addr* silos, uint32_t n_silos, const uint8_t* type_utf8,
                        const uint32_t* type_off, uint32_t n_types) {
    if (!h || !silos || n_silos < 1) return set_err(h, GD_EINVAL, "gd_encode_configure: null argument or no silo");
    if (n_types && (!type_off || (type_off[n_types] && !type_utf8)))
        return set_err(h, GD_EINVAL, "gd_encode_configure: null type table");
    if (n_types == 0xFFFFFFFFu) return set_err(h, GD_EINVAL, "gd_encode_configure: n_types too large");
    uint32_t longest = 0;
    for (uint32_t k = 0; k < n_types; ++k) {
        if (type_off[k + 1] < type_off[k]) return set_err(h, GD_EINVAL, "gd_encode_configure: type_off decreases at %u", k);
        longest = std::max(longest, type_off[k + 1] - type_off[k]);
    }
    if (n_types && type_off[0] != 0) return set_err(h, GD_EINVAL, "gd_encode_configure: type_off[0] is not 0");
    if (longest > ENC_MAX_TYPE)
        return set_err(h, GD_EINVAL, "gd_encode_configure: a type string of %u bytes (at most %u)", longest, ENC_MAX_TYPE);
    HIP_TRY(h, hipSetDevice(h->device));
    // the wire SiloAddress: 16-byte IP, int32 port, int32 generation (BinaryTokenStreamWriter.cs:485-513)
    std::vector<uint32_t> wire((size_t)n_silos * 6);
    for (uint32_t s = 0; s < n_silos; ++s) {
        std::memcpy(&wire[(size_t)s * 6], silos[s].ip, 16);
        wire[(size_t)s * 6 + 4] = (uint32_t)silos[s].port;
        wire[(size_t)s * 6 + 5] = (uint32_t)silos[s].generation;
    }
    const uint32_t zero_off[1] = {0};
    GD_TRY(sync(h));                               // a batch in flight reads the tables it was enqueued with
    h->enc_nsilos = 0;
    GD_TRY(h2d(h, h->enc_tab[0], wire.data(), wire.size()));
    GD_TRY(h2d(h, h->enc_tab[1], type_utf8, n_types ? (size_t)type_off[n_types] : 0));
    GD_TRY(h2d(h, h->enc_tab[2], n_types ? type_off : zero_off, (size_t)n_types + 1));
    GD_TRY(sync(h));
    h->enc_ntypes = n_types;
    h->enc_maxtype = longest;
    h->enc_nsilos = n_silos;
    return GD_OK;
}

int gd_encode_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                            uint32_t n, const uint32_t* d_silo, const uint32_t* d_act, const uint8_t* d_status,
                            const uint8_t* d_placed, const uint32_t* d_new_type, const uint32_t* d_order,
                            uint8_t* d_out_buf, uint64_t out_cap, uint64_t* d_out_off, uint8_t* d_enc_status) {
    GD_TRY(check_encode_state(h, "gd_encode_frames_device"));
    GD_TRY(check_encode_args(h, d_buf, d_frame_off, n, d_silo, d_act, d_status, d_out_buf, out_cap, d_out_off,
                             d_enc_status));
    uint64_t bound = 0;
    GD_TRY(encode_bound(h, buf_len, n, &bound));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_encode_frames_device"));
    return encode_device(h, d_buf, buf_len, d_frame_off, n, d_silo, d_act, d_status, d_placed, d_new_type, d_order,
                         d_out_buf, out_cap, d_out_off, d_enc_status, bound);
}

int gd_encode_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                     const uint32_t* silo, const uint32_t* act, const uint8_t* status, const uint8_t* placed,
                     const uint32_t* new_type, const uint32_t* order, uint8_t* out_buf, uint64_t out_cap,
                     uint64_t* out_off, uint8_t* enc_status, uint64_t* out_total) {
    GD_TRY(check_encode_state(h, "gd_encode_frames"));
    GD_TRY(check_encode_args(h, buf, frame_off, n, silo, act, status, out_buf, out_cap, out_off, enc_status));
    uint64_t bound = 0;
    GD_TRY(encode_bound(h, buf_len, n, &bound));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_encode_frames"));
    if (out_total) *out_total = 0;
    if (n == 0) {
        out_off[0] = 0;
        return GD_OK;
    }
    const uint64_t cap = std::min(out_cap, bound);                 // the total never exceeds the bound
    HostStage io(h);
    const uint8_t* dbuf = io.in(buf, (size_t)buf_len);
    const uint64_t* dfoff = io.in(frame_off, n);
    const uint32_t* dsilo = io.in(silo, n);
    const uint32_t* dact = io.in(act, n);
    const uint8_t* dstatus = io.in(status, n);
    const uint8_t* dplaced = io.in(placed, n);
    const uint32_t* dtype = io.in(new_type, n);
    const uint32_t* dorder = io.in(order, n);
    uint8_t* dout = io.hold<uint8_t>((size_t)cap, 16);           // out_off[n] bytes come down, once that is known
    uint64_t* dooff = io.out(out_off, (size_t)n + 1);
    uint8_t* denc = io.out(enc_status, n, 8);
    GD_TRY(io.status());
    GD_TRY(encode_device(h, dbuf, buf_len, dfoff, n, dsilo, dact, dstatus, dplaced, dtype, dorder, dout, cap, dooff,
                         denc, bound));
    return frameout_fetch(h, io, out_off, n, out_buf, dout, cap, out_total);
}

}  // extern "C"
