// eng_frameout.hip -- libgraindispatch: what the five stages that write frames into one contiguous output share on
// the host (eng_encode.hip, eng_respond.hip, eng_request.hip, eng_forward.hip, eng_reject.hip): the encoder's tables
// as the kernels take them, a stage's scratch, the offsets of a batch in output order with the capacity check
// (gd_frameout.h), and the end of a host-pointer call.
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_encode.h"

namespace gdx {

EncTab enc_tab(gd_handle* h) {
    return EncTab{(const uint64_t*)h->act_ids.p, h->n_act_ids, (const uint32_t*)h->enc_tab[0].p, h->enc_nsilos,
                  (const uint8_t*)h->enc_tab[1].p, (const uint32_t*)h->enc_tab[2].p, h->enc_ntypes};
}

int frameout_scratch(gd_handle* h, DevBuf* scr, uint32_t n, size_t plan_bytes, size_t plan_pad) {
    GD_TRY(ensure(h, scr[0], (size_t)n * plan_bytes + plan_pad));
    GD_TRY(ensure(h, scr[1], (size_t)n * 4));
    return ensure(h, scr[2], ((size_t)n + 1) * 4 + 16);
}

int frameout_offsets(gd_handle* h, const uint32_t* lens, const uint32_t* order, uint32_t n, uint32_t* offs,
                     uint64_t out_cap, uint64_t* out_off, const char* tag) {
    GD_TRY(launch(h, "k_enc_lens", dim3(blocks_for((uint64_t)n + 1, BLOCK)), dim3(BLOCK), 0, k_enc_lens, lens, order, n,
                  offs));
    GD_TRY(scan_device<OpAdd>(h, offs, n + 1, false, false, tag));
    return launch(h, "k_enc_finish", dim3(blocks_for((uint64_t)n + 1, BLOCK)), dim3(BLOCK), 0, k_enc_finish,
                  (const uint32_t*)offs, n, out_cap, (unsigned long long*)out_off, &h->ctr->err);
}

int frameout_fetch(gd_handle* h, HostStage& io, const uint64_t* out_off, uint32_t n, uint8_t* out_buf,
                   const uint8_t* d_out, uint64_t cap, uint64_t* out_total) {
    GD_TRY(io.fetch());
    GD_TRY(sync(h));
    const uint64_t total = out_off[n];
    if (out_total) *out_total = total;
    if (total && total <= cap) GD_TRY(io.fetch(out_buf, d_out, (size_t)total));
    return sync_checked(h);                                        // a total past out_cap: ERR_ENC_FULL -> GD_EFULL
}

}  // namespace gdx
