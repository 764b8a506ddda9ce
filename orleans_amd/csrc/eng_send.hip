// eng_send.hip -- libgraindispatch: the sender queues of OutboundMessageQueue.SendMessage: the queue
// rule per message and the stable partition of a batch over the sender queues (gd_sendq.h), alone or after the route.
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_sendq.h"

namespace {

// The argument checks that need no handle (so a caller's mistake is reported the same with or without one).
int check_send_outputs(gd_handle* h, const void* perm, const void* offsets) {
    if ((perm != nullptr) != (offsets != nullptr)) return set_err(h, GD_EINVAL, "perm and offsets go together");
    return GD_OK;
}

int check_send_state(gd_handle* h, const char* call) {
    if (!h) return set_err(nullptr, GD_ESTATE, "%s: null handle (no gd_send_configure)", call);
    if (!h->send_nq) return set_err(h, GD_ESTATE, "%s before gd_send_configure", call);
    return GD_OK;
}

// The send stage on device arrays (rs / cat / ttl / q / perm + offsets may be null).
int send_device(gd_handle* h, const uint32_t* silo, const uint8_t* rs, const uint8_t* cat, const int64_t* ttl,
                uint32_t n, uint8_t* st, uint32_t* q, uint32_t* perm, uint32_t* offsets) {
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "send queues: n > 2^31");
    const uint32_t B = h->send_nq + 4;
    if (n == 0) {
        if (!offsets) return GD_OK;
        return launch(h, "k_fill", dim3(blocks_for(B + 1, BLOCK)), dim3(BLOCK), 0, k_fill_u32, offsets, B + 1, 0u);
    }
    StageTime stage(h, "stage:send_queues");
    const bool tab_lds = (size_t)h->send_nsilos * 4 <= SQ_TAB_LDS_BYTES;
    const SendArgs a{(const uint32_t*)h->send_tab.p, h->send_nsilos, h->send_nq, h->cfg.my_silo, tab_lds ? 1u : 0u};
    const uint32_t tiles = blocks_for(n, SQ_TILE);
    const size_t lds_c = sq_classify_lds(B, h->send_nsilos, tab_lds);
    if (!perm)
        return launch(h, "k_sendq_classify", dim3(tiles), dim3(SQ_NT), lds_c, k_sendq_classify, silo, rs, cat, ttl, n, a,
                      tiles, st, q, (uint32_t*)nullptr);
    GD_TRY(ensure(h, h->send_scr[0], ((size_t)B * tiles + B) * 4));
    if (!q) {
        GD_TRY(ensure(h, h->send_scr[1], (size_t)n * 4));
        q = (uint32_t*)h->send_scr[1].p;
    }
    uint32_t* hist = (uint32_t*)h->send_scr[0].p;
    uint32_t* totals = hist + (size_t)B * tiles;
    uint32_t bits = 1;
    while ((1u << bits) < B) ++bits;
    GD_TRY(launch(h, "k_sendq_classify", dim3(tiles), dim3(SQ_NT), lds_c, k_sendq_classify, silo, rs, cat, ttl, n, a,
                  tiles, st, q, hist));
    GD_TRY(launch(h, "k_radix_rowscan", dim3(B), dim3(BLOCK), 0, k_radix_rowscan, hist, tiles, totals));
    GD_TRY(launch(h, "k_sendq_offsets", dim3(1), dim3(SQ_NT), 0, k_sendq_offsets, (const uint32_t*)totals, B, n,
                  offsets));
    return launch(h, "k_sendq_scatter", dim3(tiles), dim3(SQ_NT), sq_scatter_lds(B), k_sendq_scatter,
                  (const uint32_t*)q, n, B, bits, tiles, (const uint32_t*)hist, (const uint32_t*)offsets, perm,
                  h->lane_order ? h->radix_rank_atomic : 0u);
}

// Host-pointer forms: the send stage's optional inputs up, its outputs down, on the caller's staging (which may
// hold the caller's own arrays ahead of these).  silo / rs: device arrays.
int send_host(gd_handle* h, HostStage& io, const uint32_t* d_silo, const uint8_t* d_rs, const uint8_t* category,
              const int64_t* ttl, uint32_t n, uint8_t* out_st, uint32_t* out_q, uint32_t* out_perm,
              uint32_t* out_offsets) {
    const uint32_t B = h->send_nq + 4;
    const uint8_t* dcat = io.in(category, n);
    const int64_t* dttl = io.in(ttl, n);
    uint8_t* dst = io.out(out_st, n, 4);
    uint32_t* dq = io.out_if(out_q, n, 4);
    uint32_t* dperm = io.out_if(out_perm, n, 4);
    uint32_t* doff = io.out_if(out_offsets, (size_t)B + 1);
    GD_TRY(io.status());
    GD_TRY(send_device(h, d_silo, d_rs, dcat, dttl, n, dst, dq, dperm, doff));
    return io.fetch();
}

}  // namespace

extern "C" {

int gd_send_configure(gd_handle* h, const int32_t* silo_hash, uint32_t n_silos, uint32_t n_queues) {
    if (n_queues < 1 || n_queues > SQ_MAX_QUEUES)
        return set_err(h, GD_EINVAL, "gd_send_configure: n_queues %u not in 1..%u", n_queues, SQ_MAX_QUEUES);
    if (n_silos < 1 || n_silos > SQ_MAX_SILOS)
        return set_err(h, GD_EINVAL, "gd_send_configure: n_silos %u not in 1..%u", n_silos, SQ_MAX_SILOS);
    if (!h || !silo_hash) return set_err(h, GD_EINVAL, "gd_send_configure: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    // Math.Abs(hash) % n_queues per silo here, once, not per message on the device (gd_sendq.h)
    std::vector<uint32_t> tab(n_silos);
    for (uint32_t s = 0; s < n_silos; ++s) {
        const int32_t v = silo_hash[s];
        tab[s] = v == INT32_MIN ? SQ_THROWS : 3u + (uint32_t)(v < 0 ? -v : v) % n_queues;
    }
    GD_TRY(sync(h));                               // a batch in flight reads the table it was enqueued with
    h->send_nq = 0;
    GD_TRY(h2d(h, h->send_tab, tab.data(), n_silos));
    GD_TRY(sync(h));
    h->send_nsilos = n_silos;
    h->send_nq = n_queues;
    return GD_OK;
}

int gd_send_queues_device(gd_handle* h, const uint32_t* d_silo, const uint8_t* d_route_status,
                          const uint8_t* d_category, const int64_t* d_ttl, uint32_t n, uint8_t* d_send_status,
                          uint32_t* d_queue, uint32_t* d_perm, uint32_t* d_offsets) {
    GD_TRY(check_send_outputs(h, d_perm, d_offsets));
    GD_TRY(check_send_state(h, "gd_send_queues_device"));
    if (n && (!d_silo || !d_send_status)) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return send_device(h, d_silo, d_route_status, d_category, d_ttl, n, d_send_status, d_queue, d_perm, d_offsets);
}

int gd_send_queues(gd_handle* h, const uint32_t* silo, const uint8_t* route_status, const uint8_t* category,
                   const int64_t* ttl, uint32_t n, uint8_t* out_send_status, uint32_t* out_queue, uint32_t* out_perm,
                   uint32_t* out_offsets) {
    GD_TRY(check_send_outputs(h, out_perm, out_offsets));
    GD_TRY(check_send_state(h, "gd_send_queues"));
    if (n && (!silo || !out_send_status)) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    HostStage io(h);
    const uint32_t* dsilo = io.in(silo, n);
    const uint8_t* drs = io.in(route_status, n);
    GD_TRY(send_host(h, io, dsilo, drs, category, ttl, n, out_send_status, out_queue, out_perm, out_offsets));
    return sync(h);
}

int gd_route_send_device(gd_handle* h, const gd_key* d_keys, uint32_t n, const uint8_t* d_category,
                         const int64_t* d_ttl, uint32_t* d_silo, uint32_t* d_act, uint8_t* d_status,
                         uint8_t* d_send_status, uint32_t* d_queue, uint32_t* d_perm, uint32_t* d_offsets) {
    GD_TRY(check_send_outputs(h, d_perm, d_offsets));
    GD_TRY(check_send_state(h, "gd_route_send_device"));
    if (n && (!d_keys || !d_silo || !d_act || !d_status || !d_send_status)) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    if (n) GD_TRY(route_device(h, d_keys, n, d_silo, d_act, d_status));
    return send_device(h, d_silo, d_status, d_category, d_ttl, n, d_send_status, d_queue, d_perm, d_offsets);
}

int gd_route_send(gd_handle* h, const gd_key* keys, uint32_t n, const uint8_t* category, const int64_t* ttl,
                  uint32_t* out_silo, uint32_t* out_act, uint8_t* out_status, uint8_t* out_send_status,
                  uint32_t* out_queue, uint32_t* out_perm, uint32_t* out_offsets) {
    GD_TRY(check_send_outputs(h, out_perm, out_offsets));
    GD_TRY(check_send_state(h, "gd_route_send"));
    if (n && (!keys || !out_silo || !out_act || !out_status || !out_send_status))
        return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(h2d(h, h->keys_in, keys, n));
    GD_TRY(ensure(h, h->out_a, (size_t)n * 4 + 4));
    GD_TRY(ensure(h, h->out_b, (size_t)n * 4 + 4));
    GD_TRY(ensure(h, h->out_c, (size_t)n + 4));
    if (n)
        GD_TRY(route_device(h, (const gd_key*)h->keys_in.p, n, (uint32_t*)h->out_a.p, (uint32_t*)h->out_b.p,
                            (uint8_t*)h->out_c.p));
    HostStage io(h);
    GD_TRY(send_host(h, io, (const uint32_t*)h->out_a.p, (const uint8_t*)h->out_c.p, category, ttl, n,
                     out_send_status, out_queue, out_perm, out_offsets));
    GD_TRY(d2h(h, out_silo, h->out_a, n));
    GD_TRY(d2h(h, out_act, h->out_b, n));
    GD_TRY(d2h(h, out_status, h->out_c, n));
    return sync_checked(h);
}

}  // extern "C"
