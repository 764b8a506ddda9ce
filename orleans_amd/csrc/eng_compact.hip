// eng_compact.hip -- libgraindispatch: the compact route.  The class table, the launches of
// k_route_compact over the 24-B route's probe forms, the simple form of LocalLookup mode, and the entry
// points gd_classes_*, gd_route_compact*, gd_route_bucket_compact*.
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_compact.h"

namespace gdx {

// The probe variant of a compact launch: the one the 24-B route (tune kind GD_TUNE_PROBE_KEYS) is pinned to
// or has picked for this size class, read without creating, timing or changing a tune entry; while that
// kind has picked none, the 8-B index where it is built and the 16-B index's group reads elsewhere.
// Variants as cx_choose's: 0 index groups, 1 the directory, 2 index slots, 3 the 8-B index.
static int compact_variant(const gd_handle* h, uint64_t n, int nvar) {
    if (h->cx_mode == 2) return 0;
    if (h->cx_mode == 3) return 2;
    if (h->cx_mode == 4) return nvar > 3 ? 3 : 0;
    const int pin = h->tune_pin[GD_TUNE_PROBE_KEYS];
    if (pin >= 0 && pin < nvar) return pin;
    const auto it = h->cx_tune.find(tune_key(GD_TUNE_PROBE_KEYS, n, 0));
    if (it != h->cx_tune.end() && it->second.pick >= 0 && it->second.pick < nvar) return it->second.pick;
    return nvar > 3 ? 3 : 0;
}

// One k_route_compact launch of (ring mode, key-stream rule, N1 width) in the form route_form would take
// for the same batch of 24-B keys: the direct table, the pure 8-B index, the 8-B index, the 16-B index in
// group or slot reads, the directory.
template <int MODE, bool NT, int N1W>
static int compact_form(gd_handle* h, const uint8_t* cls, const void* n1s, uint32_t n, uint32_t* act, uint16_t* silo16,
                        uint8_t* status, uint32_t* wide) {
    bool cx = false;
    GD_TRY(cx_ensure(h, &cx, n));
    const int var = cx ? compact_variant(h, n, h->cx8_ok ? 4 : 3) : 1;
    const auto go = [&](auto kernel, const CxArgs& a, const Cx8Args& b, const CxdArgs& d) {
        return launch(h, "k_route_compact", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), ring_lds(h), kernel, cls, n1s, n,
                      (const unsigned long long*)h->cls_tab.p, (uint32_t)h->cls_host.size(), ring_args(h),
                      table_args(h), act, silo16, status, wide, h->route_xcd ? 1u : 0u, a, b, d);
    };
#if GD_DIRECT_INDEX
    bool direct = false;
    CxdArgs cxd{};
    GD_TRY(cxd_prepare(h, cx, var, &direct, &cxd));
    if (direct) return go(k_route_compact<MODE, NT, N1W, CF_DIRECT>, CxArgs{}, Cx8Args{}, cxd);
#endif
    if (var == 3 && h->cx8_pure)
        return go(k_route_compact<MODE, NT, N1W, CF_INDEX8_PURE>, CxArgs{}, cx8_args(h), CxdArgs{});
    if (var == 3) return go(k_route_compact<MODE, NT, N1W, CF_INDEX8>, CxArgs{}, cx8_args(h), CxdArgs{});
    if (var == 0) return go(k_route_compact<MODE, NT, N1W, CF_INDEX16>, cx_args(h), Cx8Args{}, CxdArgs{});
    if (var == 2) return go(k_route_compact<MODE, NT, N1W, CF_INDEX16_SLOT>, cx_args(h), Cx8Args{}, CxdArgs{});
    return go(k_route_compact<MODE, NT, N1W, CF_DIRECTORY>, CxArgs{}, Cx8Args{}, CxdArgs{});
}

// LocalLookup (cache) mode: the records expanded into the handle's key scratch, the cache route with its
// hit / touch order, and the routes packed.
static int compact_route_cached(gd_handle* h, const uint8_t* cls, const void* n1s, uint32_t n1w, uint32_t n,
                                uint32_t* act, uint16_t* silo16, uint8_t* status, uint32_t* wide) {
    GD_TRY(ensure(h, h->keys_in, (size_t)n * sizeof(gd_key)));
    GD_TRY(ensure(h, h->cls_silo, (size_t)n * 4));
    gd_key* keys = (gd_key*)h->keys_in.p;
    uint32_t* silo = (uint32_t*)h->cls_silo.p;
    const unsigned long long* tab = (const unsigned long long*)h->cls_tab.p;
    const uint32_t nc = (uint32_t)h->cls_host.size();
    const dim3 g(blocks_for(n, BLOCK)), b(BLOCK);
    if (n1w == 4) GD_TRY(launch(h, "k_compact_expand", g, b, 0, k_compact_expand<4>, cls, n1s, n, tab, nc, keys));
    else GD_TRY(launch(h, "k_compact_expand", g, b, 0, k_compact_expand<8>, cls, n1s, n, tab, nc, keys));
    GD_TRY(route_device(h, keys, n, silo, act, status));
    return launch(h, "k_compact_pack", g, b, 0, k_compact_pack, cls, n, nc, (const uint32_t*)silo, act, silo16, status,
                  wide);
}

// The compact route of n records on the handle's stream.  wide (optional): the silos that do not fit 16
// bits are added to *wide (the caller zeroes it).
int compact_route_device(gd_handle* h, const uint8_t* cls, const void* n1s, uint32_t n1w, uint32_t n, uint32_t* act,
                         uint16_t* silo16, uint8_t* status, uint32_t* wide) {
    GD_TRY(check_ring(h));
    if (n == 0) return GD_OK;
    if (h->cache_max) return compact_route_cached(h, cls, n1s, n1w, n, act, silo16, status, wide);
    h->routed += n;
    const bool nt = (uint64_t)h->capacity * 8u <= ROUTE_NT_INDEX_BYTES;   // route_mode's rule
    return with_ring_mode(h->ring_mode, [&](auto mode) {
        constexpr int MODE = decltype(mode)::value;
        if (nt && n1w == 4) return compact_form<MODE, true, 4>(h, cls, n1s, n, act, silo16, status, wide);
        if (nt) return compact_form<MODE, true, 8>(h, cls, n1s, n, act, silo16, status, wide);
        if (n1w == 4) return compact_form<MODE, false, 4>(h, cls, n1s, n, act, silo16, status, wide);
        return compact_form<MODE, false, 8>(h, cls, n1s, n, act, silo16, status, wide);
    });
}

// The checks every compact route shares; *go = false: n = 0, nothing to route.
static int compact_check(gd_handle* h, const uint8_t* cls, const void* n1, uint32_t n1_width, uint32_t n,
                         const void* act, const void* silo16, const void* status, bool* go) {
    *go = false;
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (n1_width != 4 && n1_width != 8) return set_err(h, GD_EINVAL, "n1_width %u is neither 4 nor 8", n1_width);
    if (n && (!n1 || !act || !silo16 || !status)) return set_err(h, GD_EINVAL, "null argument");
    if (n == 0) return GD_OK;
    if (h->cls_host.empty())
        return set_err(h, GD_ESTATE, cls ? "no class table set (gd_classes_set)"
                                         : "no class table set: class 0 is absent (gd_classes_set)");
    *go = true;
    return GD_OK;
}

static int compact_wide_error(gd_handle* h, uint32_t wide) {
    if (!wide) return GD_OK;
    return set_err(h, GD_EINVAL, "%u routes have a silo index that does not fit 16 bits (GD_NO_SILO16 stored)", wide);
}

// The host forms: out_perm == nullptr: routes only.
static int compact_host(gd_handle* h, const uint8_t* cls, const void* n1, uint32_t w, uint32_t n, uint32_t n_act,
                        uint32_t* out_act, uint16_t* out_silo16, uint8_t* out_status, uint32_t* out_perm,
                        uint32_t* out_offsets) {
    const bool bucket = out_offsets != nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(ensure(h, h->cls_wide, 4));
    uint32_t* d_wide = (uint32_t*)h->cls_wide.p;
    uint32_t wide = 0;
    HostStage st(h);
    const bool pipe = h->host_chunk && n >= 2 * (uint64_t)h->host_chunk && !h->cache_max && host_pinned(n1) &&
                      (!cls || host_pinned(cls)) && host_pinned(bucket ? (const void*)out_perm : (const void*)out_act);
    if (pipe) {
        // large pinned batch: the chunk pipeline of the 24-B forms over the record streams
        uint8_t* d_cls = st.hold<uint8_t>(n, 0, cls != nullptr);
        uint8_t* d_n1 = st.hold<uint8_t>((size_t)n * w);
        uint32_t* d_act = st.hold<uint32_t>(n, 4);
        uint16_t* d_silo = st.hold<uint16_t>(n, 4);
        uint8_t* d_st = st.hold<uint8_t>(n, 4);
        uint32_t* d_perm = st.hold<uint32_t>(n, 4, bucket);
        uint32_t* d_offs = st.hold<uint32_t>((size_t)n_act + 2, 0, bucket);
        GD_TRY(st.status());
        HIP_TRY(h, hipMemsetAsync(d_wide, 0, 4, h->stream));
        HpStream up[2];
        int n_up = 0;
        if (cls) up[n_up++] = HpStream{(void*)cls, d_cls, 1};
        up[n_up++] = HpStream{(void*)n1, d_n1, w};
        const HpStream down[3] = {{out_act, d_act, 4}, {out_silo16, d_silo, 2}, {out_status, d_st, 1}};
        HpTail tail[3];
        int n_tail = 0;
        if (bucket) {
            tail[n_tail++] = HpTail{out_perm, d_perm, (size_t)n * 4};
            tail[n_tail++] = HpTail{out_offsets, d_offs, ((size_t)n_act + 2) * 4};
        }
        tail[n_tail++] = HpTail{&wide, d_wide, 4};
        GD_TRY(host_pipeline(
            h, n, up, n_up, down, 3,
            [&](size_t off, uint32_t cnt) {
                return compact_route_device(h, cls ? d_cls + off : nullptr, d_n1 + off * w, w, cnt, d_act + off,
                                            d_silo + off, d_st + off, d_wide);
            },
            d_act, n_act, d_perm, d_offs, tail, n_tail));
        return compact_wide_error(h, wide);
    }
    // small or pageable: one copy each way through the staging helper
    const uint8_t* d_cls = st.in(cls, n);
    const uint8_t* d_n1 = st.in((const uint8_t*)n1, (size_t)n * w);
    uint32_t* d_act = st.out(out_act, n, 4);
    uint16_t* d_silo = st.out(out_silo16, n, 4);
    uint8_t* d_st = st.out(out_status, n, 4);
    uint32_t* d_perm = bucket ? st.out(out_perm, n, 4) : st.hold<uint32_t>(0, 0, false);
    uint32_t* d_offs = bucket ? st.out(out_offsets, (size_t)n_act + 2) : st.hold<uint32_t>(0, 0, false);
    GD_TRY(st.status());
    HIP_TRY(h, hipMemsetAsync(d_wide, 0, 4, h->stream));
    if (n) GD_TRY(compact_route_device(h, d_cls, d_n1, w, n, d_act, d_silo, d_st, d_wide));
    if (bucket) GD_TRY(bucket_device(h, d_act, n, n_act, d_perm, d_offs));
    GD_TRY(st.fetch());
    GD_TRY(st.fetch(&wide, d_wide, 1));
    GD_TRY(bucket ? sync_checked(h) : sync(h));
    return compact_wide_error(h, wide);
}

}  // namespace gdx

extern "C" {

int gd_classes_set(gd_handle* h, const uint64_t* type_code_data, uint32_t n) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (n > COMPACT_CLASSES) return set_err(h, GD_EINVAL, "%u classes: at most %u", n, COMPACT_CLASSES);
    if (n && !type_code_data) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(ensure(h, h->cls_tab, COMPACT_CLASSES * sizeof(uint64_t)));
    GD_TRY(sync(h));                                 // routes in flight read the table being replaced
    h->cls_host.assign(type_code_data, type_code_data + n);
    if (n) HIP_TRY(h, hipMemcpyAsync(h->cls_tab.p, h->cls_host.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    return sync(h);
}

int gd_classes_get(gd_handle* h, uint64_t* out, uint32_t max, uint32_t* out_n) {
    if (!h || !out_n || (max && !out)) return set_err(h, GD_EINVAL, "null argument");
    const uint32_t n = (uint32_t)h->cls_host.size();
    *out_n = n;
    for (uint32_t i = 0; i < std::min(n, max); ++i) out[i] = h->cls_host[i];
    return GD_OK;
}

int gd_route_compact_device(gd_handle* h, const uint8_t* d_cls, const void* d_n1, uint32_t n1_width, uint32_t n,
                            uint32_t* d_act, uint16_t* d_silo16, uint8_t* d_status, uint32_t* d_wide) {
    bool go = false;
    GD_TRY(compact_check(h, d_cls, d_n1, n1_width, n, d_act, d_silo16, d_status, &go));
    if (d_wide) HIP_TRY(h, hipMemsetAsync(d_wide, 0, 4, h->stream));
    return go ? compact_route_device(h, d_cls, d_n1, n1_width, n, d_act, d_silo16, d_status, d_wide) : GD_OK;
}

int gd_route_bucket_compact_device(gd_handle* h, const uint8_t* d_cls, const void* d_n1, uint32_t n1_width, uint32_t n,
                                   uint32_t n_act, uint32_t* d_act, uint16_t* d_silo16, uint8_t* d_status,
                                   uint32_t* d_perm, uint32_t* d_offsets, uint32_t* d_wide) {
    bool go = false;
    GD_TRY(compact_check(h, d_cls, d_n1, n1_width, n, d_act, d_silo16, d_status, &go));
    if (!d_offsets || (n && !d_perm)) return set_err(h, GD_EINVAL, "null argument");
    if (d_wide) HIP_TRY(h, hipMemsetAsync(d_wide, 0, 4, h->stream));
    if (go) GD_TRY(compact_route_device(h, d_cls, d_n1, n1_width, n, d_act, d_silo16, d_status, d_wide));
    return bucket_after_route(h, d_act, n, n_act, d_perm, d_offsets);
}

int gd_route_compact(gd_handle* h, const uint8_t* cls, const void* n1, uint32_t n1_width, uint32_t n, uint32_t* out_act,
                     uint16_t* out_silo16, uint8_t* out_status) {
    bool go = false;
    GD_TRY(compact_check(h, cls, n1, n1_width, n, out_act, out_silo16, out_status, &go));
    return go ? compact_host(h, cls, n1, n1_width, n, 0, out_act, out_silo16, out_status, nullptr, nullptr) : GD_OK;
}

int gd_route_bucket_compact(gd_handle* h, const uint8_t* cls, const void* n1, uint32_t n1_width, uint32_t n,
                            uint32_t n_act, uint32_t* out_act, uint16_t* out_silo16, uint8_t* out_status,
                            uint32_t* out_perm, uint32_t* out_offsets) {
    bool go = false;
    GD_TRY(compact_check(h, cls, n1, n1_width, n, out_act, out_silo16, out_status, &go));
    if (!out_offsets || (n && !out_perm)) return set_err(h, GD_EINVAL, "null argument");
    if (n_act == 0xFFFFFFFFu) return set_err(h, GD_EINVAL, "n_act too large");
    return compact_host(h, cls, n1, n1_width, n, n_act, out_act, out_silo16, out_status, out_perm, out_offsets);
}

}  // extern "C"
