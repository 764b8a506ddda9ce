// eng_route.hip -- libgraindispatch: the route launches (24-B keys, N1s, by region, the bound), the KeyExt
// pass, the ring owners and the pipelined host route.
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"

namespace gdx {

#if GD_DIRECT_INDEX
// The direct table for a route that took variant `var` (cx: the indexes are current): *use when the route
// may read it, *d its arguments.  Eligible while the 8-B index is pure, the table is at most half the
// 8-B index's bytes and d <= 2^30; d comes from CxCounters::n1_max of the read-back that showed the index
// pure.  A table built under another snapshot id is never read: the route takes the PURE or general form
// in that same call.  Built (a memset and k_cxd_build on the route's stream, right before the route --
// the stream order the PURE form rests on) only when the previous k_route launch on this handle found the
// index pure under the same snapshot id: a directory that changes between routes never pays for it.
int cxd_prepare(gd_handle* h, bool cx, int var, bool* use, CxdArgs* d) {
    *use = false;
    const bool pure = cx && h->cx8_pure;
    const uint64_t snap = h->cx_snap + h->tab_gen;
    const bool quiet = pure && h->cxd_seen && h->cxd_seen_snap == snap;
    h->cxd_seen = pure;
    h->cxd_seen_snap = snap;
    if (!pure || var != 3) return GD_OK;
    const uint64_t dd = ((uint64_t)h->cx_ctr_host.n1_max + 1 + 15) & ~15ull;
    if (dd * 4 > (uint64_t)h->capacity * 8 / 2 || dd > (1ull << 30)) {
        if (h->cxd_ok) h->cx_snap++;                  // no longer eligible
        h->cxd_ok = false;
        return GD_OK;
    }
    if (!(h->cxd_ok && h->cxd_snap_at == snap && h->cxd_d == dd)) {
        h->cxd_ok = false;
        if (!quiet) return GD_OK;
        GD_TRY(ensure_own(h, h->cxd_tab, dd * 4));    // kept while d fits
        HIP_TRY(h, hipMemsetAsync(h->cxd_tab.p, 0, dd * 4, h->stream));
        const uint32_t g = std::max<uint32_t>(1, std::min<uint64_t>(blocks_for(h->capacity, BLOCK), (uint64_t)h->n_cu * 16));
        GD_TRY(launch(h, "k_cxd_build", dim3(g), dim3(BLOCK), 0, k_cxd_build, (const unsigned long long*)h->cx8_tab.p,
                      (unsigned long long)h->capacity, (uint32_t*)h->cxd_tab.p, (uint32_t)dd));
        h->cxd_ok = true;
        h->cxd_d = (uint32_t)dd;
        h->cxd_snap_at = snap;
        h->cxd_builds++;
    }
    *use = true;
    *d = CxdArgs{(const uint32_t*)h->cxd_tab.p, h->cxd_d, h->cx8_layout.ab, h->cx8_layout.sb, h->cx8_layout.tcd[0]};
    return GD_OK;
}
#endif

// Every k_route launch of one (ring mode, messages a thread M, key width N1W) over the form the tuner
// picks (cx_choose kind 0 / 1).  N1W = 0: 24-B keys, with tcd = 0, rcnt = nullptr, world = 0, src =
// nullptr.  N1W = 8 / 4: keys given as N1 alone (u64 / u32) with one TypeCodeData (a compact exchange
// receive); src (optional): also the sender rank of every message, from the per-sender counts
// rcnt[world].  Not in cache mode.  NT: the key stream is read non-temporally -- by every form of the
// 24-B route, but of the N1 routes only by the direct table and the 8-B index (their 16-B-index and
// directory forms are always temporal, and they have no pure 8-B form).
template <int MODE, int M, bool NT, int N1W>
int route_form(gd_handle* h, const gd_key* keys, uint64_t tcd, uint32_t n, uint32_t* silo, uint32_t* act,
               uint8_t* status, const uint32_t* rcnt, uint32_t world, uint32_t* src) {
    constexpr bool NT16 = N1W == 0 && NT;           // the 16-B-index and directory forms' key stream
    constexpr int G = (int)CX_GROUP;
    bool cx = false;
    GD_TRY(cx_ensure(h, &cx, n));
    int meas = -1;
    const int var = cx ? cx_choose(h, N1W ? 1 : 0, n, &meas, h->cx8_ok ? 4 : 3) : 1;
    // the launch, timed for the tuner: the bracket opens after cxd_prepare, so a table build is not part
    // of the variant's timing
    const auto go = [&](auto kernel, auto... index) {
        CxMeasure m(h, meas, n);
        return launch(h, "k_route", dim3(blocks_for(n, BLOCK * M)), dim3(BLOCK), ring_lds(h), kernel, keys, n,
                      ring_args(h), table_args(h), silo, act, status, tcd, h->route_xcd ? 1u : 0u, rcnt, world, src,
                      index...);
    };
#if GD_DIRECT_INDEX
    bool direct = false;
    CxdArgs cxd{};
    GD_TRY(cxd_prepare(h, cx, var, &direct, &cxd));
    if (direct) return go(k_route_d<MODE, M, NT, N1W>, cxd);
#endif
    if constexpr (N1W == 0)                  // nothing to fall back to the directory for (gd_engine.h cx8_pure)
        if (var == 3 && h->cx8_pure) return go(k_route_m<MODE, M, NT, 0, false, G, true, true>, CxArgs{}, cx8_args(h));
    if (var == 3) return go(k_route_m<MODE, M, NT, N1W, false, G, true>, CxArgs{}, cx8_args(h));
    if (var == 0) return go(k_route_m<MODE, M, NT16, N1W, true>, cx_args(h), Cx8Args{});
    if (var == 2) return go(k_route_m<MODE, M, NT16, N1W, true, 1>, cx_args(h), Cx8Args{});
    return go(k_route_m<MODE, M, NT16, N1W>, CxArgs{}, Cx8Args{});
}

// src (optional): also the sender rank of every message, from the per-sender counts rcnt[world].
int route_n1_device(gd_handle* h, const void* n1s, uint32_t n1w, uint64_t tcd, uint32_t n, uint32_t* silo,
                    uint32_t* act, uint8_t* status, const uint32_t* rcnt, uint32_t world,
                    uint32_t* src) {
    GD_TRY(check_ring(h));
    h->routed += n;
    const gd_key* k = reinterpret_cast<const gd_key*>(n1s);
    // the N1 stream non-temporal under route_mode's rule (world-1 exchange pipeline: 0.5791 -> 0.5773 ms,
    // profiles/r05_route_n1_nt_ab.txt)
    const bool nt = (uint64_t)h->capacity * 8u <= ROUTE_NT_INDEX_BYTES;
    return with_ring_mode(h->ring_mode, [&](auto mode) {
        constexpr int MODE = decltype(mode)::value;
        if (nt && n1w == 4) return route_form<MODE, 1, true, 4>(h, k, tcd, n, silo, act, status, rcnt, world, src);
        if (nt) return route_form<MODE, 1, true, 8>(h, k, tcd, n, silo, act, status, rcnt, world, src);
        if (n1w == 4) return route_form<MODE, 1, false, 4>(h, k, tcd, n, silo, act, status, rcnt, world, src);
        return route_form<MODE, 1, false, 8>(h, k, tcd, n, silo, act, status, rcnt, world, src);
    });
}

// The owner's region-mapped probe (k_route_region) over m received messages: 24-B keys (n1w = 0) or
// N1s with one TypeCodeData; seg from k_region_segments.  Not in cache mode.
template <int MODE>
int route_region_mode(gd_handle* h, const void* k, uint32_t n1w, uint64_t tcd, uint32_t m, const uint32_t* seg,
                      uint32_t world, uint32_t* silo, uint32_t* act, uint8_t* status) {
    const dim3 g(N_REGIONS * std::max<uint32_t>(1, blocks_for(m, N_REGIONS * BLOCK))), b(BLOCK);
    const gd_key* kk = reinterpret_cast<const gd_key*>(k);
    if (n1w == 4)
        return launch(h, "k_route", g, b, ring_lds(h), k_route_region<MODE, 4>, kk, m, ring_args(h), table_args(h),
                      silo, act, status, tcd, seg, world);
    if (n1w == 8)
        return launch(h, "k_route", g, b, ring_lds(h), k_route_region<MODE, 8>, kk, m, ring_args(h), table_args(h),
                      silo, act, status, tcd, seg, world);
    return launch(h, "k_route", g, b, ring_lds(h), k_route_region<MODE, 0>, kk, m, ring_args(h), table_args(h), silo,
                  act, status, 0ull, seg, world);
}

int route_region_device(gd_handle* h, const void* k, uint32_t n1w, uint64_t tcd, uint32_t m, const uint32_t* seg,
                        uint32_t world, uint32_t* silo, uint32_t* act, uint8_t* status) {
    GD_TRY(check_ring(h));
    h->routed += m;
    return with_ring_mode(h->ring_mode, [&](auto mode) {
        return route_region_mode<decltype(mode)::value>(h, k, n1w, tcd, m, seg, world, silo, act, status);
    });
}

// A cache-sized probe index (<= 64 MB of 8-B slots: BASELINE cfg 2's 16 MB): one message a thread (2
// measured no faster, profiles/r03_route_cx_ab.txt) and the 24-B key stream read non-temporally, so it
// does not push the index out of L2 (k_route 0.292 -> 0.285 ms, the step 0.415 -> 0.406 ms).  A larger
// one (cfg 3's 2 GB, its Zipf-hot part in L2 and the MALL): temporal reads (0.882 against 0.905 ms
// non-temporal; profiles/r05_route_nt_ab.txt) and two messages a thread, two dependent key -> probe
// chains in flight (0.878 -> 0.863 ms; 4: 0.963; profiles/r05_route_m_ab.txt).  act is stored
// temporally either way: the bucketing's histogram reads it next.
template <int MODE>
int route_mode(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t* silo, uint32_t* act, uint8_t* status) {
    const uint64_t index_bytes = (uint64_t)h->capacity * 8u;
    if (index_bytes <= ROUTE_NT_INDEX_BYTES)
        return route_form<MODE, 1, true, 0>(h, keys, 0ull, n, silo, act, status, nullptr, 0u, nullptr);
    return route_form<MODE, 2, false, 0>(h, keys, 0ull, n, silo, act, status, nullptr, 0u, nullptr);
}

// gd_route_bound_device: k_route_bound over the current 8-B index, with route_mode's key-stream rule.
int route_bound_device(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t* silo, uint32_t* act,
                       uint8_t* status) {
    GD_TRY(check_ring(h));
    bool cx = false;
    GD_TRY(cx_ensure(h, &cx, n));
    if (!cx || !h->cx8_ok) return set_err(h, GD_EINVAL, "route bound: the directory has no 8-B probe index");
    const uint32_t xcd = h->route_xcd ? 1u : 0u;
    const unsigned long long mask = h->capacity - 1ull;
    // two messages a thread: the fastest of the forms measured (profiles/r06_route_bound_forms.json: one
    // a thread 0.328-0.336 ms with or without the ring-staging barrier and non-temporal keys, two 0.286,
    // four 0.288; k_route 0.288)
    const bool nt = (uint64_t)h->capacity * 8u <= ROUTE_NT_INDEX_BYTES;
    const dim3 g2(blocks_for(n, BLOCK * 2));
    if (nt)
        return launch(h, "k_route_bound", g2, dim3(BLOCK), ring_lds(h), k_route_bound<2, true>, keys, n, mask,
                      cx8_args(h), silo, act, status, xcd);
    return launch(h, "k_route_bound", g2, dim3(BLOCK), ring_lds(h), k_route_bound<2, false>, keys, n, mask,
                  cx8_args(h), silo, act, status, xcd);
}


// touch = false (LocalLookup mode only): leave the batch's generation updates to the KeyExt pass
// that follows, so plain and KeyExt cache hits are numbered in one batch order.
int route_device(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t* silo, uint32_t* act, uint8_t* status,
                 bool touch) {
    GD_TRY(check_ring(h));
    h->routed += n;
    if (h->cache_max) return route_cached(h, keys, n, silo, act, status, touch);
    return with_ring_mode(h->ring_mode, [&](auto mode) {
        return route_mode<decltype(mode)::value>(h, keys, n, silo, act, status);
    });
}

KxArgs kx_args(gd_handle* h) {
    return KxArgs{h->kx_slots, h->kx_cap ? h->kx_cap - 1 : 0ull, h->kx_maxp, (const uint8_t*)h->kx_heap.p,
                  (const uint32_t*)h->dir_valid.p, h->n_valid};
}

template <int MODE>
int route_keyext_t(gd_handle* h, const gd_key* keys, const ExtArgs& x, uint32_t n, uint32_t* silo, uint32_t* act,
                   uint8_t* st) {
    return launch(h, "k_route_keyext", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), ring_lds(h), k_route_keyext<MODE>,
                  keys, n, x, ring_args(h), kx_args(h), silo, act, st);
}

// The KeyExt pass (gd_keyext.h) over the messages route_device left at GD_ROUTE_KEYEXT.  In
// LocalLookup (cache) mode it follows route_device(..., touch = false) over the same batch: the
// KeyExt LocalLookup, then the generation updates of every cache hit of the batch.
int keyext_pass(gd_handle* h, const gd_key* keys, const ExtArgs& x, uint32_t n, uint32_t* silo, uint32_t* act,
                uint8_t* st) {
    if (n == 0) return GD_OK;
    if (h->cache_max) return route_cached_keyext(h, keys, x, n, silo, act, st);
    return with_ring_mode(h->ring_mode, [&](auto mode) {
        return route_keyext_t<decltype(mode)::value>(h, keys, x, n, silo, act, st);
    });
}

int ring_owner_device(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t* silo) {
    GD_TRY(check_ring(h));
    return with_ring_mode(h->ring_mode, [&](auto mode) {
        return launch(h, "k_ring_owner", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), ring_lds(h),
                      k_route<decltype(mode)::value, false>, keys, n, ring_args(h), table_args(h), silo,
                      (uint32_t*)nullptr, (uint8_t*)nullptr);
    });
}

// Page-locked host memory (hipHostMalloc / gd_host_alloc / hipHostRegister): copies from it are
// asynchronous.  From pageable memory HIP stages every copy, and the chunked pipeline measured
// slower than one copy each way (1.35 vs 1.42 G messages/s at cfg 2).
bool host_pinned(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// gd_route / gd_route_bucket on pinned host buffers, large batch: host_pipeline (gd_engine.h) over the 24-B
// key stream up and silo / act / status down; bounded by the 24-B-a-message upload instead of the sum of
// both directions.  out_perm == nullptr: gd_route (routes only, no bucketing).
int route_bucket_host_pipelined(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t n_act, uint32_t* out_silo,
                                uint32_t* out_act, uint8_t* out_status, uint32_t* out_perm, uint32_t* out_offsets) {
    GD_TRY(ensure(h, h->keys_in, (size_t)n * sizeof(gd_key)));
    GD_TRY(ensure(h, h->out_a, (size_t)n * 4 + 4));
    GD_TRY(ensure(h, h->out_b, (size_t)n * 4 + 4));
    GD_TRY(ensure(h, h->out_c, (size_t)n + 4));
    const bool bucket = out_perm != nullptr;        // gd_route: routes only
    if (bucket) {
        GD_TRY(ensure(h, h->u8_a, (size_t)n * 4 + 4));
        GD_TRY(ensure(h, h->offs, ((size_t)n_act + 2) * 4));
    }
    gd_key* dk = (gd_key*)h->keys_in.p;
    uint32_t* silo = (uint32_t*)h->out_a.p;
    uint32_t* act = (uint32_t*)h->out_b.p;
    uint8_t* st = (uint8_t*)h->out_c.p;
    const HpStream up[1] = {{(void*)keys, dk, sizeof(gd_key)}};
    const HpStream down[3] = {{out_silo, silo, 4}, {out_act, act, 4}, {out_status, st, 1}};
    const HpTail tail[2] = {{out_perm, h->u8_a.p, (size_t)n * 4}, {out_offsets, h->offs.p, ((size_t)n_act + 2) * 4}};
    return host_pipeline(
        h, n, up, 1, down, 3,
        [&](size_t off, uint32_t cnt) { return route_device(h, dk + off, cnt, silo + off, act + off, st + off); }, act,
        n_act, bucket ? (uint32_t*)h->u8_a.p : nullptr, bucket ? (uint32_t*)h->offs.p : nullptr, tail, bucket ? 2 : 0);
}

}  // namespace gdx
