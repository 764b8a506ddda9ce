// eng_maintain.hip -- libgraindispatch: the directory cache's maintainer (gd_maintain.h):
// AdaptiveDirectoryCacheMaintainer over the cache table -- the expiry scan and its request lists, the owner's
// LookUpMany, the response pass.  Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_maintain.h"

#include <cmath>

namespace {

// cm_scr slots
enum {
    CM_CNT = 0, CM_CAND, CM_FIRST, CM_RANK, CM_OWNER, CM_FLAG, CM_POS, CM_CKEY, CM_CSLOT, CM_PERM, CM_OFFS, CM_KEYS,
    CM_ITEM, CM_XBYTES, CM_MARK, CM_APPLY
};

int check_cm(gd_handle* h) {
    GD_TRY(cache_check(h));
    if (h->ccap > 0x7FFFFFFFull) return set_err(h, GD_EINVAL, "cache table too large for the maintainer");
    return GD_OK;
}

// The ring's distinct owners as compact indices: cm_own[0][p] for ring position p, cm_own[1][c] the silo.
int owner_table(gd_handle* h) {
    if (h->cm_ring_gen == h->layout_gen && h->cm_own[0].p) return GD_OK;
    std::vector<uint32_t> own(h->ring_n), cown(h->ring_n), silo;
    HIP_TRY(h, hipMemcpyAsync(own.data(), h->ring_own.p, (size_t)h->ring_n * 4, hipMemcpyDeviceToHost, h->stream));
    GD_TRY(sync(h));
    silo = own;
    std::sort(silo.begin(), silo.end());
    silo.erase(std::unique(silo.begin(), silo.end()), silo.end());
    for (uint32_t p = 0; p < h->ring_n; ++p)
        cown[p] = (uint32_t)(std::lower_bound(silo.begin(), silo.end(), own[p]) - silo.begin());
    GD_TRY(h2d(h, h->cm_own[0], cown.data(), cown.size()));
    GD_TRY(h2d(h, h->cm_own[1], silo.data(), silo.size()));
    GD_TRY(sync(h));                                // the vectors are host temporaries
    h->cm_nown = (uint32_t)silo.size();
    h->cm_ring_gen = h->layout_gen;
    return GD_OK;
}

// Run's loop and the request lists; the lists stay in cm_scr.
int scan_run(gd_handle* h, int64_t now, CmCounts* out) {
    GD_TRY(check_cm(h));
    GD_TRY(check_ring(h));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_cache_scan"));
    h->cm_scan_valid = false;
    h->cm_clock = now;
    GD_TRY(owner_table(h));
    DevBuf* S = h->cm_scr;
    const uint32_t cap = (uint32_t)h->ccap, nown = h->cm_nown;
    GD_TRY(ensure(h, S[CM_CNT], sizeof(CmCounts)));
    GD_TRY(ensure(h, S[CM_CAND], (size_t)cap * 4));
    GD_TRY(ensure(h, S[CM_FIRST], (size_t)nown * 4));
    GD_TRY(ensure(h, S[CM_RANK], (size_t)nown * 4));
    GD_TRY(ensure(h, S[CM_OWNER], (size_t)nown * 4));
    CmCounts* cnt = (CmCounts*)S[CM_CNT].p;
    uint32_t* cand = (uint32_t*)S[CM_CAND].p;
    uint32_t* first = (uint32_t*)S[CM_FIRST].p;
    uint32_t* rank = (uint32_t*)S[CM_RANK].p;
    const dim3 g(blocks_for(cap, BLOCK)), b(BLOCK);
    {
        StageTime stage(h, "stage:cache_scan_classify");
        HIP_TRY(h, hipMemsetAsync(cnt, 0, sizeof(CmCounts), h->stream));
        HIP_TRY(h, hipMemsetAsync(first, 0xFF, (size_t)nown * 4, h->stream));
        const RingArgs r = ring_args(h);
        GD_TRY(with_ring_mode(h->ring_mode, [&](auto mode) {
            return launch(h, "k_cm_classify", g, b, ring_lds(h), k_cm_classify<decltype(mode)::value>, h->cslots,
                          (const CacheAge*)h->cage, cap, r, (const uint32_t*)h->cm_own[0].p,
                          (const uint8_t*)h->cache_local.p, h->cache_nsilos, (long long)now, cand, first, nown, h->cctr,
                          cnt);
        }));
        GD_TRY(launch(h, "k_cm_order", dim3(1), b, 0, k_cm_order, (const uint32_t*)first, nown,
                      (const uint32_t*)h->cm_own[1].p, rank, (uint32_t*)S[CM_OWNER].p, cnt));
    }
    HIP_TRY(h, hipMemcpyAsync(out, cnt, sizeof(CmCounts), hipMemcpyDeviceToHost, h->stream));
    GD_TRY(sync(h));
    const uint64_t n64 = out->c[GD_CM_REFRESH];
    const uint32_t n = (uint32_t)n64;
    h->cm_scan_n = n;
    h->cm_scan_owners = out->n_owners;
    h->cm_scan_bytes = 0;
    if (n) {
        StageTime stage(h, "stage:cache_scan_lists");
        GD_TRY(ensure(h, S[CM_FLAG], (size_t)cap * 4));
        GD_TRY(ensure(h, S[CM_POS], (size_t)cap * 4));
        GD_TRY(ensure(h, S[CM_CKEY], (size_t)n * 4 + 64));
        GD_TRY(ensure(h, S[CM_CSLOT], (size_t)n * 4));
        GD_TRY(ensure(h, S[CM_PERM], (size_t)n * 4 + 64));
        GD_TRY(ensure(h, S[CM_OFFS], ((size_t)nown + 2) * 4));
        GD_TRY(ensure(h, S[CM_KEYS], (size_t)n * sizeof(gd_key)));
        GD_TRY(ensure(h, S[CM_ITEM], (size_t)n * 4 * 5));
        uint32_t* flag = (uint32_t*)S[CM_FLAG].p;
        uint32_t* pos = (uint32_t*)S[CM_POS].p;
        uint32_t* ckey = (uint32_t*)S[CM_CKEY].p;
        uint32_t* cslot = (uint32_t*)S[CM_CSLOT].p;
        uint32_t* perm = (uint32_t*)S[CM_PERM].p;
        uint32_t* item = (uint32_t*)S[CM_ITEM].p;
        int32_t* oetag = (int32_t*)item;
        uint32_t* oslot = item + n;
        int32_t* xlen = (int32_t*)(item + 2 * (size_t)n);
        uint32_t* xsize = item + 3 * (size_t)n;
        uint32_t* xoff = item + 4 * (size_t)n;
        GD_TRY(launch(h, "k_cm_flag", g, b, 0, k_cm_flag, (const uint32_t*)cand, cap, flag));
        GD_TRY(scan_device<OpAdd>(h, flag, cap, false, true, "cache_scan", pos));
        GD_TRY(launch(h, "k_cm_compact", g, b, 0, k_cm_compact, (const uint32_t*)cand, (const uint32_t*)pos, cap,
                      (const uint32_t*)rank, ckey, cslot));
        GD_TRY(bucket_device(h, ckey, n, nown, perm, (uint32_t*)S[CM_OFFS].p));
        const dim3 gn(blocks_for(n, BLOCK));
        GD_TRY(launch(h, "k_cm_emit", gn, b, 0, k_cm_emit, (const uint32_t*)perm, (const uint32_t*)cslot, n, h->cslots,
                      (const CacheCounters*)h->cctr, (gd_key*)S[CM_KEYS].p, oetag, oslot, xlen, xsize));
        GD_TRY(launch(h, "k_cm_advance", dim3(1), dim3(WAVE), 0, k_cm_advance, n, h->cctr));
        if (h->cx_used) {                            // KeyExt entries: their strings, compacted
            GD_TRY(scan_device<OpAdd>(h, xsize, n, false, false, "cache_scan", xoff));
            uint32_t tail[2] = {0, 0};
            HIP_TRY(h, hipMemcpyAsync(&tail[0], xoff + n - 1, 4, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipMemcpyAsync(&tail[1], xsize + n - 1, 4, hipMemcpyDeviceToHost, h->stream));
            GD_TRY(sync(h));
            h->cm_scan_bytes = (uint64_t)tail[0] + tail[1];
            if (h->cm_scan_bytes) {
                GD_TRY(ensure(h, S[CM_XBYTES], h->cm_scan_bytes));
                GD_TRY(launch(h, "k_cm_ext_copy", gn, b, 0, k_cm_ext_copy, (const uint32_t*)oslot,
                              (const uint32_t*)xsize, (const uint32_t*)xoff, n, (const CacheSlot*)h->cslots,
                              (const uint8_t*)h->cx_heap.p, (uint8_t*)S[CM_XBYTES].p));
            }
        } else {
            HIP_TRY(h, hipMemsetAsync(xoff, 0, (size_t)n * 4, h->stream));
        }
        GD_TRY(sync_checked(h));
    }
    h->cm_scan_valid = true;
    return GD_OK;
}

void scan_result(gd_handle* h, const CmCounts& c, gd_cache_scan_result* out) {
    DevBuf* S = h->cm_scr;
    const uint32_t n = h->cm_scan_n;
    *out = gd_cache_scan_result{};
    for (int k = 0; k < 5; ++k) out->counts[k] = c.c[k];
    out->n_owners = h->cm_scan_owners;
    out->n = n;
    out->ext_bytes_len = h->cm_scan_bytes;
    if (!n) return;
    const uint32_t* item = (const uint32_t*)S[CM_ITEM].p;
    out->owner = (const uint32_t*)S[CM_OWNER].p;
    out->offsets = (const uint32_t*)S[CM_OFFS].p;
    out->keys = (const gd_key*)S[CM_KEYS].p;
    out->etags = (const int32_t*)item;
    out->slots = item + n;
    out->ext_len = (const int32_t*)(item + 2 * (size_t)n);
    out->ext_off = item + 4 * (size_t)n;
    out->ext_bytes = h->cm_scan_bytes ? (const uint8_t*)S[CM_XBYTES].p : nullptr;
}

// The election words of the apply: one a cache slot, zero between calls.
int mark_words(gd_handle* h, uint32_t** mark) {
    DevBuf& b = h->cm_scr[CM_MARK];
    const size_t need = (size_t)h->ccap * 4;
    const bool fresh = !(b.p && b.bytes >= need);
    GD_TRY(ensure(h, b, need));
    if (fresh) HIP_TRY(h, hipMemsetAsync(b.p, 0, b.bytes, h->stream));
    *mark = (uint32_t*)b.p;
    return GD_OK;
}

// The SAME / ABSENT / HOST items of a response on the device (UPDATED ones: GD_CR_DEFERRED).
int apply_device(gd_handle* h, int64_t now, const gd_key* keys, const ExtArgs& x, const uint8_t* kind, uint32_t n,
                 uint8_t* status) {
    StageTime stage(h, "stage:cache_refresh_apply");
    DevBuf* S = h->cm_scr;
    uint32_t* mark = nullptr;
    GD_TRY(mark_words(h, &mark));
    GD_TRY(ensure(h, S[CM_CNT], sizeof(CmCounts)));
    GD_TRY(ensure(h, S[CM_APPLY], (size_t)n * 4 * 3));
    CmCounts* cnt = (CmCounts*)S[CM_CNT].p;
    uint32_t* slot_of = (uint32_t*)S[CM_APPLY].p;
    uint32_t* hit = slot_of + n;
    uint32_t* pos = hit + n;
    const dim3 g(blocks_for(n, BLOCK)), b(BLOCK);
    HIP_TRY(h, hipMemsetAsync(cnt, 0, sizeof(CmCounts), h->stream));
    GD_TRY(launch(h, "k_cm_find", g, b, 0, k_cm_find, keys, x, kind, n, cache_args(h), mark, slot_of, hit, cnt));
    GD_TRY(scan_device<OpAdd>(h, hit, n, false, true, "cache_apply", pos));
    GD_TRY(launch(h, "k_cm_apply", g, b, 0, k_cm_apply, kind, (const uint32_t*)slot_of, (const uint32_t*)pos, n,
                  h->cslots, h->cage, h->cctr, (const CmCounts*)cnt, mark, (long long)now, (long long)h->cm_max,
                  h->cm_growth, status));
    return launch(h, "k_cm_apply_advance", dim3(1), dim3(WAVE), 0, k_cm_apply_advance, (const uint32_t*)pos, n, h->cctr,
                  (const CmCounts*)cnt);
}

int apply_dup_check(gd_handle* h) {
    CmCounts c{};
    HIP_TRY(h, hipMemcpyAsync(&c, h->cm_scr[CM_CNT].p, sizeof c, hipMemcpyDeviceToHost, h->stream));
    GD_TRY(sync_checked(h));
    if (c.dup) return set_err(h, GD_EINVAL, "refresh response: two items name one cached entry");
    return GD_OK;
}

int lookup_many_device(gd_handle* h, const gd_key* keys, const int32_t* etags, uint32_t n, uint8_t* kind, gd_val* vals,
                       int32_t* tags) {
    StageTime stage(h, "stage:dir_lookup_many");
    return launch(h, "k_dir_lookup_many", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_dir_lookup_many, keys, etags, n,
                  table_args(h), (const uint32_t*)h->vtag, kind, vals, tags);
}

}  // namespace

extern "C" {

int gd_cache_maintain_configure(gd_handle* h, int64_t initial_ticks, int64_t max_ticks, double growth, int64_t now) {
    GD_TRY(cache_check(h));
    if (initial_ticks < 0 || max_ticks < 0) return set_err(h, GD_EINVAL, "gd_cache_maintain_configure: negative ticks");
    if (!std::isfinite(growth) || growth <= 0.0)
        return set_err(h, GD_EINVAL, "gd_cache_maintain_configure: growth is not a positive finite number");
    if ((double)std::max(initial_ticks, max_ticks) * growth >= 4611686018427387904.0)
        return set_err(h, GD_EINVAL, "gd_cache_maintain_configure: timer * growth reaches 2^62");
    h->cm_initial = initial_ticks;
    h->cm_max = max_ticks;
    h->cm_growth = growth;
    h->cm_clock = now;
    return GD_OK;
}

int gd_cache_clock_set(gd_handle* h, int64_t now) {
    GD_TRY(cache_check(h));
    h->cm_clock = now;
    return GD_OK;
}

int gd_cache_entries_age(gd_handle* h, int64_t* refreshed, int64_t* timer, int32_t* num_accesses, uint64_t capacity,
                         uint64_t* out_n) {
    GD_TRY(check_cm(h));
    if (!out_n) return set_err(h, GD_EINVAL, "null argument");
    if (refreshed && (!timer || !num_accesses)) return set_err(h, GD_EINVAL, "null output");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_cache_entries_age"));
    const uint32_t cap = (uint32_t)h->ccap;
    GD_TRY(ensure(h, h->cbuf[0], (size_t)cap * 4));
    GD_TRY(ensure(h, h->cbuf[2], (size_t)cap * 4));
    uint32_t* flag = (uint32_t*)h->cbuf[0].p;
    uint32_t* pos = (uint32_t*)h->cbuf[2].p;
    const dim3 g(blocks_for(cap, BLOCK)), b(BLOCK);
    GD_TRY(launch(h, "k_cache_live_flag", g, b, 0, k_cache_live_flag, (const CacheSlot*)h->cslots, cap, flag));
    GD_TRY(scan_device<OpAdd>(h, flag, cap, false, true, "cache", pos));
    uint32_t total = 0;
    HIP_TRY(h, hipMemcpyAsync(&total, pos + cap - 1, 4, hipMemcpyDeviceToHost, h->stream));
    GD_TRY(sync(h));
    *out_n = total;
    if (!refreshed || total == 0) return GD_OK;
    if (total > capacity)
        return set_err(h, GD_EINVAL, "cache holds %u entries, output holds %llu", total, (unsigned long long)capacity);
    HostStage io(h);
    long long* dr = (long long*)io.out(refreshed, total);
    long long* dt = (long long*)io.out(timer, total);
    int32_t* dn = io.out(num_accesses, total);
    GD_TRY(io.status());
    GD_TRY(launch(h, "k_cm_dump_age", g, b, 0, k_cm_dump_age, (const CacheSlot*)h->cslots, (const CacheAge*)h->cage, cap,
                  (const uint32_t*)flag, (const uint32_t*)pos, dr, dt, dn));
    GD_TRY(io.fetch());
    return sync_checked(h);
}

int gd_cache_scan_device(gd_handle* h, int64_t now, gd_cache_scan_result* out) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (!out) return set_err(h, GD_EINVAL, "null argument");
    CmCounts c{};
    GD_TRY(scan_run(h, now, &c));
    scan_result(h, c, out);
    return GD_OK;
}

int gd_cache_scan(gd_handle* h, int64_t now, uint64_t* out_counts, uint32_t* out_n_owners, uint32_t* out_n,
                  uint64_t* out_bytes) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (!out_counts || !out_n_owners || !out_n || !out_bytes) return set_err(h, GD_EINVAL, "null argument");
    CmCounts c{};
    GD_TRY(scan_run(h, now, &c));
    for (int k = 0; k < 5; ++k) out_counts[k] = c.c[k];
    *out_n_owners = h->cm_scan_owners;
    *out_n = h->cm_scan_n;
    *out_bytes = h->cm_scan_bytes;
    return GD_OK;
}

int gd_cache_scan_fetch(gd_handle* h, uint32_t* owner, uint32_t* offsets, gd_key* keys, int32_t* etags,
                        uint32_t* slots, int32_t* ext_len, uint64_t* ext_off, uint8_t* ext_bytes,
                        uint32_t owner_capacity, uint32_t capacity, uint64_t bytes_capacity) {
    GD_TRY(cache_check(h));
    if (!h->cm_scan_valid) return set_err(h, GD_ESTATE, "gd_cache_scan_fetch: no scan is held");
    const uint32_t n = h->cm_scan_n, no = h->cm_scan_owners;
    if (((owner || offsets) && no > owner_capacity) || n > capacity || (ext_bytes && h->cm_scan_bytes > bytes_capacity))
        return set_err(h, GD_EINVAL, "gd_cache_scan_fetch: %u lists, %u candidates, %llu bytes do not fit the outputs", no,
                       n, (unsigned long long)h->cm_scan_bytes);
    if (offsets) offsets[0] = 0;
    if (!n) return GD_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_cache_scan_fetch"));
    CmCounts c{};
    gd_cache_scan_result r;
    scan_result(h, c, &r);
    HostStage io(h);
    std::vector<uint32_t> xo(ext_off ? n : 0);
    GD_TRY(io.fetch(owner, r.owner, no));
    GD_TRY(io.fetch(offsets, r.offsets, (size_t)no + 1));
    GD_TRY(io.fetch(keys, r.keys, n));
    GD_TRY(io.fetch(etags, r.etags, n));
    GD_TRY(io.fetch(slots, r.slots, n));
    GD_TRY(io.fetch(ext_len, r.ext_len, n));
    if (ext_off) GD_TRY(io.fetch(xo.data(), r.ext_off, n));
    if (ext_bytes && h->cm_scan_bytes) GD_TRY(io.fetch(ext_bytes, r.ext_bytes, h->cm_scan_bytes));
    GD_TRY(sync_checked(h));
    for (uint32_t k = 0; k < (ext_off ? n : 0); ++k) ext_off[k] = xo[k];
    return GD_OK;
}

int gd_dir_lookup_many_device(gd_handle* h, const gd_key* d_keys, const int32_t* d_etags, uint32_t n, uint8_t* d_kind,
                              gd_val* d_vals, int32_t* d_tags) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (n && (!d_keys || !d_etags || !d_kind || !d_vals || !d_tags)) return set_err(h, GD_EINVAL, "null argument");
    if (!n) return GD_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return lookup_many_device(h, d_keys, d_etags, n, d_kind, d_vals, d_tags);
}

int gd_dir_lookup_many(gd_handle* h, const gd_key* keys, const int32_t* etags, uint32_t n, uint8_t* out_kind,
                       gd_val* out_vals, int32_t* out_tags) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (n && (!keys || !etags || !out_kind || !out_vals || !out_tags)) return set_err(h, GD_EINVAL, "null argument");
    if (!n) return GD_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_dir_lookup_many"));
    HostStage io(h);
    const gd_key* dk = io.in(keys, n);
    const int32_t* de = io.in(etags, n);
    uint8_t* dkind = io.out(out_kind, n);
    gd_val* dv = io.out(out_vals, n);
    int32_t* dt = io.out(out_tags, n);
    GD_TRY(io.status());
    GD_TRY(lookup_many_device(h, dk, de, n, dkind, dv, dt));
    GD_TRY(io.fetch());
    return sync_checked(h);
}

int gd_cache_refresh_apply_device(gd_handle* h, int64_t now, const gd_key* d_keys, const gd_key_ext* d_ext,
                                  const uint8_t* d_kind, uint32_t n, uint8_t* d_status) {
    GD_TRY(check_cm(h));
    if (n && (!d_keys || !d_kind)) return set_err(h, GD_EINVAL, "null argument");
    if (n && d_ext && (!d_ext->offset || !d_ext->length)) return set_err(h, GD_EINVAL, "null KeyExt arrays");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_cache_refresh_apply_device"));
    h->cm_clock = now;
    if (!n) return GD_OK;
    ExtArgs x{};
    if (d_ext) x = ExtArgs{d_ext->bytes, d_ext->offset, d_ext->length, d_ext->bytes_len};
    GD_TRY(apply_device(h, now, d_keys, x, d_kind, n, d_status));
    return apply_dup_check(h);
}

int gd_cache_refresh_apply(gd_handle* h, int64_t now, const gd_key* keys, const gd_key_ext* ext, const uint8_t* kind,
                           const gd_val* vals, const int32_t* tags, uint32_t n, uint8_t* out_status) {
    GD_TRY(check_cm(h));
    if (n && (!keys || !kind)) return set_err(h, GD_EINVAL, "null argument");
    if (n && !ext_ok(ext, n)) return set_err(h, GD_EINVAL, "null KeyExt arrays");
    bool any_updated = false;
    for (uint32_t i = 0; i < n; ++i) {
        if (kind[i] > GD_LM_HOST) return set_err(h, GD_EINVAL, "refresh response: kind %u at %u", kind[i], i);
        any_updated |= kind[i] == GD_LM_UPDATED;
    }
    if (any_updated && (!vals || !tags)) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_cache_refresh_apply"));
    h->cm_clock = now;
    if (!n) return GD_OK;
    if (any_updated) {
        StageTime stage(h, "stage:cache_refresh_apply_host");
        return cache_batch_impl(h, keys, ext, kind, vals, tags, n, out_status);
    }
    HostStage io(h);
    const gd_key* dk = io.in(keys, n);
    const uint8_t* dkind = io.in(kind, n);
    uint8_t* dst = io.out_if(out_status, n);
    GD_TRY(io.status());
    ExtArgs x{};
    if (ext) {
        // the strings are checked as the add path checks them (GD_KEYEXT_HOST or a bad range: GD_EINVAL)
        for (uint32_t i = 0; i < n; ++i) {
            if (!is_keyext_cat(keys[i].type_code_data) || kind[i] == GD_LM_HOST) continue;
            const uint8_t* s;
            int32_t len;
            GD_TRY(host_ext(h, ext, i, s, len));
        }
        gd_key_ext dx{};
        GD_TRY(stage_ext(h, ext, n, &dx));
        x = ExtArgs{dx.bytes, dx.offset, dx.length, dx.bytes_len};
    }
    GD_TRY(apply_device(h, now, dk, x, dkind, n, dst));
    GD_TRY(io.fetch());
    return apply_dup_check(h);
}

}  // extern "C"
