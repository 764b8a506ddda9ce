// gd_maintain.h -- gfx950 device code for the directory cache's maintainer:
// AdaptiveDirectoryCacheMaintainer.Run (src/Orleans.Runtime/GrainDirectory/AdaptiveDirectoryCacheMaintainer.cs
// :42-131), its request lists (SendBatchCacheRefreshRequests :133-153, BuildGrainAndETagList :202-224), the
// owner's RemoteGrainDirectory.LookUpMany (RemoteGrainDirectory.cs:65-96) and the response pass
// (ProcessCacheRefreshResponse :155-193) over the cache table of gd_cache.h.
//
// Per-entry state: NumAccesses in the slot (CacheSlot::nacc), LastRefreshed and ExpirationTimer in the CacheAge
// array beside the slots.  Created (AdaptiveGrainDirectoryCache.cs:13) is never read on this path and is not stored.
//
// The reference enumerates a ConcurrentDictionary, whose order is unspecified; here the enumeration order is
// ascending cache slot, the order of gd_cache_entries.  The request lists follow from it: owners in order of
// first appearance, one owner's candidates in enumeration order.  Every candidate takes the next LRU
// generation in that grouped order (BuildGrainAndETagList's cache.Get is LRU.TryGetValue, LRU.cs:124-163).
// Nothing depends on the order atomics arrive in: the counts are sums, the first positions minima, the
// partition a stable bucketing.
//
// Integer table walks, 64 B a slot plus 16 B of times for a live non-local entry: HBM-bound, no MFMA.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_cache.h"
#include "gd_common.h"
#include "gd_dirops.h"
#include "gd_hash.h"
#include "gd_probe.h"
#include "graindispatch.h"

namespace gd {

constexpr uint32_t CM_LDS_OWN = 1024;      // distinct ring owners whose first positions a workgroup keeps in LDS

struct CmCounts {
    unsigned long long c[5];               // entries seen, self-owned, fresh, dropped, to refresh (cnt1..cnt4 of :63)
    uint32_t n_owners;
    uint32_t dup;                          // apply: two items of a batch on one cached entry
};

// Run's loop (:66-119) over the slots.  cand[j] = the compact index of the owner whose list entry j joins, NONE32
// for every other slot; first[c] = the lowest slot among owner c's candidates.
template <int MODE>
static __global__ void __launch_bounds__(BLOCK) k_cm_classify(CacheSlot* slots, const CacheAge* __restrict__ age,
                                                       uint32_t cap, RingArgs ring, const uint32_t* __restrict__ cown,
                                                       const uint8_t* __restrict__ local, uint32_t n_local,
                                                       long long now, uint32_t* __restrict__ cand,
                                                       uint32_t* __restrict__ first, uint32_t nown, CacheCounters* ctr,
                                                       CmCounts* cnt) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_ring[];
    __shared__ uint32_t s_first[CM_LDS_OWN];
    __shared__ uint32_t s_cnt[5];
    uint32_t* s_pts = s_ring;
    uint32_t* s_own = s_ring + ring.n;
    const bool lds_first = nown <= CM_LDS_OWN;
    if (lds_first)
        for (uint32_t c = threadIdx.x; c < nown; c += BLOCK) s_first[c] = NONE32;
    if (threadIdx.x < 5) s_cnt[threadIdx.x] = 0;
    stage_ring(ring, s_pts, s_own);
    __syncthreads();
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t cls = 0, c = NONE32;
    if (j < cap) {
        const CacheSlot s = slots[j];
        if (slot_state(s.meta) == SLOT_LIVE) {
            const uint32_t p = ring_position<MODE>(s_pts, ring.n, ring.top, cache_slot_hash(s));
            const uint32_t owner = s_own[p];
            if (owner < n_local && local[owner]) {
                cls = 1;                                           // our own entry (:79-86)
            } else {
                const CacheAge a = age[j];
                if (now < a.refreshed + a.timer) cls = 2;          // !IsExpired (:95-99; IsExpired is >=)
                else if (s.nacc == 0) cls = 3;                     // expired, not accessed (:100-105)
                else {                                             // expired, accessed (:106-117)
                    cls = 4;
                    c = cown[p];
                    slots[j].nacc = 0;
                }
            }
            if (cls == 1 || cls == 3) slots[j].meta = make_meta(SLOT_TOMB, 0);
        }
        cand[j] = c;
    }
    const bool lane0 = (threadIdx.x & (WAVE - 1)) == 0;
    const unsigned long long b_live = __ballot(cls != 0);
    if (b_live) {                                                  // wave-uniform
#pragma unroll
        for (uint32_t k = 1; k <= 4; ++k) {
            const unsigned long long b = __ballot(cls == k);
            if (lane0 && b) atomicAdd(&s_cnt[k], (uint32_t)__popcll(b));
        }
        const unsigned long long b_rm = __ballot(cls == 1 || cls == 3);
        if (lane0) {
            atomicAdd(&s_cnt[0], (uint32_t)__popcll(b_live));
            if (b_rm) {
                const unsigned long long r = (unsigned long long)__popcll(b_rm);
                atomicAdd(&ctr->live, 0ull - r);
                atomicAdd(&ctr->tomb, r);
            }
        }
    }
    if (c != NONE32) atomicMin(lds_first ? &s_first[c] : &first[c], j);
    __syncthreads();
    if (lds_first)
        for (uint32_t k = threadIdx.x; k < nown; k += BLOCK)
            if (s_first[k] != NONE32) atomicMin(&first[k], s_first[k]);
    if (threadIdx.x < 5 && s_cnt[threadIdx.x]) atomicAdd(&cnt->c[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// The owners with a candidate in order of first appearance (a Dictionary that is only added to enumerates in
// insertion order): rank[c] = owner c's place in that order (NONE32: no candidate), owner_out[rank] = its silo.
// One workgroup; nown <= 4096 (the ring's size).
static __global__ void __launch_bounds__(BLOCK) k_cm_order(const uint32_t* __restrict__ first, uint32_t nown,
                                                    const uint32_t* __restrict__ own_silo, uint32_t* __restrict__ rank,
                                                    uint32_t* __restrict__ owner_out, CmCounts* cnt) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < nown; c += BLOCK) {
        const uint32_t f = first[c];
        uint32_t r = NONE32;
        if (f != NONE32) {
            r = 0;
            for (uint32_t o = 0; o < nown; ++o) r += first[o] < f ? 1u : 0u;   // candidates' slots are distinct
            owner_out[r] = own_silo[c];
            atomicAdd(&s_n, 1u);
        }
        rank[c] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) cnt->n_owners = s_n;
}

static __global__ void __launch_bounds__(BLOCK) k_cm_flag(const uint32_t* __restrict__ cand, uint32_t cap,
                                                   uint32_t* __restrict__ flag) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j < cap) flag[j] = cand[j] != NONE32 ? 1u : 0u;
}

// The candidates in enumeration order (pos: inclusive scan of the flags): their owner's rank, their slot.
static __global__ void __launch_bounds__(BLOCK) k_cm_compact(const uint32_t* __restrict__ cand,
                                                      const uint32_t* __restrict__ pos, uint32_t cap,
                                                      const uint32_t* __restrict__ rank, uint32_t* __restrict__ ckey,
                                                      uint32_t* __restrict__ cslot) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= cap) return;
    const uint32_t c = cand[j];
    if (c == NONE32) return;
    const uint32_t k = pos[j] - 1;
    ckey[k] = rank[c];
    cslot[k] = j;
}

// The request lists (perm: the stable bucketing of the candidates by owner rank) and BuildGrainAndETagList's
// generations: list position k takes next_gen + k + 1.  xlen: the KeyExt length (GD_KEYEXT_NULL for a
// three-word key), xsize its bytes.
static __global__ void __launch_bounds__(BLOCK) k_cm_emit(const uint32_t* __restrict__ perm,
                                                   const uint32_t* __restrict__ cslot, uint32_t n, CacheSlot* slots,
                                                   const CacheCounters* ctr, gd_key* __restrict__ okeys,
                                                   int32_t* __restrict__ oetag, uint32_t* __restrict__ oslot,
                                                   int32_t* __restrict__ xlen, uint32_t* __restrict__ xsize) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const uint32_t j = cslot[perm[k]];
    const CacheSlot s = slots[j];
    slots[j].gen = ctr->next_gen + k + 1ull;
    okeys[k] = gd_key{s.n0, s.n1, s.tcd};
    oetag[k] = s.version;
    oslot[k] = j;
    xlen[k] = s.xlen1 ? (int32_t)(s.xlen1 - 1u) : GD_KEYEXT_NULL;
    xsize[k] = s.xlen1 > 1 ? s.xlen1 - 1u : 0u;
}

static __global__ void k_cm_advance(uint32_t n, CacheCounters* ctr) {
    if (threadIdx.x == 0 && blockIdx.x == 0) ctr->next_gen += n;
}

// The candidates' KeyExt strings, compacted (xoff: exclusive scan of xsize).
static __global__ void __launch_bounds__(BLOCK) k_cm_ext_copy(const uint32_t* __restrict__ oslot,
                                                       const uint32_t* __restrict__ xsize,
                                                       const uint32_t* __restrict__ xoff, uint32_t n,
                                                       const CacheSlot* __restrict__ slots,
                                                       const uint8_t* __restrict__ heap, uint8_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n || xsize[k] == 0) return;
    const uint8_t* src = heap + slots[oslot[k]].xoff;
    uint8_t* dst = out + xoff[k];
    for (uint32_t q = 0; q < xsize[k]; ++q) dst[q] = src[q];
}

// gd_cache_entries_age: the three fields in the dump's order (flag / pos as k_cache_dump).
static __global__ void __launch_bounds__(BLOCK) k_cm_dump_age(const CacheSlot* __restrict__ slots,
                                                       const CacheAge* __restrict__ age, uint32_t cap,
                                                       const uint32_t* __restrict__ flag,
                                                       const uint32_t* __restrict__ pos, long long* __restrict__ refreshed,
                                                       long long* __restrict__ timer, int32_t* __restrict__ nacc) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= cap || !flag[j]) return;
    const uint32_t k = pos[j] - 1;
    refreshed[k] = age[j].refreshed;
    timer[k] = age[j].timer;
    nacc[k] = (int32_t)slots[j].nacc;
}

// RemoteGrainDirectory.LookUpMany (RemoteGrainDirectory.cs:65-96), items independent.  cur = GetGrainETag
// (GrainDirectoryPartition.cs:479-491): the slot's VersionTag, -1 without an entry.  The equality test comes
// first, so an unchanged multi-activation entry is SAME.
static __global__ void __launch_bounds__(BLOCK) k_dir_lookup_many(const gd_key* __restrict__ keys,
                                                           const int32_t* __restrict__ etags, uint32_t n,
                                                           TableArgs tab, const uint32_t* __restrict__ vtag,
                                                           uint8_t* __restrict__ out_kind, gd_val* __restrict__ out_vals,
                                                           int32_t* __restrict__ out_tags) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t n0 = keys[i].n0, n1 = keys[i].n1, tcd = keys[i].type_code_data;
    gd_val v{NONE32, NONE32};
    int32_t cur = -1;
    uint8_t kind = GD_LM_ABSENT;
    if (is_keyext_tcd(tcd)) {                       // the KeyExt partition carries no VersionTags: in C#
        kind = GD_LM_HOST;
    } else {
        unsigned long long s = home_slot(uniform_hash(n0, n1, tcd), tab.mask);
        const uint32_t max_probe = tab.ctr->max_probe;
        for (uint32_t p = 0; p <= max_probe; ++p) {
            const Slot sl = tab.slots[s];
            const uint32_t st = slot_state(sl.meta);
            if (st == SLOT_EMPTY) break;
            if (st == SLOT_LIVE && sl.n0 == n0 && sl.n1 == n1 && sl.tcd == tcd) {
                cur = (int32_t)(vtag[s] & 0x7FFFFFFFu);
                if (cur == etags[i]) {
                    kind = GD_LM_SAME;
                } else if (sl.act == GD_ACT_MULTI) {
                    kind = GD_LM_HOST;              // its instance list lives in C#
                    v = gd_val{sl.act, slot_silo(sl.meta)};
                } else {
                    kind = GD_LM_UPDATED;           // an invalid silo: the filtered list is empty, not null (:83-88)
                    if (tab_silo_valid(tab, slot_silo(sl.meta))) v = gd_val{sl.act, slot_silo(sl.meta)};
                }
                break;
            }
            s = (s + 1) & tab.mask;
        }
    }
    out_kind[i] = kind;
    out_vals[i] = v;
    out_tags[i] = cur;
}

// ---- the response without UPDATED items, on the device
// Each SAME / ABSENT item's cached entry; two items on one entry raise cnt->dup (mark: one word a slot, zero
// between calls).  hit[i] = 1 for a SAME item found.
static __global__ void __launch_bounds__(BLOCK) k_cm_find(const gd_key* __restrict__ keys, ExtArgs ext,
                                                   const uint8_t* __restrict__ kind, uint32_t n, CacheArgs cache,
                                                   uint32_t* mark, uint32_t* __restrict__ slot_of,
                                                   uint32_t* __restrict__ hit, CmCounts* cnt) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t slot = NONE32, act, meta;
    const uint8_t k = kind[i];
    bool found = false;
    if (k == GD_LM_SAME || k == GD_LM_ABSENT) found = cache_find_msg(cache, keys, ext, i, slot, act, meta);
    if (found && atomicAdd(&mark[slot], 1u) != 0) atomicOr(&cnt->dup, 1u);
    slot_of[i] = found ? slot : NONE32;
    hit[i] = (found && k == GD_LM_SAME) ? 1u : 0u;
}

// ProcessCacheRefreshResponse (:155-193) for SAME / ABSENT items of distinct keys, which commute: Remove, or
// MarkAsFresh (AdaptiveGrainDirectoryCache.cs:127-136) with the generation next_gen + pos (pos: inclusive scan
// of hit, batch order) and the timer min(max, (long)((double)timer * growth)).  A batch with a duplicate
// changes nothing.  UPDATED items are left to the host form (GD_CR_DEFERRED).
static __global__ void __launch_bounds__(BLOCK) k_cm_apply(const uint8_t* __restrict__ kind,
                                                    const uint32_t* __restrict__ slot_of,
                                                    const uint32_t* __restrict__ pos, uint32_t n, CacheSlot* slots,
                                                    CacheAge* age, CacheCounters* ctr, const CmCounts* cnt,
                                                    uint32_t* mark, long long now, long long max_timer, double growth,
                                                    uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool rm = false;
    if (i < n) {
        const uint32_t slot = slot_of[i];
        const uint8_t k = kind[i];
        uint8_t st = k == GD_LM_UPDATED ? GD_CR_DEFERRED : (k == GD_LM_SAME || k == GD_LM_ABSENT) ? GD_CR_NOT_PRESENT
                                                                                                : GD_CR_SKIPPED;
        if (slot != NONE32) {
            mark[slot] = 0;
            if (!cnt->dup) {
                if (k == GD_LM_ABSENT) {
                    slots[slot].meta = make_meta(SLOT_TOMB, 0);
                    rm = true;
                    st = GD_CR_REMOVED;
                } else {
                    const long long grown = (long long)((double)age[slot].timer * growth);
                    slots[slot].gen = ctr->next_gen + pos[i];
                    age[slot] = CacheAge{now, grown < max_timer ? grown : max_timer};
                    st = GD_CR_FRESHENED;
                }
            }
        }
        if (status) status[i] = st;
    }
    const unsigned long long b = __ballot(rm);
    if ((threadIdx.x & (WAVE - 1)) == 0 && b) {
        const unsigned long long r = (unsigned long long)__popcll(b);
        atomicAdd(&ctr->live, 0ull - r);
        atomicAdd(&ctr->tomb, r);
    }
}

static __global__ void k_cm_apply_advance(const uint32_t* __restrict__ pos, uint32_t n, CacheCounters* ctr,
                                          const CmCounts* cnt) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && n && !cnt->dup) ctr->next_gen += pos[n - 1];
}

}  // namespace gd
