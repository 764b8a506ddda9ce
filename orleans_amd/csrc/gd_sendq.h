// gd_sendq.h -- gfx950 device code for the sender-queue partition: the queue rule of
// OutboundMessageQueue.SendMessage (OutboundMessageQueue.cs:54-131) for a batch of addressed messages,
// and the stable partition of the batch over its B = n_queues + 4 buckets:
//   0 loopback (InboundQueue.PostMessage, :90-95), 1 the ping sender, 2 the system sender,
//   3 + q the application sender q = Math.Abs(TargetSilo.GetConsistentHashCode()) % SiloSenderQueues
//   (:125), 3 + n_queues the trailing bucket: everything not queued (held, expired, no / unknown silo,
//   Math.Abs(int.MinValue) throwing), told apart by its send status.
//
// One pass, three kernels and two small scans per batch:
//   k_sendq_classify  reads silo (4 B), route status (1), category (1) and ttl (8) once; writes the send
//                     status (1 B) and the bucket id (4 B); per-tile bucket counts from LDS
//   k_radix_rowscan   (gd_radix.h) each bucket's row of tile counts, and the bucket totals
//   k_sendq_offsets   the totals' exclusive scan: offsets[B + 1]
//   k_sendq_scatter   stable rank of each tile's messages, staged in LDS in bucket order, perm written
//                     run by run.  No second level, no intermediate records.
// The general bucketing (gd_msd.h, gd_bucket2.h) is shaped for 10^4 .. 10^8 activations; at 5 .. 1,028
// buckets its MSD pass sees one range holding the whole batch.
//
// The per-silo table: gd_send_configure turns silo_hash[s] into the silo's application bucket on the
// host (SQ_THROWS for INT32_MIN, whose Math.Abs throws), so the kernel does a table read where the
// reference does an abs and a modulo per message.  The table is staged in LDS when it fits 32 KB
// (n_silos <= 8,192) and read through global memory otherwise.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_common.h"
#include "gd_scan.h"
#include "graindispatch.h"

namespace gd {

constexpr int SQ_NT = 256;
constexpr int SQ_IT = 16;
constexpr uint32_t SQ_TILE = SQ_NT * SQ_IT;       // 4096 messages per tile
constexpr int SQ_NW = SQ_NT / WAVE;
constexpr uint32_t SQ_TAB_LDS_BYTES = 32768;      // the per-silo table is staged in LDS up to this size
constexpr uint32_t SQ_THROWS = 0xFFFFFFFFu;       // table entry of a silo whose hash is INT32_MIN
constexpr uint32_t SQ_MAX_QUEUES = 1024;
constexpr uint32_t SQ_MAX_SILOS = 65536;

struct SendArgs {
    const uint32_t* tab;      // [n_silos]: 3 + abs(hash) % n_queues, or SQ_THROWS
    uint32_t n_silos, n_queues, my_silo;
    uint32_t tab_lds;         // stage tab in LDS
};

// u32 words of k_sendq_classify's / k_sendq_scatter's dynamic LDS
__host__ __device__ __forceinline__ uint32_t sq_pad4(uint32_t x) { return (x + 3u) & ~3u; }
inline size_t sq_classify_lds(uint32_t B, uint32_t n_silos, bool tab_lds) {
    return ((size_t)sq_pad4(B) + (tab_lds ? sq_pad4(n_silos) : 0u)) * 4;
}
inline size_t sq_scatter_lds(uint32_t B) {
    return ((size_t)(SQ_NW + 2) * sq_pad4(B) + 4u * SQ_NW) * 4 + (size_t)SQ_TILE * 4;
}

// The rules of SendMessage in the reference's order; returns the bucket, st = the send status.
__device__ __forceinline__ uint32_t send_bucket(uint32_t silo, uint32_t rs, uint32_t cat, int64_t ttl,
                                                const SendArgs& a, const uint32_t* tab, uint32_t& st) {
    const uint32_t trailing = 3u + a.n_queues;
    if (rs != GD_ROUTE_OK && rs != GD_ROUTE_SYSTEM_TARGET && rs != GD_ROUTE_MEMBERSHIP) {
        st = GD_SEND_HELD;                          // not addressed yet: AddressMessage's slow path
        return trailing;
    }
    if (ttl != GD_TTL_NONE && ttl <= 0) {           // Message.IsExpired (Message.cs:293-302)
        st = GD_SEND_EXPIRED;
        return trailing;
    }
    if (silo == GD_NO_SILO) {                       // :82-87
        st = GD_SEND_NO_SILO;
        return trailing;
    }
    if (silo >= a.n_silos) {
        st = GD_SEND_UNKNOWN_SILO;
        return trailing;
    }
    if (silo == a.my_silo) {                        // :90-95
        st = GD_SEND_LOOPBACK;
        return 0u;
    }
    st = GD_SEND_QUEUED;
    if (cat == 0u) return 1u;                       // Ping (Message.cs:75-80)
    if (cat == 1u) return 2u;                       // System
    const uint32_t t = tab[silo];                   // default: Application and every other byte
    if (t == SQ_THROWS) {
        st = GD_SEND_THROWS;
        return trailing;
    }
    return min(t, trailing - 1u);
}

// Item (w, r, lane) of a tile <-> message base + (w * SQ_IT + r) * 64 + lane (k_sendq_scatter ranks in
// that order).  hist == nullptr: classification only.  Counts are not ranks, so LDS atomics in any
// order do; the lanes sharing the first valid lane's bucket (every lane, with one hot queue) take one
// add by that lane.
static __global__ void __launch_bounds__(SQ_NT) k_sendq_classify(const uint32_t* __restrict__ silo,
                                                          const uint8_t* __restrict__ rs,
                                                          const uint8_t* __restrict__ cat,
                                                          const int64_t* __restrict__ ttl, uint32_t n, SendArgs a,
                                                          uint32_t tiles, uint8_t* __restrict__ st_out,
                                                          uint32_t* __restrict__ q_out,
                                                          uint32_t* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_sq[];
    const uint32_t B = a.n_queues + 4u;
    uint32_t* s_cnt = s_sq;                         // [B]
    uint32_t* s_tab = s_sq + sq_pad4(B);            // [n_silos] when staged
    for (uint32_t d = threadIdx.x; d < B; d += SQ_NT) s_cnt[d] = 0;
    if (a.tab_lds)
        for (uint32_t s = threadIdx.x; s < a.n_silos; s += SQ_NT) s_tab[s] = a.tab[s];
    const uint32_t* tab = a.tab_lds ? s_tab : a.tab;
    const uint32_t base = blockIdx.x * SQ_TILE;
    const uint32_t lane = lane_id(), w = threadIdx.x / WAVE;
    // every load of the thread before the first use (one wait, not one per message)
    uint32_t sv[SQ_IT], rv[SQ_IT], cv[SQ_IT];
    int64_t tv[SQ_IT];
#pragma unroll
    for (int r = 0; r < SQ_IT; ++r) {
        const uint32_t li = min(base + (w * SQ_IT + r) * WAVE + lane, n - 1);
        sv[r] = silo[li];
        rv[r] = rs ? (uint32_t)rs[li] : (uint32_t)GD_ROUTE_OK;
        cv[r] = cat ? (uint32_t)cat[li] : 2u;
        tv[r] = ttl ? ttl[li] : GD_TTL_NONE;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SQ_IT; ++r) {
        const uint32_t i = base + (w * SQ_IT + r) * WAVE + lane;
        const bool valid = i < n;
        uint32_t st = 0, d = 0;
        if (valid) {
            d = send_bucket(sv[r], rv[r], cv[r], tv[r], a, tab, st);
            st_out[i] = (uint8_t)st;
            if (q_out) q_out[i] = d;
        }
        if (hist) {
            const unsigned long long live = __ballot(valid);
            const uint32_t lead = live ? (uint32_t)__ffsll((long long)live) - 1u : 0u;
            const uint32_t hd = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)lead);
            const unsigned long long hot = __ballot(valid && d == hd);
            if (valid) {
                if (d != hd) atomicAdd(&s_cnt[d], 1u);
                else if (lane == lead) atomicAdd(&s_cnt[d], (uint32_t)__popcll(hot));
            }
        }
    }
    if (!hist) return;
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < B; d += SQ_NT) hist[(size_t)d * tiles + blockIdx.x] = s_cnt[d];
}

// offsets[d] = messages in the buckets before d (totals: k_radix_rowscan's row totals); offsets[B] = n.
// One workgroup.
static __global__ void __launch_bounds__(SQ_NT) k_sendq_offsets(const uint32_t* __restrict__ totals, uint32_t B,
                                                         uint32_t n, uint32_t* __restrict__ offsets) {
    __shared__ uint32_t s_wsum[SQ_NW];
    const uint32_t dpt = (B + SQ_NT - 1) / SQ_NT;
    const uint32_t d0 = min(threadIdx.x * dpt, B), d1 = min(d0 + dpt, B);
    uint32_t sum = 0;
    for (uint32_t d = d0; d < d1; ++d) sum += totals[d];
    uint32_t run = block_excl_scan_add_n<SQ_NT>(sum, s_wsum);
    for (uint32_t d = d0; d < d1; ++d) {
        offsets[d] = run;
        run += totals[d];
    }
    if (threadIdx.x == 0) offsets[B] = n;
}

// gscan: the (bucket, tile) counts after k_radix_rowscan (exclusive along each bucket's row); offsets:
// k_sendq_offsets' bucket starts.  rank_atomic: the in-wave stable rank by ds_add_rtn (a wave's
// same-address LDS atomics are served in lane order: gd_create's check, gd_msd.h k_lane_order_check)
// or, 0, by ballot matching over the bucket id's `bits` bits (a handle without lane order).
static __global__ void __launch_bounds__(SQ_NT) k_sendq_scatter(const uint32_t* __restrict__ q_in, uint32_t n,
                                                         uint32_t B, uint32_t bits, uint32_t tiles,
                                                         const uint32_t* __restrict__ gscan,
                                                         const uint32_t* __restrict__ offsets,
                                                         uint32_t* __restrict__ perm, uint32_t rank_atomic) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_sq[];
    const uint32_t Bp = sq_pad4(B);
    uint32_t* s_wcnt = s_sq;                        // [SQ_NW][Bp]
    uint32_t* s_lstart = s_wcnt + SQ_NW * Bp;       // [Bp]
    uint32_t* s_gbase = s_lstart + Bp;              // [Bp]
    uint32_t* s_wsum = s_gbase + Bp;                // [4 * SQ_NW]
    uint16_t* s_src = reinterpret_cast<uint16_t*>(s_wsum + 4 * SQ_NW);   // [SQ_TILE]
    uint16_t* s_dig = s_src + SQ_TILE;              // [SQ_TILE]
    static_assert(SQ_TILE <= 65536 && SQ_MAX_QUEUES + 4 <= 65536, "u16 source slots and bucket ids");

    const uint32_t tile = blockIdx.x;
    const uint32_t base = tile * SQ_TILE;
    const uint32_t cnt_tile = min(SQ_TILE, n - base);
    for (uint32_t d = threadIdx.x; d < B; d += SQ_NT) {
#pragma unroll
        for (int w = 0; w < SQ_NW; ++w) s_wcnt[w * Bp + d] = 0;
        s_gbase[d] = offsets[d] + gscan[(size_t)d * tiles + tile];
    }
    const uint32_t lane = lane_id();
    const uint32_t w = threadIdx.x / WAVE;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t* wc = s_wcnt + w * Bp;
    uint32_t dd[SQ_IT], rk[SQ_IT];
#pragma unroll
    for (int r = 0; r < SQ_IT; ++r)
        dd[r] = min(__builtin_nontemporal_load(q_in + min(base + (w * SQ_IT + r) * WAVE + lane, n - 1)), B - 1u);
    __syncthreads();
    if (rank_atomic) {
        // as k_radix_scatter: the lanes sharing the first valid lane's bucket take one counter update by
        // that lane and rank among themselves by ballot; the others use their own ds_add_rtn
        // (SQ_RG rows' updates issued before their results are used; hot / lead are wave-uniform)
        constexpr int SQ_RG = 4;
#pragma unroll
        for (int r0 = 0; r0 < SQ_IT; r0 += SQ_RG) {
            unsigned long long hot[SQ_RG];
            uint32_t lead[SQ_RG];
#pragma unroll
            for (int u = 0; u < SQ_RG; ++u) {
                const int r = r0 + u;
                const bool valid = base + (w * SQ_IT + r) * WAVE + lane < n;
                const uint32_t d = dd[r];
                const unsigned long long live = __ballot(valid);
                lead[u] = live ? (uint32_t)__ffsll((long long)live) - 1u : 0u;
                const uint32_t hd = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)lead[u]);
                hot[u] = __ballot(valid && d == hd);
                rk[r] = 0;
                if (valid && (d != hd || lane == lead[u]))
                    rk[r] = atomicAdd(&wc[d], lane == lead[u] ? (uint32_t)__popcll(hot[u]) : 1u);
            }
#pragma unroll
            for (int u = 0; u < SQ_RG; ++u) {
                const int r = r0 + u;
                const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)rk[r], (int)lead[u]);
                if ((hot[u] >> lane) & 1ull) rk[r] = b0 + (uint32_t)__popcll(hot[u] & lt);
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < SQ_IT; ++r) {
            const bool valid = base + (w * SQ_IT + r) * WAVE + lane < n;
            const uint32_t d = dd[r];
            unsigned long long peers = __ballot(valid);
            for (uint32_t b = 0; b < bits; ++b) {
                const bool bit = (d >> b) & 1u;
                const unsigned long long bal = __ballot(bit);
                peers &= bit ? bal : ~bal;
            }
            uint32_t c = 0;
            if (valid) c = wc[d];
            rk[r] = c + (uint32_t)__popcll(peers & lt);
            if (valid && (peers & lt) == 0) wc[d] = c + (uint32_t)__popcll(peers);
        }
    }
    __syncthreads();
    // cross-wave exclusive prefix per bucket, then the tile-local bucket starts; thread t owns the
    // buckets [t * dpt, (t + 1) * dpt)
    const uint32_t dpt = (B + SQ_NT - 1) / SQ_NT;
    const uint32_t d0 = min(threadIdx.x * dpt, B), d1 = min(d0 + dpt, B);
    uint32_t my_total = 0;
    for (uint32_t d = d0; d < d1; ++d) {
        uint32_t run = 0;
#pragma unroll
        for (int ww = 0; ww < SQ_NW; ++ww) {
            const uint32_t t = s_wcnt[ww * Bp + d];
            s_wcnt[ww * Bp + d] = run;
            run += t;
        }
        s_lstart[d] = run;                          // the bucket's total for now
        my_total += run;
    }
    uint32_t run = block_excl_scan_add_n<SQ_NT>(my_total, s_wsum);
    for (uint32_t d = d0; d < d1; ++d) {
        const uint32_t t = s_lstart[d];
        s_lstart[d] = run;
        s_gbase[d] -= run;                          // the write-out adds the tile position
        run += t;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SQ_IT; ++r) {
        const uint32_t loc = (w * SQ_IT + r) * WAVE + lane;
        if (base + loc < n) {
            const uint32_t d = dd[r];
            const uint32_t p = s_lstart[d] + wc[d] + rk[r];
            if (p < SQ_TILE) {                      // always true when the counts are right
                s_src[p] = (uint16_t)loc;
                s_dig[p] = (uint16_t)d;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SQ_IT; ++j) {
        const uint32_t p = j * SQ_NT + threadIdx.x;
        if (p < cnt_tile) {
            const uint32_t g = s_gbase[min((uint32_t)s_dig[p], B - 1u)] + p;
            if (g < n) perm[g] = base + s_src[p];   // always true when the scan is right; never write out of bounds
        }
    }
}

}  // namespace gd
