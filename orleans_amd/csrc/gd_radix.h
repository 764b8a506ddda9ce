// gd_radix.h -- the LSD radix partition of message indices by activation (ActivationData.cs:566-606
// per-activation FIFO), reduce-then-scan, and the bucket starts' range scan.
#pragma once
#include "gd_scan.h"

namespace gd {

// ------------------------------------------------------------------ K3: stable radix partition
// LSD passes, reduce-then-scan (no in-kernel waiting between workgroups: on
// gfx950 every cross-CU hand-off round-trips through the memory side, which a
// chained look-back pays per step; a kernel boundary costs ~1.5 us once).
// Tile = NT*IT consecutive positions.  Per pass:
//   k_radix_hist    per-tile digit counts, stored digit-major hist[d * tiles + t]
//   scan            one exclusive scan gives every (digit, tile) its global base
//   k_radix_scatter stable rank in the tile (wave-striped order = index order),
//                   stage the tile in LDS in digit order, write each digit run
//                   contiguously.

// Histogram.  Keys are read 16 B per lane (order is irrelevant here).  Equal
// digits within a wave instruction: the lanes sharing the first active lane's
// digit (the hot key under Zipf skew) are folded into one LDS atomic.
template <int BITS, int NT, int IT>
static __global__ void __launch_bounds__(NT) k_radix_hist(const uint32_t* __restrict__ keys, uint32_t n, uint32_t clamp,
                                                   uint32_t shift, uint32_t tiles, uint32_t* __restrict__ hist,
                                                   FillArgs fill) {
    constexpr uint32_t R = 1u << BITS;
    constexpr int NW = NT / WAVE;
    constexpr uint32_t TILE = NT * IT;
    static_assert(IT % 4 == 0, "16-B loads");
    __shared__ uint32_t s_cnt[NW * R];
    for (uint32_t d = threadIdx.x; d < NW * R; d += NT) s_cnt[d] = 0;
    __syncthreads();
    uint32_t* my_cnt = s_cnt + (threadIdx.x / WAVE) * R;
    const uint32_t base = blockIdx.x * TILE;
    const uint32_t lane = lane_id();
    const bool vec = (reinterpret_cast<uintptr_t>(keys) & 15u) == 0 && base + TILE <= n;
    uint32_t k[IT];
#pragma unroll
    for (int j = 0; j < IT / 4; ++j) {
        const uint32_t i0 = base + 4 * (j * NT + threadIdx.x);
        if (vec) {
            const uint4 v = *reinterpret_cast<const uint4*>(keys + i0);
            k[4 * j] = v.x; k[4 * j + 1] = v.y; k[4 * j + 2] = v.z; k[4 * j + 3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) k[4 * j + q] = (i0 + q < n) ? keys[i0 + q] : NONE32;
        }
    }
#pragma unroll
    for (int j = 0; j < IT; ++j) {
        const uint32_t i = base + 4 * ((j / 4) * NT + threadIdx.x) + (j % 4);
        const bool valid = i < n;
        const uint32_t d = (min(k[j], clamp) >> shift) & (R - 1);
        const unsigned long long act = __ballot(valid);
        if (act == 0) continue;
        const uint32_t lead = (uint32_t)__ffsll((long long)act) - 1;
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)lead);
        const unsigned long long hot = __ballot(valid && d == d0);
        if (valid) {
            if (d != d0) atomicAdd(&my_cnt[d], 1u);
            else if (lane == lead) atomicAdd(&my_cnt[d], (uint32_t)__popcll(hot));
        }
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < R; d += NT) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) c += s_cnt[w * R + d];
        hist[d * tiles + blockIdx.x] = c;
    }
    fill_grid(fill, NT);
}

// First tile of a TPB-tile histogram workgroup.  xcd_rev: workgroup b runs on XCD b % 8 (round-robin
// dispatch) and counts tiles from the XCD's range of the scatter's tile order (xcd_tile) in reverse,
// so the tiles the XCD's scatter workgroups read first are the ones its histogram read last -- still
// in that XCD's L2.  Only when the ranges split evenly (tiles a multiple of 8 * TPB).
__device__ __forceinline__ uint32_t hist_t0(uint32_t b, uint32_t nb, uint32_t tpb, uint32_t tiles, uint32_t xcd_rev) {
    if (!xcd_rev || (tiles % (8u * tpb)) != 0 || (nb & 7u) != 0) return b * tpb;
    const uint32_t per = nb >> 3, x = b & 7u, g = b >> 3;
    return (x * per + (per - 1u - g)) * tpb;
}

// Multi-tile histogram: one workgroup counts TPB consecutive tiles, with every tile's 16-B key
// loads issued before the first count, and one counter set per tile shared by the waves.  The
// digit-major counts it writes for one digit are then TPB consecutive words, instead of one word
// every `tiles` words per workgroup.  Same output as k_radix_hist.
template <int BITS, int NT, int IT, int TPB>
static __global__ void __launch_bounds__(NT) k_radix_hist_multi(const uint32_t* __restrict__ keys, uint32_t n,
                                                         uint32_t clamp, uint32_t shift, uint32_t tiles,
                                                         uint32_t* __restrict__ hist, FillArgs fill,
                                                         uint32_t xcd_rev) {
    constexpr uint32_t R = 1u << BITS;
    constexpr uint32_t TILE = NT * IT;
    static_assert(IT % 4 == 0, "16-B loads");
    __shared__ uint32_t s_cnt[TPB][R];
    for (uint32_t x = threadIdx.x; x < TPB * R; x += NT) (&s_cnt[0][0])[x] = 0;
    __syncthreads();
    const uint32_t t0 = hist_t0(blockIdx.x, gridDim.x, TPB, tiles, xcd_rev);
    const uint32_t lane = lane_id();
    const bool aligned = (reinterpret_cast<uintptr_t>(keys) & 15u) == 0;
    uint32_t k[TPB][IT];
    // One workgroup-uniform branch: in a full, aligned range every 16-B load is unconditional, so
    // all TPB * IT / 4 of them are issued before the first wait (a per-tile branch around them
    // makes the compiler wait at each).
    if (aligned && (uint64_t)(t0 + TPB) * TILE <= n) {
#pragma unroll
        for (int t = 0; t < TPB; ++t)
#pragma unroll
            for (int j = 0; j < IT / 4; ++j) {
                const uint64_t i0 = (uint64_t)(t0 + t) * TILE + 4 * (j * NT + threadIdx.x);
                const uint4 v = *reinterpret_cast<const uint4*>(keys + i0);
                k[t][4 * j] = v.x; k[t][4 * j + 1] = v.y; k[t][4 * j + 2] = v.z; k[t][4 * j + 3] = v.w;
            }
    } else {
#pragma unroll
        for (int t = 0; t < TPB; ++t)
#pragma unroll
            for (int j = 0; j < IT / 4; ++j) {
                const uint64_t i0 = (uint64_t)(t0 + t) * TILE + 4 * (j * NT + threadIdx.x);
#pragma unroll
                for (int q = 0; q < 4; ++q) k[t][4 * j + q] = (i0 + q < n) ? keys[i0 + q] : NONE32;
            }
    }
#pragma unroll
    for (int t = 0; t < TPB; ++t) {
        const uint64_t base = (uint64_t)(t0 + t) * TILE;
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const uint64_t i = base + 4 * ((j / 4) * NT + threadIdx.x) + (j % 4);
            const bool valid = i < n;
            const uint32_t d = (min(k[t][j], clamp) >> shift) & (R - 1);
            const unsigned long long act = __ballot(valid);
            if (act == 0) continue;
            const uint32_t lead = (uint32_t)__ffsll((long long)act) - 1;
            const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)lead);
            const unsigned long long hot = __ballot(valid && d == d0);
            if (valid) {
                if (d != d0) atomicAdd(&s_cnt[t][d], 1u);
                else if (lane == lead) atomicAdd(&s_cnt[t][d], (uint32_t)__popcll(hot));
            }
        }
    }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < TPB * R; x += NT) {
        const uint32_t t = x % TPB, d = x / TPB;
        if (t0 + t < tiles) hist[d * tiles + t0 + t] = s_cnt[t][d];
    }
    fill_grid(fill, NT);
}

// Histogram of a packed pass (k_radix_scatter with Pack::in): the key bits above the first pass's
// digit are a u16 array (8 keys per 16-B load), already clamped by the first pass.  TPB tiles per
// workgroup as k_radix_hist_multi (TPB = 1: k_radix_hist's layout).  Same output as those for the
// full keys.
template <int BITS, int NT, int IT, int TPB>
static __global__ void __launch_bounds__(NT) k_radix_hist16(const uint16_t* __restrict__ keys, uint32_t n, uint32_t shift,
                                                     uint32_t tiles, uint32_t* __restrict__ hist, uint32_t xcd_rev) {
    constexpr uint32_t R = 1u << BITS;
    constexpr uint32_t TILE = NT * IT;
    static_assert(IT % 8 == 0, "16-B loads of 8 keys");
    __shared__ uint32_t s_cnt[TPB][R];
    for (uint32_t x = threadIdx.x; x < TPB * R; x += NT) (&s_cnt[0][0])[x] = 0;
    __syncthreads();
    const uint32_t t0 = hist_t0(blockIdx.x, gridDim.x, TPB, tiles, xcd_rev);
    const uint32_t lane = lane_id();
    const bool aligned = (reinterpret_cast<uintptr_t>(keys) & 15u) == 0;
    uint32_t k[TPB][IT];
    if (aligned && (uint64_t)(t0 + TPB) * TILE <= n) {
#pragma unroll
        for (int t = 0; t < TPB; ++t)
#pragma unroll
            for (int j = 0; j < IT / 8; ++j) {
                const uint64_t i0 = (uint64_t)(t0 + t) * TILE + 8 * (j * NT + threadIdx.x);
                const uint4 v = *reinterpret_cast<const uint4*>(keys + i0);
                const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    k[t][8 * j + 2 * q] = u[q] & 0xFFFFu;
                    k[t][8 * j + 2 * q + 1] = u[q] >> 16;
                }
            }
    } else {
#pragma unroll
        for (int t = 0; t < TPB; ++t)
#pragma unroll
            for (int j = 0; j < IT / 8; ++j) {
                const uint64_t i0 = (uint64_t)(t0 + t) * TILE + 8 * (j * NT + threadIdx.x);
#pragma unroll
                for (int q = 0; q < 8; ++q) k[t][8 * j + q] = (i0 + q < n) ? keys[i0 + q] : 0u;
            }
    }
#pragma unroll
    for (int t = 0; t < TPB; ++t) {
        const uint64_t base = (uint64_t)(t0 + t) * TILE;
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const uint64_t i = base + 8 * ((j / 8) * NT + threadIdx.x) + (j % 8);
            const bool valid = i < n;
            const uint32_t d = (k[t][j] >> shift) & (R - 1);
            const unsigned long long act = __ballot(valid);
            if (act == 0) continue;
            const uint32_t lead = (uint32_t)__ffsll((long long)act) - 1;
            const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)lead);
            const unsigned long long hot = __ballot(valid && d == d0);
            if (valid) {
                if (d != d0) atomicAdd(&s_cnt[t][d], 1u);
                else if (lane == lead) atomicAdd(&s_cnt[t][d], (uint32_t)__popcll(hot));
            }
        }
    }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < TPB * R; x += NT) {
        const uint32_t t = x % TPB, d = x / TPB;
        if (t0 + t < tiles) hist[d * tiles + t0 + t] = s_cnt[t][d];
    }
}


// Packed records between radix passes (bucket_device, when the key bits above the first pass's
// digit fit 16 bits and the message index fits beside that digit in 32): A = (key's low b1 bits)
// << ib | index, in the keys array, and B = key >> b1 as u16, in the values array.  6 B a record
// instead of 8, and the later histograms read B alone (2 B).  in: this pass reads packed records;
// out: it writes them (never the last pass, which writes the permutation and the starts).
struct Pack {
    uint32_t ib, b1;
    bool in, out;
};

// Downsweep.  FIRST: values are the message indices themselves.  The keys are
// clamped to `clamp` (unrouted messages -> trailing bucket).
// starts != nullptr (the last pass): the output is fully sorted, so instead of the keys the
// pass writes bucket starts -- the first item of each key in a tile's digit run (the run is
// sorted by the whole key: the lower passes ordered it) lowers starts[key] to its output
// position with atomicMin; the earliest tile holding the key wins (starts pre-filled with n).
template <int BITS, bool FIRST, int NT, int IT>
static __global__ void __launch_bounds__(NT) k_radix_scatter(const uint32_t* __restrict__ keys_in,
                                                      const uint32_t* __restrict__ vals_in, uint32_t n,
                                                      uint32_t clamp, uint32_t shift, uint32_t tiles,
                                                      const uint32_t* __restrict__ gscan,
                                                      uint32_t* __restrict__ keys_out,
                                                      uint32_t* __restrict__ vals_out, uint32_t rank_atomic,
                                                      uint32_t* __restrict__ starts, uint32_t xcd,
                                                      uint32_t* __restrict__ rank_out,
                                                      const uint32_t* __restrict__ totals, Pack pk) {
    constexpr uint32_t R = 1u << BITS;
    constexpr int NW = NT / WAVE;
    constexpr uint32_t TILE = NT * IT;
    __shared__ uint32_t s_wcnt[NW][R];
    __shared__ uint32_t s_lstart[R];
    __shared__ uint32_t s_gbase[R];
    __shared__ uint2 s_kv[TILE];
    __shared__ uint32_t s_wsum[2 * NW];

    const uint32_t tile = xcd_tile(blockIdx.x, gridDim.x, xcd);
    const uint32_t base = tile * TILE;
    const uint32_t cnt_tile = min(TILE, n - base);
    for (uint32_t d = threadIdx.x; d < R; d += NT) {
#pragma unroll
        for (int w = 0; w < NW; ++w) s_wcnt[w][d] = 0;
        s_gbase[d] = gscan[d * tiles + tile];
    }
    const uint32_t lane = lane_id();
    const uint32_t w = threadIdx.x / WAVE;
    const unsigned long long lt = (1ull << lane) - 1ull;
    // thread t owns digits [t*DPT, (t+1)*DPT) in the digit-total scans below
    constexpr uint32_t DPT = (R + NT - 1) / NT;
    uint32_t rk[IT], kk[IT], vv[IT];
    // Branch-free loads (clamped index, masked after): a per-item `if (valid)` around
    // each load makes hipcc wait vmcnt(0) after every one of them.
#pragma unroll
    for (int r = 0; r < IT; ++r) {
        const uint32_t idx = base + (w * IT + r) * WAVE + lane;
        const uint32_t li = min(idx, n - 1);
        kk[r] = __builtin_nontemporal_load(keys_in + li);          // read once: stream past the caches
        if constexpr (!FIRST) {
            if (pk.in) vv[r] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(vals_in) + li);
            else vv[r] = __builtin_nontemporal_load(vals_in + li);
        }
    }
    if constexpr (!FIRST)
        if (pk.in) {                       // (A, B) -> (key, index)
            const uint32_t imask = (1u << pk.ib) - 1u;
#pragma unroll
            for (int r = 0; r < IT; ++r) {
                const uint32_t a = kk[r];
                kk[r] = (vv[r] << pk.b1) | (a >> pk.ib);
                vv[r] = a & imask;
            }
        }
    // totals != nullptr: k_radix_rowscan left gscan per digit row only, and the digit's base (the
    // exclusive prefix of the R row totals) is added below, in the tile-local digit scan; the
    // totals are loaded here, beside the keys
    uint32_t tv[DPT], my_g = 0;
#pragma unroll
    for (uint32_t q = 0; q < DPT; ++q) {
        const uint32_t d = threadIdx.x * DPT + q;
        tv[q] = totals && d < R ? totals[d] : 0u;
        my_g += tv[q];
    }
#pragma unroll
    for (int r = 0; r < IT; ++r) {
        const uint32_t idx = base + (w * IT + r) * WAVE + lane;
        kk[r] = idx < n ? min(kk[r], clamp) : 0u;
        if constexpr (FIRST) vv[r] = idx;
    }
    __syncthreads();
    if (rank_atomic) {
        // One ds_add_rtn per item: lanes of one wave instruction that hit the same counter are
        // served in ascending lane order (checked on gfx950 by tools/ubench_lds_order.hip), and a
        // wave's LDS instructions complete in program order, so the returned count is the stable
        // rank in (row, lane) = index order.
        // The lanes sharing the first valid lane's digit (the hot key under skew) take one
        // counter update by that lane and rank among themselves by ballot; the others use
        // their own ds_add_rtn.  Different digits are different counters, so the two groups
        // do not interact.
        // Issue every row's counter update first (one ds_add_rtn per row: the lead adds the
        // hot group's size, the other non-hot lanes add 1, hot non-lead lanes stay idle), then
        // resolve the hot lanes' ranks: no per-row wait for an LDS result.
        unsigned long long hot[IT];
        uint32_t lead[IT], hd[IT];
#pragma unroll
        for (int r = 0; r < IT; ++r) {
            const uint32_t idx = base + (w * IT + r) * WAVE + lane;
            const bool valid = idx < n;
            const uint32_t d = (kk[r] >> shift) & (R - 1);
            const unsigned long long live = __ballot(valid);
            lead[r] = live ? (uint32_t)__ffsll((long long)live) - 1 : 0u;
            hd[r] = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)lead[r]);
            hot[r] = __ballot(valid && d == hd[r]);
            rk[r] = 0;
            if (valid && (d != hd[r] || lane == lead[r]))
                rk[r] = atomicAdd(&s_wcnt[w][d], lane == lead[r] ? (uint32_t)__popcll(hot[r]) : 1u);
        }
#pragma unroll
        for (int r = 0; r < IT; ++r) {
            const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)rk[r], (int)lead[r]);
            if ((hot[r] >> lane) & 1ull) rk[r] = b0 + (uint32_t)__popcll(hot[r] & lt);
        }
    } else {
#pragma unroll
        for (int r = 0; r < IT; ++r) {
            const uint32_t idx = base + (w * IT + r) * WAVE + lane;
            const bool valid = idx < n;
            const uint32_t d = (kk[r] >> shift) & (R - 1);
            const unsigned long long peers = match_digit<BITS>(d, valid);
            uint32_t c = 0;
            if (valid) c = s_wcnt[w][d];
            rk[r] = c + (uint32_t)__popcll(peers & lt);
            if (valid && (peers & lt) == 0) s_wcnt[w][d] = c + (uint32_t)__popcll(peers);
        }
    }
    __syncthreads();
    // cross-wave exclusive prefix per digit, then tile-local digit starts
    uint32_t my_total = 0;
#pragma unroll
    for (uint32_t q = 0; q < DPT; ++q) {
        const uint32_t d = threadIdx.x * DPT + q;
        if (d < R) {
            uint32_t run = 0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) {
                const uint32_t t = s_wcnt[ww][d];
                s_wcnt[ww][d] = run;
                run += t;
            }
            s_lstart[d] = run;          // digit total for now
            my_total += run;
        }
    }
    uint32_t ex, exg;
    block_excl_scan_add2<NT>(my_total, my_g, s_wsum, ex, exg);     // its barrier orders s_gbase's stores
    {
        // one LDS lookup per item on each side below: the waves' prefixes become absolute tile
        // positions (s_wcnt += the digit's tile start), and the write-out's base is gbase - lstart
        uint32_t run = ex, rung = exg;
#pragma unroll
        for (uint32_t q = 0; q < DPT; ++q) {
            const uint32_t d = threadIdx.x * DPT + q;
            if (d < R) {
                const uint32_t t = s_lstart[d];
#pragma unroll
                for (int ww = 0; ww < NW; ++ww) s_wcnt[ww][d] += run;
                s_gbase[d] = s_gbase[d] + (totals ? rung : 0u) - run;
                run += t;
                rung += tv[q];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < IT; ++r) {
        const uint32_t idx = base + (w * IT + r) * WAVE + lane;
        if (idx < n) {
            const uint32_t d = (kk[r] >> shift) & (R - 1);
            s_kv[s_wcnt[w][d] + rk[r]] = make_uint2(kk[r], vv[r]);
        }
    }
    __syncthreads();
    // the write-out's LDS reads in batches of WB items (every staged record, then every digit base), not
    // one item's two dependent reads and a wait at a time (as k_b2_scatter / k_seg_scatter; past the tile
    // the records are stale LDS, masked to a digit, and nothing is stored)
    constexpr int WB = IT < 8 ? IT : 8;
#pragma unroll
    for (int j0 = 0; j0 < IT; j0 += WB) {
    uint2 kq[WB];
    uint32_t gq[WB];
#pragma unroll
    for (int u = 0; u < WB; ++u) kq[u] = s_kv[(j0 + u) * NT + threadIdx.x];
#pragma unroll
    for (int u = 0; u < WB; ++u) gq[u] = s_gbase[(kq[u].x >> shift) & (R - 1)] + (j0 + u) * NT + threadIdx.x;
#pragma unroll
    for (int u = 0; u < WB; ++u) {
        const uint32_t p = (j0 + u) * NT + threadIdx.x;
        if (p < cnt_tile) {
            const uint2 kv = kq[u];
            const uint32_t g = gq[u];                // s_gbase holds the digit's global base - its tile start
            if (g < n) {            // always true when the scan is right; never write out of bounds
                if (starts) {
                    // a key's first item in the tile: the item before it holds another key (a digit
                    // boundary is a key boundary too)
                    if (p == 0 || s_kv[p - 1].x != kv.x) atomicMin(&starts[kv.x], g);
                    vals_out[g] = kv.y;
                } else if (pk.out) {
                    keys_out[g] = ((kv.x & ((1u << pk.b1) - 1u)) << pk.ib) | kv.y;
                    reinterpret_cast<uint16_t*>(vals_out)[g] = (uint16_t)(kv.x >> pk.b1);
                } else {
                    keys_out[g] = kv.x;
                    vals_out[g] = kv.y;
                }
                if (rank_out) rank_out[kv.y] = g;     // the inverse permutation (last pass, on request)
            }
        }
    }
    }
}

// One workgroup per digit d (the radix pass's counts are digit-major): exclusive add-scan of the
// row hist[d * tiles, (d + 1) * tiles) in place, and the row total into totals[d].  The scatter
// adds the digit's base (the exclusive prefix of the totals) itself, so a pass takes one scan
// launch here instead of a device-wide reduce + down-sweep.
static __global__ void __launch_bounds__(BLOCK) k_radix_rowscan(uint32_t* __restrict__ hist, uint32_t tiles,
                                                         uint32_t* __restrict__ totals) {
    constexpr int IPT = 16;
    constexpr uint32_t CH = BLOCK * IPT;
    __shared__ uint32_t s_wsum[BLOCK / WAVE];
    uint32_t* row = hist + (size_t)blockIdx.x * tiles;
    const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15u) == 0;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < tiles; c0 += CH) {
        const uint32_t p0 = c0 + IPT * threadIdx.x;
        const bool vec = aligned && p0 + IPT <= tiles;
        uint32_t v[IPT];
        if (vec) {
#pragma unroll
            for (int q = 0; q < IPT / 4; ++q) {
                const uint4 u = *reinterpret_cast<const uint4*>(row + p0 + 4 * q);
                v[4 * q] = u.x; v[4 * q + 1] = u.y; v[4 * q + 2] = u.z; v[4 * q + 3] = u.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < IPT; ++k) v[k] = p0 + k < tiles ? row[p0 + k] : 0u;
        }
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < IPT; ++k) acc += v[k];
        uint32_t run = carry + block_excl_scan<OpAdd>(acc, s_wsum);
        uint32_t chunk = 0;
#pragma unroll
        for (int k = 0; k < BLOCK / WAVE; ++k) chunk += s_wsum[k];
        uint32_t r[IPT];
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            r[k] = run;
            run += v[k];
        }
        if (vec) {
#pragma unroll
            for (int q = 0; q < IPT / 4; ++q)
                *reinterpret_cast<uint4*>(row + p0 + 4 * q) = make_uint4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < IPT; ++k)
                if (p0 + k < tiles) row[p0 + k] = r[k];
        }
        carry += chunk;
        __syncthreads();                    // s_wsum is rewritten by the next chunk's scan
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// The bucket starts' reverse inclusive min-scan in one launch, when the last radix pass's digit
// covers at most RS_RANGE * RS_MAX_SUB activations (1 << shift): workgroup d scans the activations
// [d << shift, (d + 1) << shift) of offsets[0, n_scan) alone, RS_RANGE at a time from the top.  Its
// carry -- the first start past the range -- is the last pass's digit base base(d + 1) = the
// number of messages whose (clamped) key lies below the range's end (n when there is none): the
// starts of non-empty activations increase with the activation, and the empty ones hold n.  Each
// lower sub-range then carries the minimum of the ones above it.
constexpr uint32_t RS_THREADS = 1024;
constexpr uint32_t RS_IPT = 16;
constexpr uint32_t RS_RANGE = RS_THREADS * RS_IPT;      // 16,384 activations per sub-range
constexpr uint32_t RS_MAX_SUB = 16;                      // digit ranges up to 2^18 activations
static __global__ void __launch_bounds__(RS_THREADS) k_starts_rangescan(uint32_t* __restrict__ offsets, uint32_t n_scan,
                                                                 uint32_t shift, const uint32_t* __restrict__ totals,
                                                                 uint32_t n_digits) {
    constexpr uint32_t NW = RS_THREADS / WAVE;
    __shared__ uint32_t s_w[2][NW];
    const uint32_t d = blockIdx.x;
    const uint64_t lo64 = (uint64_t)d << shift;
    if (lo64 >= n_scan) return;                          // workgroup-uniform: an empty top range
    const uint32_t lo = (uint32_t)lo64;
    const uint32_t hi = (uint32_t)min<uint64_t>(lo64 + (1ull << shift), n_scan);
    const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    // thread t takes chunk c = RS_THREADS - 1 - t of a sub-range, so a forward exclusive scan over
    // the threads is the minimum over the chunks above c.  The next sub-range's loads go out before
    // the current one is scanned (the top one's before the carry is summed).
    const uint32_t c = RS_THREADS - 1 - threadIdx.x;
    const uint32_t n_sub = (hi - lo + RS_RANGE - 1) / RS_RANGE;
    auto load = [&](uint32_t sub, uint32_t (&v)[RS_IPT]) {
        const uint32_t p0 = lo + sub * RS_RANGE + c * RS_IPT;
        if (p0 + RS_IPT <= hi && (reinterpret_cast<uintptr_t>(offsets + p0) & 15u) == 0) {
#pragma unroll
            for (uint32_t q = 0; q < RS_IPT / 4; ++q) {
                const uint4 u = *reinterpret_cast<const uint4*>(offsets + p0 + 4 * q);
                v[4 * q] = u.x; v[4 * q + 1] = u.y; v[4 * q + 2] = u.z; v[4 * q + 3] = u.w;
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < RS_IPT; ++k) v[k] = p0 + k < hi ? offsets[min(p0 + k, n_scan - 1)] : 0xFFFFFFFFu;
        }
    };
    uint32_t v[RS_IPT], nx[RS_IPT];
    load(n_sub - 1, v);
    // base(d + 1), the carry into the range's top
    uint32_t part = 0;
    for (uint32_t j = threadIdx.x; j <= d && j < n_digits; j += RS_THREADS) part += totals[j];
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) part += __shfl_xor(part, off, WAVE);
    if (lane == 0) s_w[1][w] = part;
    __syncthreads();
    uint32_t carry = 0;
#pragma unroll
    for (uint32_t k = 0; k < NW; ++k) carry += s_w[1][k];
    for (uint32_t sub = n_sub; sub-- > 0;) {
        if (sub > 0) load(sub - 1, nx);
        const uint32_t p0 = lo + sub * RS_RANGE + c * RS_IPT;
        const bool vec = p0 + RS_IPT <= hi && (reinterpret_cast<uintptr_t>(offsets + p0) & 15u) == 0;
        uint32_t m = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t k = 0; k < RS_IPT; ++k) m = min(m, v[k]);
        uint32_t x = m;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const uint32_t y = __shfl_up(x, off, WAVE);
            if (lane >= (uint32_t)off) x = min(x, y);
        }
        uint32_t ex = __shfl_up(x, 1, WAVE);
        if (lane == 0) ex = 0xFFFFFFFFu;
        if (lane == WAVE - 1) s_w[0][w] = x;
        __syncthreads();
        uint32_t wmin = 0xFFFFFFFFu, bmin = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t k = 0; k < NW; ++k) {
            const uint32_t t = s_w[0][k];
            if (k < w) wmin = min(wmin, t);
            bmin = min(bmin, t);
        }
        uint32_t run = min(carry, min(wmin, ex));
#pragma unroll
        for (int k = RS_IPT - 1; k >= 0; --k) {
            run = min(run, v[k]);
            v[k] = run;
        }
        if (vec) {
#pragma unroll
            for (uint32_t q = 0; q < RS_IPT / 4; ++q)
                *reinterpret_cast<uint4*>(offsets + p0 + 4 * q) = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < RS_IPT; ++k)
                if (p0 + k < hi) offsets[p0 + k] = v[k];
        }
        carry = min(carry, bmin);
#pragma unroll
        for (uint32_t k = 0; k < RS_IPT; ++k) v[k] = nx[k];
        __syncthreads();                                 // s_w[0] is rewritten by the next sub-range
    }
}

}  // namespace gd
