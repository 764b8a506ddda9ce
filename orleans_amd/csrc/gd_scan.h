// gd_scan.h -- wave and block scan helpers, the device-wide scan (reduce, then down-sweep) and the fill
// kernel.
#pragma once
#include "gd_hash.h"

namespace gd {

constexpr int SCAN_ITEMS = 4;     // 1024-entry scan tiles: enough blocks to fill the chip
constexpr int SCAN_TILE = BLOCK * SCAN_ITEMS;

// ------------------------------------------------------------------ wave helpers
__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

// Lanes of the wave holding the same BITS-bit digit (match_any by ballots).
template <int BITS>
__device__ __forceinline__ unsigned long long match_digit(uint32_t d, bool valid) {
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(bit);
        peers &= bit ? bal : ~bal;
    }
    return peers;
}

// Wave-wide inclusive sum with DPP (row shifts, then the row broadcasts of lanes 15 and 31): no
// LDS round trips, unlike ds_bpermute shuffles.
__device__ __forceinline__ uint32_t wave_incl_sum_dpp(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);   // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);   // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);   // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);   // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);   // row_bcast:15
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);   // row_bcast:31
    return x;
}

// Wave-wide sum, uniform.
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_sum_dpp(x), WAVE - 1);
}

// Block-wide exclusive add-scan of one value per thread (NTH threads).
template <int NTH>
__device__ __forceinline__ uint32_t block_excl_scan_add_n(uint32_t v, uint32_t* s_wsum) {
    const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, WAVE);
        if (lane >= (uint32_t)off) x += y;
    }
    if (lane == WAVE - 1) s_wsum[w] = x;
    __syncthreads();
    uint32_t wbase = 0;
#pragma unroll
    for (int k = 0; k < NTH / WAVE; ++k)
        if ((uint32_t)k < w) wbase += s_wsum[k];
    __syncthreads();
    return wbase + x - v;
}

// Two block-wide exclusive add-scans (one value each per thread) sharing one pair of barriers.
template <int NTH>
__device__ __forceinline__ void block_excl_scan_add2(uint32_t a, uint32_t b, uint32_t* s_wsum2, uint32_t& ea,
                                                     uint32_t& eb) {
    const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    uint32_t x = a, y = b;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t xa = __shfl_up(x, off, WAVE), yb = __shfl_up(y, off, WAVE);
        if (lane >= (uint32_t)off) {
            x += xa;
            y += yb;
        }
    }
    if (lane == WAVE - 1) {
        s_wsum2[w] = x;
        s_wsum2[NTH / WAVE + w] = y;
    }
    __syncthreads();
    uint32_t wa = 0, wb = 0;
#pragma unroll
    for (int k = 0; k < NTH / WAVE; ++k)
        if ((uint32_t)k < w) {
            wa += s_wsum2[k];
            wb += s_wsum2[NTH / WAVE + k];
        }
    __syncthreads();
    ea = wa + x - a;
    eb = wb + y - b;
}

// p[0..n) = v by the whole grid, at the end of a kernel that has other work: the first pass's
// histogram pre-fills the bucket starts this way (one launch fewer per bucketing).
struct FillArgs {
    uint32_t* p;
    uint32_t n, v;
};
__device__ __forceinline__ void fill_grid(const FillArgs& f, uint32_t nt) {
    if (!f.p) return;
    for (uint32_t i = blockIdx.x * nt + threadIdx.x; i < f.n; i += gridDim.x * nt) f.p[i] = f.v;
}

static __global__ void k_fill_u32(uint32_t* __restrict__ p, uint32_t n, uint32_t v) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ------------------------------------------------------------------ device-wide scan
struct OpAdd {
    static constexpr uint32_t identity = 0u;
    __device__ static uint32_t apply(uint32_t a, uint32_t b) { return a + b; }
};
struct OpMin {
    static constexpr uint32_t identity = 0xFFFFFFFFu;
    __device__ static uint32_t apply(uint32_t a, uint32_t b) { return min(a, b); }
};

template <class Op>
__device__ __forceinline__ uint32_t block_reduce(uint32_t v, uint32_t* s_wsum) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v = Op::apply(v, __shfl_xor(v, off, WAVE));
    if ((threadIdx.x & (WAVE - 1)) == 0) s_wsum[threadIdx.x / WAVE] = v;
    __syncthreads();
    uint32_t r = Op::identity;
#pragma unroll
    for (int k = 0; k < BLOCK / WAVE; ++k) r = Op::apply(r, s_wsum[k]);
    __syncthreads();
    return r;
}

template <class Op>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_wsum) {
    const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, WAVE);
        if (lane >= (uint32_t)off) x = Op::apply(y, x);
    }
    uint32_t ex = __shfl_up(x, 1, WAVE);
    if (lane == 0) ex = Op::identity;
    if (lane == WAVE - 1) s_wsum[w] = x;
    __syncthreads();
    uint32_t wbase = Op::identity;
#pragma unroll
    for (int k = 0; k < BLOCK / WAVE; ++k)
        if ((uint32_t)k < w) wbase = Op::apply(wbase, s_wsum[k]);
    __syncthreads();
    return Op::apply(wbase, ex);
}

// Tiles are physical: block b scans physical tile T = b (forward) or nb - 1 - b (reverse), and
// thread t the IPT entries at T * IPT * BLOCK + IPT * c with c = t (forward) or BLOCK - 1 - t
// (reverse), taken high to low in a reverse scan.  Every thread's entries are then IPT / 4 aligned
// 16-B loads / stores; a reverse scan meets the entries past n (identity) first, which changes
// nothing.  IPT = 4 (1,024-entry tiles: enough blocks to fill the chip) or 16 (4,096-entry tiles,
// for arrays whose 1,024-entry tiles would be too many aggregates to fold in the down-sweep).
static_assert(SCAN_ITEMS == 4, "scan tiles are read as uint4 per thread");

template <int IPT>
__device__ __forceinline__ uint32_t scan_chunk_base(uint32_t n, bool rev) {
    constexpr uint32_t TILE = BLOCK * IPT;
    const uint32_t nb = (n + TILE - 1) / TILE;
    const uint32_t tile = rev ? nb - 1 - blockIdx.x : blockIdx.x;
    const uint32_t c = rev ? BLOCK - 1 - threadIdx.x : threadIdx.x;
    return tile * TILE + IPT * c;
}

// The thread's IPT entries in scan order (identity past n).
template <class Op, int IPT>
__device__ __forceinline__ void scan_load(const uint32_t* in, uint32_t n, bool rev, uint32_t p0, uint32_t (&v)[IPT]) {
    uint32_t x[IPT];
    if (p0 + IPT - 1 < n && (reinterpret_cast<uintptr_t>(in) & 15) == 0) {
#pragma unroll
        for (int q = 0; q < IPT / 4; ++q) {
            const uint4 u = *reinterpret_cast<const uint4*>(in + p0 + 4 * q);
            x[4 * q] = u.x; x[4 * q + 1] = u.y; x[4 * q + 2] = u.z; x[4 * q + 3] = u.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < IPT; ++k) {                 // clamped loads: no per-item branch
            const uint32_t y = in[min(p0 + k, n - 1)];
            x[k] = p0 + k < n ? y : Op::identity;
        }
    }
#pragma unroll
    for (int k = 0; k < IPT; ++k) v[k] = rev ? x[IPT - 1 - k] : x[k];
}

template <class Op, int IPT = SCAN_ITEMS>
static __global__ void __launch_bounds__(BLOCK) k_scan_reduce(const uint32_t* __restrict__ in, uint32_t n, bool rev,
                                                       uint32_t* __restrict__ partials) {
    __shared__ uint32_t s_wsum[BLOCK / WAVE];
    uint32_t v[IPT];
    scan_load<Op, IPT>(in, n, rev, scan_chunk_base<IPT>(n, rev), v);
    uint32_t acc = Op::identity;
#pragma unroll
    for (int k = 0; k < IPT; ++k) acc = Op::apply(acc, v[k]);
    acc = block_reduce<Op>(acc, s_wsum);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// Exclusive scan of `m` partials in one block (sequential over chunks).
template <class Op>
static __global__ void __launch_bounds__(BLOCK) k_scan_partials(uint32_t* partials, uint32_t m) {
    __shared__ uint32_t s_wsum[BLOCK / WAVE];
    __shared__ uint32_t s_carry;
    if (threadIdx.x == 0) s_carry = Op::identity;
    __syncthreads();
    for (uint32_t c = 0; c < m; c += BLOCK) {
        const uint32_t j = c + threadIdx.x;
        const uint32_t v = j < m ? partials[j] : Op::identity;
        const uint32_t ex = block_excl_scan<Op>(v, s_wsum);
        const uint32_t carry = s_carry;
        __syncthreads();
        if (j < m) partials[j] = Op::apply(carry, ex);
        if (threadIdx.x == BLOCK - 1) s_carry = Op::apply(carry, Op::apply(ex, v));
        __syncthreads();
    }
}

template <class Op, int IPT = SCAN_ITEMS>
static __global__ void __launch_bounds__(BLOCK) k_scan_down(const uint32_t* in, uint32_t* out, uint32_t n, bool rev,
                                                     bool inclusive, const uint32_t* __restrict__ partials,
                                                     uint32_t n_partials_raw) {
    __shared__ uint32_t s_wsum[BLOCK / WAVE];
    __shared__ uint32_t s_prefix;
    // n_partials_raw > 0: `partials` holds raw block aggregates; fold those of the
    // preceding blocks here instead of a separate single-block scan launch.
    if (n_partials_raw) {
        uint32_t acc = Op::identity;
        for (uint32_t j = threadIdx.x; j < blockIdx.x; j += BLOCK) acc = Op::apply(acc, partials[j]);
        acc = block_reduce<Op>(acc, s_wsum);
        if (threadIdx.x == 0) s_prefix = acc;
    } else if (threadIdx.x == 0) {
        s_prefix = partials[blockIdx.x];
    }
    __syncthreads();
    const uint32_t prefix = s_prefix;
    const uint32_t p0 = scan_chunk_base<IPT>(n, rev);
    uint32_t v[IPT];
    scan_load<Op, IPT>(in, n, rev, p0, v);
    uint32_t acc = Op::identity;
#pragma unroll
    for (int k = 0; k < IPT; ++k) acc = Op::apply(acc, v[k]);
    uint32_t run = Op::apply(prefix, block_excl_scan<Op>(acc, s_wsum));
    uint32_t r[IPT];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const uint32_t next = Op::apply(run, v[k]);
        r[k] = inclusive ? next : run;
        run = next;
    }
    uint32_t x[IPT];                                    // back to physical order
#pragma unroll
    for (int k = 0; k < IPT; ++k) x[k] = rev ? r[IPT - 1 - k] : r[k];
    if (p0 + IPT - 1 < n && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
#pragma unroll
        for (int q = 0; q < IPT / 4; ++q)
            *reinterpret_cast<uint4*>(out + p0 + 4 * q) = make_uint4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < IPT; ++k)
            if (p0 + k < n) out[p0 + k] = x[k];
    }
}

}  // namespace gd
