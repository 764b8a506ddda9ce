// gd_frameout.h -- what the stages that write frames into one contiguous output share (the frame encoder,
// gd_encode.h; the response writer, gd_respond.h): the output offsets of a batch in a given order, the capacity
// check, and the constants and the search of the tiled writers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_common.h"

namespace gd {

constexpr uint32_t ERR_ENC_FULL = 128u;      // DevCounters::err: the encoded total exceeds out_cap

// lens[j] = out_len[order[j]] for j < n, lens[n] = 0 (the exclusive scan leaves the total there).  An order entry
// that is no index of the batch is clamped: `order` is required to be a permutation.
static __global__ __launch_bounds__(BLOCK) void k_enc_lens(const uint32_t* __restrict__ out_len,
                                                    const uint32_t* __restrict__ order, uint32_t n,
                                                    uint32_t* __restrict__ lens) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j > n) return;
    lens[j] = j < n ? out_len[order ? min(order[j], n - 1) : j] : 0u;
}

static __global__ __launch_bounds__(BLOCK) void k_enc_finish(const uint32_t* __restrict__ offs, uint32_t n,
                                                      uint64_t out_cap, unsigned long long* __restrict__ out_off,
                                                      uint32_t* __restrict__ err) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j > n) return;
    out_off[j] = offs[j];
    if (j == n && (uint64_t)offs[n] > out_cap) atomicOr(err, ERR_ENC_FULL);
}

constexpr uint32_t ENC_TILE_CHUNKS = 1024;              // 16-B chunks a workgroup: a 16-KiB tile of the output
constexpr uint32_t ENC_TILE_FRAMES = 1024;              // frame offsets kept in LDS (4 KiB + 4); more: global search

struct __attribute__((packed, aligned(4))) EncU4 {
    uint32_t x, y, z, w;
};

// The last j in [lo, hi] with so[j - base] <= pos (so is non-decreasing and so[lo - base] <= pos).
__device__ __forceinline__ uint32_t enc_find(const uint32_t* so, uint32_t base, uint32_t lo, uint32_t hi, uint32_t pos) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (so[mid - base] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace gd
