// gd_rank.h -- row counts and ranks of the bucketing kernels (gd_bucket2.h, gd_msd.h, gd_msd2.h) and of
// the micro-batch sorter (gd_mbsort.h).
#pragma once
#include "gd_scan.h"

namespace gd {

// ---- row counts and ranks of the bucketing kernels (gd_bucket2.h, gd_msd.h, gd_msd2.h) ----------
// A row is one wave instruction's 64 items, each with a digit d; counters are per wave.
//
// The wave's hot digit: the digit most of a row holds, of four candidate lanes' digits (lanes 0, 16,
// 32, 48), when at least 8 of the row's valid lanes hold it; else NONE32.  Uniform over the wave.
// Under Zipf skew (BASELINE cfg 3: one pass-A digit holds 86 % of the messages, one range 62 %) the
// hot digit's items are then counted and ranked in registers by ballot -- no LDS atomic and none of the
// same-address serialisation a hot counter costs (64 lanes on one LDS address take 64 cycles) -- and
// every other item takes its own counter update.  A wave keeps one hot digit for all its rows of a tile.
// One histogram item without a branch: a live item of the wave's hot digit h counts in the register hc,
// any other live item adds 1 to its counter, and an item that is not live (past the tile) or hot adds 1
// to its lane's own sink word (never read; lane-distinct, so no two lanes of one instruction meet there).
// Replaces two nested lane-masked branches an item (their exec-mask juggling was most of the issued
// instructions of the histogram kernels).
__device__ __forceinline__ void hist_add(uint32_t* s_cnt, uint32_t* s_sink, uint32_t d, uint32_t h, bool live,
                                         uint32_t& hc) {
    const bool hot = d == h;
    hc += live && hot ? 1u : 0u;
    atomicAdd(live && !hot ? &s_cnt[d] : &s_sink[threadIdx.x & (WAVE - 1)], 1u);
}

__device__ __forceinline__ uint32_t wave_hot_digit(uint32_t d, bool valid) {
    uint32_t best = NONE32, bc = 7;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t cd = (uint32_t)__builtin_amdgcn_readlane((int)(valid ? d : NONE32), 16 * q);
        const uint32_t c = (uint32_t)__popcll(__ballot(valid && d == cd));
        if (cd != NONE32 && c > bc) {
            bc = c;
            best = cd;
        }
    }
    return best;
}

// This lane's place among the wave's earlier items with its digit d, from the wave's u16 counter at
// bit sh of *p, which this row's valid items then advance.  BALLOT = false: one ds_add_rtn a lane --
// the lanes of one instruction on one address are served in ascending lane order (gd_create
// checks it on the device).  BALLOT = true: stable by construction -- the lanes sharing d found by
// ballots over its B bits (match_digit), the lowest of them adds the group's size, every lane of the
// group takes the base from that lane (ds_bpermute) plus its count of lower peers (GD_OPT_STABLE_RANK
// 0, and the library's choice when gd_create finds the lane order missing).  Call with every lane.
template <bool BALLOT, int B>
__device__ __forceinline__ uint32_t row_rank16(uint32_t* p, uint32_t sh, uint32_t d, bool valid) {
    if constexpr (!BALLOT) {
        uint32_t old = 0;
        if (valid) old = atomicAdd(p, 1u << sh);
        return (old >> sh) & 0xFFFFu;
    } else {
        const unsigned long long peers = match_digit<B>(d, valid);
        const uint32_t lane = lane_id();
        const uint32_t below = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        uint32_t old = 0;
        if (valid && below == 0) old = atomicAdd(p, (uint32_t)__popcll(peers) << sh);
        const int src = peers ? __ffsll((long long)peers) - 1 : (int)lane;
        old = (uint32_t)__shfl((int)old, src, WAVE);
        return ((old >> sh) & 0xFFFFu) + below;
    }
}

// row_rank16 over whole u32 counters.
template <bool BALLOT, int B>
__device__ __forceinline__ uint32_t row_rank32(uint32_t* p, uint32_t d, bool valid) {
    if constexpr (!BALLOT) {
        uint32_t old = 0;
        if (valid) old = atomicAdd(p, 1u);
        return old;
    } else {
        const unsigned long long peers = match_digit<B>(d, valid);
        const uint32_t lane = lane_id();
        const uint32_t below = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        uint32_t old = 0;
        if (valid && below == 0) old = atomicAdd(p, (uint32_t)__popcll(peers));
        const int src = peers ? __ffsll((long long)peers) - 1 : (int)lane;
        old = (uint32_t)__shfl((int)old, src, WAVE);
        return old + below;
    }
}

}  // namespace gd
