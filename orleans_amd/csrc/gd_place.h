// gd_place.h -- gfx950 device code for the batched placement of unregistered grains: what
// Dispatcher.AddressMessageAsync's slow path (Dispatcher.cs:742-767) does per message, for a whole routed batch:
//   PlacementDirectorsManager.SelectOrAddActivation (PlacementDirectorsManager.cs:79-116) asks the grain
//   class's placement director for a silo, AddSingleActivation registers the address, first wins
//   (GrainDirectoryPartition.cs:304-326), SetTargetPlacement writes it into the message and the message that
//   caused the activation carries IsNewPlacement (Dispatcher.cs:753-767).
//
// The silo, per message strategy:
//   GD_PLACE_NONE   none: the message stays GD_ROUTE_MISS
//   GD_PLACE_HASH   sorted_compatible[(uniform hash & 0x7fffffff) % count] (HashBasedPlacementDirector.cs:11-14);
//                   the compatible silos sorted by SiloAddress.CompareTo on the host (gd_place_configure)
//   GD_PLACE_LOCAL  my_silo when the local silo is active and compatible (PreferLocalPlacementDirector.cs:17-26);
//                   else the reference draws a random silo: here the caller's given silo, or none
//   GD_PLACE_GIVEN  given_silo[i]: RandomPlacementDirector and ActivationCountPlacementDirector.cs:89-122 draw
//                   SafeRandom, so C# chooses and the library applies
// Candidates are the messages the route left GD_ROUTE_MISS whose UniqueKey category is Grain; a Client target
// is never placed (PlacementDirectorsManager.cs:85-93,108-109).  A candidate whose strategy gives no silo, or a
// silo that is out of range, not compatible or not valid (IsValidSilo, GrainDirectoryPartition.cs:310), is
// SKIPPED and stays GD_ROUTE_MISS -- even when a later message of the batch places its grain: its slow path in
// C# then finds the entry.
//
// The batch equals the sequential order: the j-th placing candidate (batch order) proposes act_base + j, and
// the registration keeps the first proposal of each grain, so the numbers handed out are sparse.
//
// One call, after the route:
//   k_place_mark     walks the 1-B route status with 16-B loads; loads the key of each MISS message only;
//                    writes the place status (NONE, SKIPPED or the provisional PL_PENDING) and the tile's
//                    count of placing candidates (by ballots, no per-item atomics)
//   scan_device      exclusive scan of the tile counts; its total m is the call's read-back
//   k_place_gather   stable compaction: candidate j -> idx[j], keys[j], {act_base + j, silo}.  The silo is
//                    derived again from the key the gather loads anyway, so the mark writes no n-sized
//                    array of silos
//   register_core    the directory batch (gd_dirbatch.h), unchanged: winners and `inserted` per candidate
//   k_place_apply    scatters the winning address and GD_ROUTE_OK to message idx[j], NEW or JOINED by
//                    inserted[j]; counts each block's NEW messages
//   scan_device, k_place_new   the ordered list new_idx[0..n_new) of the messages that created an entry
// Ranks come from ballots and prefix popcounts only, so they hold with and without the LDS lane order.
//
// The tables: the sorted compatible list and the compatible / valid bitsets are staged in LDS by the mark
// when the silo table has at most PL_TAB_LDS_SILOS entries (34 KB at most), read through global memory
// otherwise; the gather touches them once per candidate and reads them through global memory.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_common.h"
#include "gd_scan.h"
#include "graindispatch.h"

namespace gd {

constexpr int PL_NT = 256;
constexpr int PL_IT = 16;                           // messages a thread: one 16-B load of status bytes
constexpr uint32_t PL_TILE = PL_NT * PL_IT;         // 4096 messages per tile
constexpr int PL_NW = PL_NT / WAVE;
constexpr uint32_t PL_TAB_LDS_SILOS = 8192;         // the tables are staged in LDS up to this many silos
constexpr uint32_t PL_MAX_SILOS = 0xFFFEu;          // a directory value's silo index (gd_dir_register)
constexpr uint32_t PL_PENDING = 4;                  // place status between the mark and the apply
constexpr uint32_t PL_CNT_BITS = 5;                 // a thread's count of candidates: 0 .. PL_IT

struct PlaceArgs {
    const uint32_t* sorted;   // [n_comp] compatible silo indices in SiloAddress.CompareTo order
    const uint32_t* compat;   // bitset over silo indices [0, n_silos)
    const uint32_t* valid;    // IsValidSilo bitset over [0, n_valid) (gd_dir_set_valid_silos)
    uint32_t n_silos, n_comp, n_valid, my_silo;
    uint32_t local_ok;        // the local silo is active, in the table and compatible
    uint32_t tab_lds;         // k_place_mark stages the tables in LDS
};

__host__ __device__ __forceinline__ uint32_t pl_words(uint32_t bits) { return (bits + 31u) >> 5; }
// valid bits staged: a chosen silo is below n_silos, so the bits past it are never read
__host__ __device__ __forceinline__ uint32_t pl_valid_words(const PlaceArgs& a) {
    return pl_words(a.n_valid < a.n_silos ? a.n_valid : a.n_silos);
}
inline size_t pl_mark_lds(const PlaceArgs& a) {
    return a.tab_lds ? ((size_t)a.n_comp + pl_words(a.n_silos) + pl_valid_words(a)) * 4 : 0;
}

// One MISS message: 0 not a candidate (place status NONE), 1 skipped, 2 places on `silo`.
__device__ __forceinline__ uint32_t place_choose(uint64_t n0, uint64_t n1, uint64_t tcd, uint32_t strat,
                                                 const uint32_t* __restrict__ given, uint32_t i, const PlaceArgs& a,
                                                 const uint32_t* sorted, const uint32_t* compat,
                                                 const uint32_t* valid, uint32_t& silo) {
    if ((uint32_t)(tcd >> 56) != CAT_GRAIN) return 0u;   // PlacementDirectorsManager.cs:85-93,108-109
    if (a.n_comp == 0) return 1u;                        // no compatible silo
    uint32_t s = GD_NO_SILO;
    if (strat == GD_PLACE_HASH) {                        // HashBasedPlacementDirector.cs:11-14
        s = sorted[(uniform_hash(n0, n1, tcd) & 0x7fffffffu) % a.n_comp];
    } else if (strat == GD_PLACE_LOCAL) {                // PreferLocalPlacementDirector.cs:17-26
        if (a.local_ok) s = a.my_silo;
        else if (given) s = given[i];                    // the reference's random fallback, drawn in C#
    } else if (strat == GD_PLACE_GIVEN) {                // RandomPlacementDirector, ActivationCountPlacementDirector
        if (given) s = given[i];
    }
    if (s >= a.n_silos) return 1u;                       // GD_PLACE_NONE, no given silo, or out of range
    if (!((compat[s >> 5] >> (s & 31u)) & 1u)) return 1u;
    if (!valid_silo(valid, a.n_valid, s)) return 1u;     // IsValidSilo, GrainDirectoryPartition.cs:310
    silo = s;
    return 2u;
}

// A thread's 16 bytes at p[i0 .. i0 + 16) as four words (byte r of the run = message i0 + r); bytes at or
// past n read as `fill`.  wide: p is 16-B aligned.
__device__ __forceinline__ void pl_load16(const uint8_t* __restrict__ p, uint32_t i0, uint32_t n, bool wide,
                                          uint32_t fill, uint32_t (&w)[4]) {
    if (wide && i0 + PL_IT <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(p + i0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        w[q] = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t i = i0 + q * 4 + b;
            w[q] |= (i < n ? (uint32_t)p[i] : fill) << (8 * b);
        }
    }
}

// Bit r set: byte r of the 16 equals v.
__device__ __forceinline__ uint32_t pl_eq_mask(const uint32_t (&w)[4], uint32_t v) {
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < PL_IT; ++r) m |= (((w[r >> 2] >> (8 * (r & 3))) & 0xFFu) == v ? 1u : 0u) << r;
    return m;
}

// Wave-wide sum and exclusive lane prefix of a small count (c <= PL_IT) by one ballot a bit.
__device__ __forceinline__ uint32_t pl_wave_prefix(uint32_t c, uint32_t lane, uint32_t& total) {
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t pre = 0;
    total = 0;
#pragma unroll
    for (uint32_t b = 0; b < PL_CNT_BITS; ++b) {
        const unsigned long long bal = __ballot((c >> b) & 1u);
        pre += (uint32_t)__popcll(bal & lt) << b;
        total += (uint32_t)__popcll(bal) << b;
    }
    return pre;
}
static_assert(PL_IT < (1 << PL_CNT_BITS), "a thread's candidate count fits PL_CNT_BITS bits");

// Thread t of tile b holds messages b * PL_TILE + t * PL_IT + 0 .. 15, so (tile, wave, lane, byte) order is
// batch order.  tile_cnt[tiles] = 0: the scan's total lands there.
static __global__ void __launch_bounds__(PL_NT) k_place_mark(const uint8_t* __restrict__ status,
                                                      const gd_key* __restrict__ keys,
                                                      const uint8_t* __restrict__ strategy, uint32_t default_strategy,
                                                      const uint32_t* __restrict__ given, uint32_t n, PlaceArgs a,
                                                      uint32_t tiles, uint32_t wide, uint8_t* __restrict__ placed,
                                                      uint32_t* __restrict__ tile_cnt) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_pl[];
    __shared__ uint32_t s_wcnt[PL_NW];
    const uint32_t *sorted = a.sorted, *compat = a.compat, *valid = a.valid;
    if (a.tab_lds) {
        const uint32_t cw = pl_words(a.n_silos), vw = pl_valid_words(a);
        uint32_t* s_sorted = s_pl;                      // [n_comp]
        uint32_t* s_compat = s_sorted + a.n_comp;       // [cw]
        uint32_t* s_valid = s_compat + cw;              // [vw]
        for (uint32_t k = threadIdx.x; k < a.n_comp; k += PL_NT) s_sorted[k] = a.sorted[k];
        for (uint32_t k = threadIdx.x; k < cw; k += PL_NT) s_compat[k] = a.compat[k];
        for (uint32_t k = threadIdx.x; k < vw; k += PL_NT) s_valid[k] = a.valid[k];
        sorted = s_sorted;
        compat = s_compat;
        valid = s_valid;
    }
    const uint32_t i0 = blockIdx.x * PL_TILE + threadIdx.x * PL_IT;
    uint32_t sw[4];
    pl_load16(status, i0, n, wide != 0, (uint32_t)GD_ROUTE_OK, sw);
    __syncthreads();
    uint32_t pw[4] = {0, 0, 0, 0};                      // GD_PLACED_NONE
    uint32_t cnt = 0;
    for (uint32_t m = pl_eq_mask(sw, GD_ROUTE_MISS); m; m &= m - 1u) {
        const uint32_t r = (uint32_t)__ffs((int)m) - 1u, i = i0 + r;
        const gd_key k = keys[i];
        uint32_t silo;
        const uint32_t c = place_choose(k.n0, k.n1, k.type_code_data, strategy ? (uint32_t)strategy[i] : default_strategy,
                                        given, i, a, sorted, compat, valid, silo);
        const uint32_t ps = c == 2u ? PL_PENDING : (c == 1u ? (uint32_t)GD_PLACED_SKIPPED : (uint32_t)GD_PLACED_NONE);
        pw[r >> 2] |= ps << (8 * (r & 3u));
        cnt += c == 2u ? 1u : 0u;
    }
    if (wide && i0 + PL_IT <= n) {
        *reinterpret_cast<uint4*>(placed + i0) = make_uint4(pw[0], pw[1], pw[2], pw[3]);
    } else {
        for (uint32_t r = 0; r < (uint32_t)PL_IT && i0 + r < n; ++r)
            placed[i0 + r] = (uint8_t)(pw[r >> 2] >> (8 * (r & 3u)));
    }
    uint32_t total;
    (void)pl_wave_prefix(cnt, lane_id(), total);
    if (lane_id() == 0) s_wcnt[threadIdx.x / WAVE] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < PL_NW; ++w) t += s_wcnt[w];
        tile_cnt[blockIdx.x] = t;
        if (blockIdx.x == 0) tile_cnt[tiles] = 0;
    }
}

// tile_off: the exclusive scan of k_place_mark's counts (tile_off[tiles] = m).  A tile without candidates
// ends after two loads.
static __global__ void __launch_bounds__(PL_NT) k_place_gather(const uint8_t* __restrict__ placed,
                                                        const gd_key* __restrict__ keys,
                                                        const uint8_t* __restrict__ strategy,
                                                        uint32_t default_strategy, const uint32_t* __restrict__ given,
                                                        uint32_t n, PlaceArgs a, uint32_t wide,
                                                        const uint32_t* __restrict__ tile_off, uint32_t act_base,
                                                        uint32_t m, uint32_t* __restrict__ idx,
                                                        gd_key* __restrict__ out_keys, gd_val* __restrict__ out_vals) {
    __shared__ uint32_t s_wcnt[PL_NW];
    const uint32_t tile_base = tile_off[blockIdx.x];
    if (tile_off[blockIdx.x + 1] == tile_base) return;  // the whole workgroup
    const uint32_t i0 = blockIdx.x * PL_TILE + threadIdx.x * PL_IT;
    uint32_t pw[4];
    pl_load16(placed, i0, n, wide != 0, (uint32_t)GD_PLACED_NONE, pw);
    uint32_t pend = pl_eq_mask(pw, PL_PENDING);
    const uint32_t lane = lane_id(), w = threadIdx.x / WAVE;
    uint32_t total;
    const uint32_t pre = pl_wave_prefix((uint32_t)__popc(pend), lane, total);
    if (lane == 0) s_wcnt[w] = total;
    __syncthreads();
    uint32_t j = tile_base + pre;
#pragma unroll
    for (int k = 0; k < PL_NW; ++k)
        if ((uint32_t)k < w) j += s_wcnt[k];
    for (; pend; pend &= pend - 1u, ++j) {
        const uint32_t i = i0 + ((uint32_t)__ffs((int)pend) - 1u);
        const gd_key k = keys[i];
        uint32_t silo = GD_NO_SILO;
        (void)place_choose(k.n0, k.n1, k.type_code_data, strategy ? (uint32_t)strategy[i] : default_strategy, given, i,
                           a, a.sorted, a.compat, a.valid, silo);
        if (j < m) {                                    // always true when the scan is right
            idx[j] = i;
            out_keys[j] = k;
            out_vals[j] = gd_val{act_base + j, silo};
        }
    }
}

// Candidate j -> message idx[j]: the winning address (register_core's report) and GD_ROUTE_OK; NEW when this
// candidate created the entry, else JOINED.  A candidate the registration refused (none, after the mark's
// checks) stays GD_ROUTE_MISS, SKIPPED.  blk_cnt[b] = NEW messages of block b, blk_cnt[blocks] = 0.
static __global__ void __launch_bounds__(PL_NT) k_place_apply(const uint32_t* __restrict__ idx,
                                                       const gd_val* __restrict__ win,
                                                       const uint8_t* __restrict__ inserted, uint32_t m, uint32_t n,
                                                       uint32_t* __restrict__ silo, uint32_t* __restrict__ act,
                                                       uint8_t* __restrict__ status, uint8_t* __restrict__ placed,
                                                       uint32_t* __restrict__ blk_cnt, uint32_t blocks) {
    __shared__ uint32_t s_wcnt[PL_NW];
    const uint32_t j = blockIdx.x * PL_NT + threadIdx.x;
    bool is_new = false;
    if (j < m) {
        const uint32_t i = idx[j];
        const gd_val v = win[j];
        if (i < n) {
            if (v.act == NONE32) {
                placed[i] = (uint8_t)GD_PLACED_SKIPPED;
            } else {
                is_new = inserted[j] != 0;
                silo[i] = v.silo;
                act[i] = v.act;
                status[i] = (uint8_t)GD_ROUTE_OK;
                placed[i] = (uint8_t)(is_new ? GD_PLACED_NEW : GD_PLACED_JOINED);
            }
        }
    }
    const unsigned long long bal = __ballot(is_new);
    if (lane_id() == 0) s_wcnt[threadIdx.x / WAVE] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < PL_NW; ++w) t += s_wcnt[w];
        blk_cnt[blockIdx.x] = t;
        if (blockIdx.x == 0) blk_cnt[blocks] = 0;
    }
}

// new_idx[0 .. n_new): the messages that created an entry, in batch order (idx ascends with j).  blk_off: the
// exclusive scan of k_place_apply's counts; cap: new_idx's entries.
static __global__ void __launch_bounds__(PL_NT) k_place_new(const uint32_t* __restrict__ idx,
                                                     const gd_val* __restrict__ win,
                                                     const uint8_t* __restrict__ inserted, uint32_t m,
                                                     const uint32_t* __restrict__ blk_off,
                                                     uint32_t* __restrict__ new_idx, uint32_t cap) {
    __shared__ uint32_t s_wcnt[PL_NW];
    const uint32_t j = blockIdx.x * PL_NT + threadIdx.x;
    const bool is_new = j < m && inserted[j] != 0 && win[j].act != NONE32;
    const uint32_t lane = lane_id(), w = threadIdx.x / WAVE;
    const unsigned long long bal = __ballot(is_new);
    if (lane == 0) s_wcnt[w] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t r = blk_off[blockIdx.x] + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
    for (int k = 0; k < PL_NW; ++k)
        if ((uint32_t)k < w) r += s_wcnt[k];
    if (is_new && r < cap) new_idx[r] = idx[j];
}

}  // namespace gd
