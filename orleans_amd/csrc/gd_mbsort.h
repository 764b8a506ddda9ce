// gd_mbsort.h -- the micro-batch sorter: one workgroup sorts a whole micro-batch and compacts its runs.
#pragma once
#include "gd_rank.h"

namespace gd {

// ------------------------------------------------------------------ micro-batch bucketing (f3)
// One workgroup sorts the whole micro-batch: LSD radix passes of BITS-bit digits (up to 11, so
// 2^20..2^22 activations take 2 passes) of min(act, n_act), each pass ranking stably inside the
// block and exchanging the (key, index) pairs through LDS.  Item (w, r, lane) <-> position
// (w * IT + r) * 64 + lane; IT = 4 for batches up to 4,096 messages (all 16 waves busy), 8 above.
// Ranking: per row, the wave-ballot ranking of k_radix_scatter into per-(digit, wave) counters
// kept as packed u16 pairs in digit-major order, so ONE block-wide exclusive scan of the counters
// gives every (digit, wave) its output base (the digits' starts and the waves' offsets at once).
// Then the runs of equal keys are compacted with ballots.  For micro-batches this replaces the
// multi-launch radix pipeline and the O(n_act) offsets: the host gets perm[n] and, per activation
// present, run_act[r] / run_start[r] (run_start[n_runs] = n), each run in arrival order
// (ActivationData.cs:566-606).
constexpr int MB_THREADS = 1024;
constexpr int MB_NW = MB_THREADS / WAVE;
constexpr uint32_t MB_MAX = MB_THREADS * 8;        // 8192 messages
constexpr int MB_MAX_BITS = 11;

struct MbShared {
    uint32_t cnt[(1u << MB_MAX_BITS) * MB_NW / 2];  // u16 (digit, wave) counters, digit-major, 2 per word
    uint2 kv[MB_MAX];
    uint32_t wsum[MB_NW];
};

// Block-wide exclusive sum over MB_THREADS threads (two barriers).
__device__ __forceinline__ uint32_t mb_block_excl_sum(uint32_t v, uint32_t* s_wsum) {
    const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const uint32_t x = wave_incl_sum_dpp(v);
    if (lane == WAVE - 1) s_wsum[w] = x;
    __syncthreads();
    const uint32_t ws = lane < (uint32_t)MB_NW ? s_wsum[lane] : 0u;
    const uint32_t wi = wave_incl_sum_dpp(lane < w ? ws : 0u);   // sum of the waves before w
    const uint32_t wbase = (uint32_t)__builtin_amdgcn_readlane((int)wi, WAVE - 1);
    __syncthreads();
    return wbase + x - v;
}

// The sort + runs over keys kk (already clamped to n_act) and indices vv held in registers.
// Outputs are written for positions in [lo, hi) only (the calling workgroup's share; n_runs and
// run_start[n_runs] by the share holding n).
template <int BITS, int IT>
__device__ __forceinline__ void mb_sort_runs_core(MbShared& sh, uint32_t (&kk)[IT], uint32_t (&vv)[IT], uint32_t n,
                                                  uint32_t passes, uint32_t* __restrict__ perm,
                                                  uint32_t* __restrict__ run_act, uint32_t* __restrict__ run_start,
                                                  uint32_t* __restrict__ n_runs, uint32_t lo, uint32_t hi,
                                                  unsigned long long* ts, bool ballot) {
    constexpr uint32_t R = 1u << BITS;
    constexpr uint32_t WORDS = R * MB_NW / 2;
    constexpr uint32_t WPT = WORDS >= MB_THREADS ? WORDS / MB_THREADS : 1;   // counter words per thread
    constexpr uint32_t COLS = WORDS / WPT;
    // scan word q (q = thread * WPT + j) lives at word (q % WPT) * COLS + q / WPT: the scan's reads
    // are unit-stride across lanes, the ranking atomics spread over the banks by digit
    auto cw = [](uint32_t q) { return (q % WPT) * COLS + q / WPT; };
    static_assert(BITS <= MB_MAX_BITS && IT * MB_THREADS <= (int)MB_MAX, "micro-batch shape");
    uint32_t* s_cnt = sh.cnt;
    uint2* s_kv = sh.kv;
    uint32_t* s_wsum = sh.wsum;
    const uint32_t lane = lane_id(), w = threadIdx.x / WAVE;
    const unsigned long long lt = (1ull << lane) - 1ull;
    unsigned long long t = 0;
    mb_mark(ts, 0, t);
    const unsigned long long c0 = ts ? clock64() : 0, r0 = t;
    for (uint32_t e = threadIdx.x * 4; e < WORDS; e += MB_THREADS * 4)
        *reinterpret_cast<uint4*>(s_cnt + e) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const uint32_t shift = pass * BITS;
        // Stable in-wave rank: the wave's hot digit by ballot in registers, the others by row_rank16
        // (ds_add_rtn in lane order, or ballots when `ballot`: GD_OPT_STABLE_RANK 0).  Rows past n are
        // skipped wave-uniformly.
        uint32_t rk[IT];
        const uint32_t h = wave_hot_digit(kk[0] >> shift & (R - 1), (uint32_t)(w * IT) * WAVE + lane < n);
        uint32_t hrun = 0;
#pragma unroll
        for (int r = 0; r < IT; ++r) {
            rk[r] = 0;
            if ((uint32_t)(w * IT + r) * WAVE >= n) continue;
            const bool valid = (w * IT + r) * WAVE + lane < n;
            const uint32_t d = (kk[r] >> shift) & (R - 1);
            const uint32_t e = d * MB_NW + w, sh16 = (e & 1u) * 16u;
            const unsigned long long hm = __ballot(valid && d == h);
            const bool cold = valid && d != h;
            const uint32_t cr = ballot ? row_rank16<true, BITS>(&s_cnt[cw(e >> 1)], sh16, d, cold)
                                       : row_rank16<false, BITS>(&s_cnt[cw(e >> 1)], sh16, d, cold);
            rk[r] = d == h ? hrun + (uint32_t)__popcll(hm & lt) : cr;
            hrun += (uint32_t)__popcll(hm);
        }
        if (lane == 0 && hrun) {
            const uint32_t e = h * MB_NW + w;
            atomicAdd(&s_cnt[cw(e >> 1)], hrun << ((e & 1u) * 16u));
        }
        __syncthreads();
        if (pass == 0) mb_mark(ts, 4, t);
        // exclusive scan of the counters in (digit, wave) order: base of every (digit, wave)
        {
            const bool mine = threadIdx.x < COLS;
            uint32_t cv[WPT];
            uint32_t sum = 0;
#pragma unroll
            for (uint32_t j = 0; j < WPT; ++j) {
                cv[j] = mine ? s_cnt[j * COLS + threadIdx.x] : 0u;
                sum += (cv[j] & 0xFFFFu) + (cv[j] >> 16);
            }
            uint32_t run = mb_block_excl_sum(sum, s_wsum);
            if (mine) {
#pragma unroll
                for (uint32_t j = 0; j < WPT; ++j) {
                    const uint32_t a = run;
                    run += cv[j] & 0xFFFFu;
                    s_cnt[j * COLS + threadIdx.x] = a | (run << 16);
                    run += cv[j] >> 16;
                }
            }
        }
        __syncthreads();
        if (pass == 0) mb_mark(ts, 14, t);
#pragma unroll
        for (int r = 0; r < IT; ++r) {
            if ((w * IT + r) * WAVE + lane < n) {
                const uint32_t d = (kk[r] >> shift) & (R - 1);
                const uint32_t e = d * MB_NW + w;
                const uint32_t base = (s_cnt[cw(e >> 1)] >> ((e & 1u) * 16u)) & 0xFFFFu;
                s_kv[base + rk[r]] = make_uint2(kk[r], vv[r]);
            }
        }
        __syncthreads();
        if (pass == 0) mb_mark(ts, 15, t);
#pragma unroll
        for (int r = 0; r < IT; ++r) {
            const uint32_t p = (w * IT + r) * WAVE + lane;
            if (p < n) {
                const uint2 kv = s_kv[p];
                kk[r] = kv.x;
                vv[r] = kv.y;
            }
        }
        if (pass + 1 < passes)       // the counters are free again: clear them for the next pass
            for (uint32_t e = threadIdx.x * 4; e < WORDS; e += MB_THREADS * 4)
                *reinterpret_cast<uint4*>(s_cnt + e) = make_uint4(0, 0, 0, 0);
        __syncthreads();
        mb_mark(ts, 5 + (int)pass, t);
    }
    // runs: a head where the key changes; wave w owns positions [w * IT * 64, (w + 1) * IT * 64)
    // in (r, lane) order, so heads are counted per wave, scanned across waves, ranked in-wave.
    uint32_t prev[IT];
#pragma unroll
    for (int r = 0; r < IT; ++r) {
        const uint32_t p = (w * IT + r) * WAVE + lane;
        // key of position p - 1: lane - 1 of the same row, lane 63 of the previous row, or the
        // previous wave's last item (read through LDS, which still holds the sorted pairs)
        const uint32_t up = __shfl_up(kk[r], 1, WAVE);
        uint32_t pk = up;
        if (lane == 0) pk = (p > 0 && p - 1 < n) ? s_kv[p - 1].x : ~0u;
        prev[r] = pk;
    }
    uint32_t heads_w = 0;
    unsigned long long hb[IT];
#pragma unroll
    for (int r = 0; r < IT; ++r) {
        const uint32_t p = (w * IT + r) * WAVE + lane;
        hb[r] = __ballot(p < n && (p == 0 || prev[r] != kk[r]));
        heads_w += (uint32_t)__popcll(hb[r]);
    }
    const uint32_t wbase = mb_block_excl_sum(lane == 0 ? heads_w : 0u, s_wsum);
    mb_mark(ts, 9, t);
    const uint32_t base = __shfl(wbase, 0, WAVE);
    uint32_t before = base;
#pragma unroll
    for (int r = 0; r < IT; ++r) {
        const uint32_t p = (w * IT + r) * WAVE + lane;
        if (p < n && p >= lo && p < hi) {
            perm[p] = vv[r];
            if ((hb[r] >> lane) & 1ull) {
                const uint32_t q = before + (uint32_t)__popcll(hb[r] & lt);
                run_act[q] = kk[r];
                run_start[q] = p;
            }
        }
        before += (uint32_t)__popcll(hb[r]);
    }
    if (threadIdx.x == MB_THREADS - 1 && n >= lo && n < hi) {
        const uint32_t tot = base + heads_w;   // last wave's base + its heads = all runs
        n_runs[0] = tot;
        run_start[tot] = n;
    }
    mb_mark(ts, 10, t);
    if (ts) {
        __threadfence_system();
        mb_mark(ts, 11, t);
        if (blockIdx.x == 0 && threadIdx.x == 0) {     // shader clocks vs wall ticks over the kernel
            atomicAdd(ts + 12, clock64() - c0);
            atomicAdd(ts + 13, t - r0);
        }
    }
}

// gridDim.x workgroups sort the same batch redundantly and each writes its 1/gridDim.x share of
// the outputs: zero-copy stores to host memory are spread over as many CUs.  act_copy (optional):
// the activations also go to the host block.  done (optional, pinned host memory): each workgroup adds
// 1 once its share is stored and fenced, so the host sees the batch finished without waiting for the
// dispatch's completion signal (gd_microbatch_run's poll).
template <int BITS, int IT>
static __global__ void __launch_bounds__(MB_THREADS) k_mb_sort_runs(const uint32_t* __restrict__ act, uint32_t n,
                                                              uint32_t passes, uint32_t n_act,
                                                              uint32_t* __restrict__ perm,
                                                              uint32_t* __restrict__ run_act,
                                                              uint32_t* __restrict__ run_start,
                                                              uint32_t* __restrict__ n_runs,
                                                              uint32_t* __restrict__ act_copy,
                                                              unsigned long long* ts, uint32_t ballot,
                                                              uint32_t* done) {
    __shared__ MbShared sh;
    const uint32_t lane = lane_id(), w = threadIdx.x / WAVE;
    const uint32_t lo = (uint32_t)((uint64_t)n * blockIdx.x / gridDim.x);
    const uint32_t hi = blockIdx.x + 1 == gridDim.x ? n + 1 : (uint32_t)((uint64_t)n * (blockIdx.x + 1) / gridDim.x);
    uint32_t kk[IT], vv[IT];
#pragma unroll
    for (int r = 0; r < IT; ++r) {
        const uint32_t idx = (w * IT + r) * WAVE + lane;
        const uint32_t a = act[idx < n ? idx : (n ? n - 1 : 0)];
        if (act_copy && idx < n && idx >= lo && idx < hi) act_copy[idx] = a;
        kk[r] = a < n_act ? a : n_act;
        vv[r] = idx;
    }
    mb_sort_runs_core<BITS, IT>(sh, kk, vv, n, passes, perm, run_act, run_start, n_runs, lo, hi, ts, ballot != 0);
    if (done) {
        __threadfence_system();                    // this thread's host stores before the count
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace gd
