// gd_pump.h -- gfx950 device code for the turn completion and message pump of a batch of completions (DESIGN
// 5.12): what Dispatcher.OnActivationCompletedRequest (Core/Dispatcher.cs:822-843) does per completed request
// under lock(activation): ActivationData.ResetRunning (Catalog/ActivationData.cs:495-514), then RunMessagePump
// (Core/Dispatcher.cs:845-874) over the waiting list with ActivationMayAcceptRequest / CanInterleave (:313-336)
// and RecordRunning (ActivationData.cs:475-493).  The rule, step by step: include/graindispatch.h.
//
// The rule is sequential per activation, and activations do not interact, so the unit of work is a context
// with its completions (bucketed by context, arrival order kept) and its waiting list.  Along a context R takes
// at most the values X -> none -> one waiting position; after that only nr moves.  Two regimes follow:
//   - a pump first takes the accepts that nr <= 0 or R == none force (a count, no scan), then -- nr > 0 and R
//     fixed -- the run of messages the predicate accepts under that R: the first clear bit of its ballot over
//     64 flag bytes a step;
//   - after a pump the head is blocked (or the list is empty) until a completion clears R == X or brings nr to
//     0.  The completions in between only lower nr: they are skipped 64 at a time, with a ballot of the
//     non-PUMP_ONLY flag, each lane's prefix count of it compared with nr, and the IS_RUNNING flag while R == X.
//   A REENTRANT context's predicate holds for every message: its pump takes the whole rest of the list, no scan.
//
// Per batch:
//   bucket_device    the completions by context (done_ctx of a taking-part completion, else n_ctx)
//   k_pump_ctx       one lane per context: no completion -> its state copied; a thin context (completions +
//                    list length < PUMP_THIN) walked by the lane, the literal loop; the rest appended to a work
//                    list, one aggregated atomic a workgroup (the list's order is free: every output is per
//                    context or per completion)
//   k_pump_wave      one wave per listed context, state wave-uniform, the two regimes above
//   scan_device      over n_started_by (+ 1 entry: the total)
//   k_pump_starts    start_pos: completion i's starts are the run first[i] .. first[i] + n_started_by[i]; a tile
//                    of PUMP_START_TILE outputs finds its first and last completion by one binary search each
//                    over the scanned counts, its lanes search only between the two
//   k_merge_count, scan_device, k_merge_copy   the wait-list merge; the copy is one thread per output element
//                    with a binary search over the new offsets -- a first form, kept
//
// PUMP_THIN, PUMP_WAVE_NT, PUMP_SKIP_U and PUMP_START_TILE are design constants; alternatives were not measured
// (PUMP_SKIP_U 1 -> 8 was: DESIGN 5.12).
// Every store is a plain vector store; n_started_by is zero-filled once and written where non-zero.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_common.h"
#include "gd_hash.h"
#include "gd_scan.h"
#include "graindispatch.h"

namespace gd {

constexpr uint32_t PUMP_THIN = 32;                  // completions + list length below this: one lane walks the context
constexpr int PUMP_WAVE_NT = 256;                   // k_pump_wave: 4 waves a workgroup, a context each
constexpr int PUMP_WAVE_NW = PUMP_WAVE_NT / WAVE;
constexpr int PUMP_SKIP_U = 8;                      // k_pump_wave: ballots of 64 completions whose gathers are issued together
constexpr int PUMP_START_NT = 256;
constexpr int PUMP_START_IT = 8;
constexpr uint32_t PUMP_START_TILE = PUMP_START_NT * PUMP_START_IT;   // 2048 start_pos entries per workgroup
constexpr uint32_t PUMP_MSG_STATIC = GD_MSG_ALWAYS_INTERLEAVE | GD_MSG_MAY_INTERLEAVE | GD_MSG_CALL_CHAIN;

struct PumpArgs {
    const uint32_t* boff;           // [n_ctx + 2] the completions bucketed by context; null: no completions
    const uint32_t* bperm;          // [n_done]
    const uint8_t* done_flags;      // [n_done] or null
    const uint8_t* ctx_flags;       // [n_ctx]
    const uint32_t* num_running;    // [n_ctx]
    const uint32_t* woff;           // [n_ctx + 1]
    const uint8_t* wflags;          // [woff[n_ctx]]
    uint32_t wait_cap, n_ctx;
    uint8_t* ctx_flags_out;
    uint32_t *num_running_out, *n_dequeued, *running_pos;
    uint8_t* event;
    uint32_t* cnt;                  // n_started_by, zero-filled; null: not wanted
    uint32_t* first;                // [n_done] the first position completion i started; null: not wanted
};

// nr, R (rk: 0 none, 1 the batch-start Running X, 2 the waiting position rpos; ro = R's read-only flag), the
// list head p, the events.
struct PumpState {
    int32_t nr;
    uint32_t rk, ro, rpos, p, ev;
};

__device__ __forceinline__ PumpState pump_begin(uint32_t f, uint32_t nr, uint32_t lo) {
    return PumpState{(int32_t)nr, f & GD_CTX_HAS_RUNNING ? 1u : 0u, f & GD_CTX_RUNNING_READ_ONLY ? 1u : 0u, NONE32,
                     lo, 0u};
}

// ResetRunning
__device__ __forceinline__ void pump_reset(PumpState& s, uint32_t df) {
    if (df & GD_DONE_PUMP_ONLY) return;
    s.nr = (int32_t)((uint32_t)s.nr - 1u);
    if (s.nr == 0) s.ev |= GD_PUMP_BECAME_IDLE;
    if (s.rk == 1u && (df & GD_DONE_IS_RUNNING)) {
        s.rk = 0u;
        s.ev |= GD_PUMP_RUNNING_CLEARED;
    }
}

__device__ __forceinline__ void pump_accept_first(PumpState& s, uint32_t f) {
    if (s.rk != 0u) return;
    s.rk = 2u;
    s.rpos = s.p;
    s.ro = f & GD_MSG_READ_ONLY ? 1u : 0u;
    s.ev |= GD_PUMP_RUNNING_SET;
}

__device__ __forceinline__ void pump_store(const PumpArgs& a, uint32_t c, uint32_t f, const PumpState& s, uint32_t lo) {
    a.num_running_out[c] = (uint32_t)s.nr;
    a.ctx_flags_out[c] = (uint8_t)((f & ~(GD_CTX_HAS_RUNNING | GD_CTX_RUNNING_READ_ONLY)) |
                                   (s.rk ? GD_CTX_HAS_RUNNING : 0u) | (s.rk && s.ro ? GD_CTX_RUNNING_READ_ONLY : 0u));
    a.n_dequeued[c] = s.p - lo;
    a.running_pos[c] = s.rk == 2u ? s.rpos : NONE32;
    a.event[c] = (uint8_t)s.ev;
}

// Context c's list, clamped into [0, wait_cap] (the caller promises offsets[n_ctx] <= wait_cap; nothing at or
// past wait_cap is read whatever the offsets hold).
__device__ __forceinline__ void pump_list(const PumpArgs& a, uint32_t c, uint32_t& lo, uint32_t& hi) {
    hi = min(a.woff[c + 1], a.wait_cap);
    lo = min(a.woff[c], hi);
}

// RunMessagePump by one lane: the literal loop.  Returns the messages started.
__device__ __forceinline__ uint32_t pump_serial(PumpState& s, uint32_t hi, bool reent, const uint8_t* __restrict__ wflags) {
    const uint32_t p0 = s.p;
    while (s.p < hi) {
        const uint32_t f = wflags[s.p];
        const bool ok = s.nr <= 0 || s.rk == 0u || reent || (f & PUMP_MSG_STATIC) || (s.ro && (f & GD_MSG_READ_ONLY));
        if (!ok) break;
        s.nr = (int32_t)((uint32_t)s.nr + 1u);
        pump_accept_first(s, f);
        ++s.p;
    }
    return s.p - p0;
}

// work[0 .. *n_work): the contexts k_pump_wave walks (*n_work zero on entry; entries past work_cap are dropped,
// which the bound the host computes it from rules out).
static __global__ void __launch_bounds__(BLOCK) k_pump_ctx(PumpArgs a, uint32_t* __restrict__ work,
                                                    uint32_t* __restrict__ n_work, uint32_t work_cap) {
    __shared__ uint32_t s_n, s_base;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    bool fat = false;
    if (c < a.n_ctx) {
        const uint32_t kb = a.boff ? a.boff[c] : 0u, ke = a.boff ? a.boff[c + 1] : 0u;
        const uint32_t f = a.ctx_flags[c];
        const uint32_t nr = a.num_running[c];
        if (ke <= kb) {
            a.num_running_out[c] = nr;
            a.ctx_flags_out[c] = (uint8_t)f;
            a.n_dequeued[c] = 0u;
            a.running_pos[c] = NONE32;
            a.event[c] = 0;
        } else {
            uint32_t lo, hi;
            pump_list(a, c, lo, hi);
            if ((uint64_t)(ke - kb) + (hi - lo) < PUMP_THIN) {
                PumpState s = pump_begin(f, nr, lo);
                const bool valid = (f & GD_CTX_STATE_MASK) == GD_CTX_VALID;
                const bool reent = f & GD_CTX_REENTRANT;
                for (uint32_t k = kb; k < ke; ++k) {
                    const uint32_t i = a.bperm[k];
                    pump_reset(s, a.done_flags ? (uint32_t)a.done_flags[i] : 0u);
                    if (!valid) continue;
                    const uint32_t p0 = s.p;
                    const uint32_t started = pump_serial(s, hi, reent, a.wflags);
                    if (started && a.cnt) {
                        a.cnt[i] = started;
                        if (a.first) a.first[i] = p0;
                    }
                }
                pump_store(a, c, f, s, lo);
            } else {
                fat = true;
            }
        }
    }
    uint32_t slot = 0;
    if (fat) slot = atomicAdd(&s_n, 1u);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) s_base = atomicAdd(n_work, s_n);
    __syncthreads();
    if (fat && s_base + slot < work_cap) work[s_base + slot] = c;
}

// RunMessagePump by a wave, state wave-uniform.  Returns the messages started.
__device__ __forceinline__ uint32_t pump_wave(PumpState& s, uint32_t hi, bool reent, const uint8_t* __restrict__ wflags,
                                              uint32_t lane) {
    const uint32_t p0 = s.p;
    if (s.p >= hi) return 0u;
    // the accepts nr <= 0 (until it is positive) or R == none (one) force, whatever the flags
    const int64_t forced = s.nr <= 0 ? 1 - (int64_t)s.nr : (s.rk == 0u ? 1 : 0);
    const uint32_t avail = hi - s.p;
    const uint32_t take = forced < (int64_t)avail ? (uint32_t)forced : avail;
    if (take) {
        if (s.rk == 0u) pump_accept_first(s, wflags[s.p]);
        s.nr = (int32_t)((uint32_t)s.nr + take);
        s.p += take;
    }
    if ((int64_t)take != forced || s.p >= hi) return s.p - p0;
    if (reent) {                                        // the predicate holds for every message: no scan
        s.nr = (int32_t)((uint32_t)s.nr + (hi - s.p));
        s.p = hi;
        return s.p - p0;
    }
    // nr > 0 and R fixed from here: the run the predicate accepts, 64 flag bytes a step; the next step's bytes
    // are in flight during the ballot
    uint64_t q = (uint64_t)s.p + lane;
    uint32_t f = q < hi ? (uint32_t)wflags[q] : 0u;
    for (;;) {
        const uint64_t qn = (uint64_t)s.p + WAVE + lane;
        const uint32_t fn = qn < hi ? (uint32_t)wflags[qn] : 0u;
        const bool in = (uint64_t)s.p + lane < hi;
        const bool acc = (f & PUMP_MSG_STATIC) || (s.ro && (f & GD_MSG_READ_ONLY));
        const unsigned long long in_m = __ballot(in);
        const unsigned long long stop = in_m & ~__ballot(in && acc);
        const uint32_t k = stop ? (uint32_t)__ffsll((long long)stop) - 1u : (uint32_t)__popcll(in_m);
        s.nr = (int32_t)((uint32_t)s.nr + k);
        s.p += k;
        if (k < (uint32_t)WAVE) break;
        f = fn;
    }
    return s.p - p0;
}

static __global__ void __launch_bounds__(PUMP_WAVE_NT) k_pump_wave(PumpArgs a, const uint32_t* __restrict__ work,
                                                            const uint32_t* __restrict__ n_work, uint32_t work_cap) {
    const uint32_t lane = lane_id();
    const uint32_t nwaves = gridDim.x * PUMP_WAVE_NW;
    const uint32_t nw = min(*n_work, work_cap);
    for (uint32_t w = blockIdx.x * PUMP_WAVE_NW + threadIdx.x / WAVE; w < nw; w += nwaves) {
        const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)work[w]);
        const uint32_t kb = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.boff[c]);
        const uint32_t ke = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.boff[c + 1]);
        const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.ctx_flags[c]);
        uint32_t lo, hi;
        pump_list(a, c, lo, hi);
        lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
        hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)hi);
        PumpState s = pump_begin(f, (uint32_t)__builtin_amdgcn_readfirstlane((int)a.num_running[c]), lo);
        const bool valid = (f & GD_CTX_STATE_MASK) == GD_CTX_VALID;
        const bool reent = f & GD_CTX_REENTRANT;
        // blocked: a pump now would start nothing, and that stays so until R == X is cleared or nr reaches 0
        // (true after every pump; a pump that never runs leaves nothing to re-test)
        bool blocked = !valid;
        uint32_t k = kb;
        while (k < ke) {
            if (!blocked) {
                const uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.bperm[k]);
                const uint32_t df = a.done_flags ? (uint32_t)__builtin_amdgcn_readfirstlane((int)a.done_flags[i]) : 0u;
                pump_reset(s, df);
                if (valid) {
                    const uint32_t p0 = s.p;
                    const uint32_t started = pump_wave(s, hi, reent, a.wflags, lane);
                    if (started && a.cnt && lane == 0) {
                        a.cnt[i] = started;
                        if (a.first) a.first[i] = p0;
                    }
                }
                blocked = true;
                ++k;
                continue;
            }
            // the first completion that clears R == X or brings nr to 0, if any: 64 completions a ballot, the
            // flag gathers of PUMP_SKIP_U ballots in flight together (a hot context's walk is their latency)
            const uint32_t span = min(ke - k, (uint32_t)(WAVE * PUMP_SKIP_U));
            uint32_t dfv[PUMP_SKIP_U];
#pragma unroll
            for (int j = 0; j < PUMP_SKIP_U; ++j) {
                const uint32_t idx = (uint32_t)j * WAVE + lane;
                dfv[j] = idx < span && a.done_flags ? (uint32_t)a.done_flags[a.bperm[k + idx]] : 0u;
            }
            const uint32_t k0 = k;
#pragma unroll
            for (int j = 0; j < PUMP_SKIP_U; ++j) {
                if (!blocked || (uint32_t)j * WAVE >= span) break;
                const uint32_t m = min(span - (uint32_t)j * WAVE, (uint32_t)WAVE);
                const uint32_t df = dfv[j];
                const bool lowers = lane < m && !(df & GD_DONE_PUMP_ONLY);
                const unsigned long long low_m = __ballot(lowers);
                // the lowering completions up to and including this lane's
                const uint32_t upto = (uint32_t)__popcll(low_m & ((2ull << lane) - 1ull));
                const bool trig = lowers && ((s.rk == 1u && (df & GD_DONE_IS_RUNNING)) || (int64_t)upto == (int64_t)s.nr);
                const unsigned long long trig_m = __ballot(trig);
                if (!trig_m) {
                    s.nr = (int32_t)((uint32_t)s.nr - (uint32_t)__popcll(low_m));
                    k = k0 + (uint32_t)j * WAVE + m;
                } else {
                    const uint32_t t = (uint32_t)__ffsll((long long)trig_m) - 1u;
                    s.nr = (int32_t)((uint32_t)s.nr - (uint32_t)__popcll(low_m & ((1ull << t) - 1ull)));
                    k = k0 + (uint32_t)j * WAVE + t;
                    blocked = false;
                }
            }
        }
        if (lane == 0) pump_store(a, c, f, s, lo);
    }
}

// start_pos[j] for j < total = scan[n_done] (scan: the exclusive scan of n_started_by, n_done + 1 entries):
// the completion i with scan[i] <= j < scan[i + 1] started position first[i] + (j - scan[i]).
__device__ __forceinline__ uint32_t pump_owner(const uint32_t* __restrict__ scan, uint32_t lo, uint32_t hi, uint32_t j) {
    // scan[lo] <= j < scan[hi]: the last index whose scan is <= j
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (scan[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

static __global__ void __launch_bounds__(PUMP_START_NT) k_pump_starts(const uint32_t* __restrict__ scan,
                                                               const uint32_t* __restrict__ first, uint32_t n_done,
                                                               uint32_t* __restrict__ start_pos, uint32_t cap,
                                                               uint32_t* __restrict__ n_start) {
    __shared__ uint32_t s_i[2];
    const uint32_t total = scan[n_done];
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_start = total;
    const uint64_t j0 = (uint64_t)blockIdx.x * PUMP_START_TILE;
    if (j0 >= total) return;                            // the whole workgroup
    const uint32_t j1 = (uint32_t)min(j0 + PUMP_START_TILE, (uint64_t)total) - 1u;   // the tile's last output
    if (threadIdx.x < 2) s_i[threadIdx.x] = pump_owner(scan, 0u, n_done, threadIdx.x ? j1 : (uint32_t)j0);
    __syncthreads();
    const uint32_t i_lo = s_i[0], i_hi = s_i[1] + 1u;   // scan[i_lo] <= j < scan[i_hi] for every j of the tile
#pragma unroll
    for (int r = 0; r < PUMP_START_IT; ++r) {
        const uint64_t j = j0 + (uint32_t)r * PUMP_START_NT + threadIdx.x;
        if (j > j1 || j >= cap) continue;
        const uint32_t i = pump_owner(scan, i_lo, i_hi, (uint32_t)j);
        start_pos[j] = first[i] + ((uint32_t)j - scan[i]);
    }
}

// ---- the wait-list merge ----------------------------------------------------------------------
struct MergeArgs {
    const uint32_t *old_off, *old_msg;      // null: no old list
    const uint8_t* old_flags;
    const uint32_t* n_deq;                  // null: nothing dequeued
    const uint32_t *wperm, *woff;           // a gd_turns result
    const uint32_t* msg_id;                 // null: id_base + i
    const uint8_t* msg_flags;               // null: 0
    const gd_key *ta, *sa;                  // null: no call-chain bit
    uint32_t n, n_ctx, id_base, cap;
};

__device__ __forceinline__ void merge_old(const MergeArgs& a, uint32_t c, uint32_t& start, uint32_t& rest) {
    start = 0u;
    rest = 0u;
    if (!a.old_off) return;
    const uint32_t lo = a.old_off[c], hi = a.old_off[c + 1];
    const uint32_t len = hi > lo ? hi - lo : 0u;
    const uint32_t d = a.n_deq ? min(a.n_deq[c], len) : 0u;
    start = lo + d;
    rest = len - d;
}

// new_off[c] = context c's new length; new_off[n_ctx] = 0 (the scan's total lands there).
static __global__ void __launch_bounds__(BLOCK) k_merge_count(MergeArgs a, uint32_t* __restrict__ new_off) {
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c > a.n_ctx) return;
    uint32_t len = 0u;
    if (c < a.n_ctx) {
        uint32_t start, rest;
        merge_old(a, c, start, rest);
        len = rest + (a.woff[c + 1] - a.woff[c]);
    }
    new_off[c] = len;
}

static __global__ void __launch_bounds__(BLOCK) k_merge_copy(MergeArgs a, const uint32_t* __restrict__ new_off,
                                                      uint32_t* __restrict__ msg, uint8_t* __restrict__ flags,
                                                      uint32_t* __restrict__ total_out) {
    const uint32_t total = new_off[a.n_ctx];
    if (blockIdx.x == 0 && threadIdx.x == 0) *total_out = total;
    const uint32_t lim = min(total, a.cap);
    for (uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; p < lim; p += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t c = pump_owner(new_off, 0u, a.n_ctx, (uint32_t)p);
        const uint32_t k = (uint32_t)p - new_off[c];
        uint32_t start, rest;
        merge_old(a, c, start, rest);
        uint32_t m, f;
        if (k < rest) {
            m = a.old_msg[start + k];
            f = a.old_flags[start + k];
        } else {
            const uint32_t i = min(a.wperm[a.woff[c] + (k - rest)], a.n - 1u);
            m = a.msg_id ? a.msg_id[i] : a.id_base + i;
            f = a.msg_flags ? (uint32_t)a.msg_flags[i] : 0u;
            if (a.ta) {
                const uint64_t* pa = reinterpret_cast<const uint64_t*>(a.ta + i);
                const uint64_t* pb = reinterpret_cast<const uint64_t*>(a.sa + i);
                if (pa[1] == pb[1] && pa[0] == pb[0] && pa[2] == pb[2]) f |= GD_MSG_CALL_CHAIN;
            }
        }
        msg[p] = m;
        flags[p] = (uint8_t)f;
    }
}

}  // namespace gd
