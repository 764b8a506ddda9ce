// gd_turns.h -- gfx950 device code for the turn admission of a received batch: what
// Dispatcher.ReceiveMessage (Core/Dispatcher.cs:75-123) -> ReceiveRequest (:262-301) decides per message under
// lock(activation), after IncomingMessageAgent.ReceiveMessage (gd_receive, gd_actdir.h) found the activation:
//   ActivationMayAcceptRequest / CanInterleave (:313-336), HandleIncomingRequest + RecordRunning (:399-424,
//   ActivationData.cs:475-493), EnqueueRequest + the second CheckOverloaded (:431-466, ActivationData.cs:616-649),
//   ProcessRequestToInvalidActivation -> TryForwardRequest (:468-484, :563-568, :627-630), IsExpired (:79-85).
//
// The rule is sequential per activation (numRunning and Running change along the batch).  Its closed form, per
// context c, with F = the first "eligible" message of c in arrival order (participating, not expired, Request or
// OneWay, state not INVALID) when c is VALID:
//   - !HAS_RUNNING: F is accepted and becomes Running; a later eligible message is accepted iff it interleaves
//     with Running = F -- whose read-only flag is read from message F itself (msg_flags[F]);
//   - HAS_RUNNING: Running never changes; F is accepted outright when num_running starts at 0 (IsCurrently
//     Executing false), every other eligible message iff it interleaves with the context's Running;
//   - the request count never rises along a context (each message changes it by -1 or 0), so a message that is
//     not accepted, of rank j among the context's participating messages, is rejected iff
//     request_count[c] - j > limit.
// So the only order-dependent quantities are F (a minimum over arrival index) and j (the stable rank, from the
// bucketing).
//
// Per batch:
//   k_turn_init      running_idx[c] = none, num_running_out[c] = num_running[c]
//   k_turn_classify  one lane per message: ctx (4 B), receive status (1), direction (1), ttl (8), forward count
//                    (1), flags (1), one context flag byte and, for a context with a Running, num_running;
//                    the two activation keys word by word while they compare equal, and only for a message
//                    nothing else decides.  Writes the turn byte: final, or provisional (TP_*) when it depends
//                    on F or on the rank.  atomicMin of the arrival index into running_idx[c] for the eligible
//                    messages of the contexts that need F, combined within the wave first.  With limits: the
//                    bucketing key (ctx of a participating message, else n_ctx).
//   bucket_device    (limits only) the stable rank of every participating message in its context
//   k_turn_decide    resolves the provisional bytes (1 B + ctx 4 B; F, msg_flags[F], rank, request_count where
//                    needed), adds the STARTs to num_running_out (combined within the wave), counts each tile's
//                    STARTs, writes the wait-list key when the lists are wanted
//   k_turn_finish    running_idx[c] = none where the context had a Running (F was only its outright accept)
//   scan_device, k_turn_starts   start_idx: the stable compaction of the STARTs; *n_start
//   bucket_device    wait_perm / wait_offsets over the wait-list key
//
// Wave-level combining: the lanes of a wave row hold 64 consecutive messages.  The lanes that would touch the
// same context word are peeled group by group (ballot + readlane): one lane a group issues the atomic, with the
// group's minimum (its own index: the lowest lane) or the group's count.  The first group's context is carried
// across the wave's rows, so a context every message of the wave targets takes one atomic a wave.  Past the
// wave: the minimum is skipped when a plain read of the word is already below the lane's index (the word only
// falls), and the counts are combined over the workgroup in a small LDS table before they go to memory -- with
// Zipf(1.1) targets a row holds several hot contexts, and one atomic a row on each of their words serialised.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_common.h"
#include "gd_place.h"
#include "gd_scan.h"
#include "graindispatch.h"

namespace gd {

constexpr int TN_NT = 256;
constexpr int TN_IT = 16;
constexpr uint32_t TN_TILE = TN_NT * TN_IT;         // 4096 messages per workgroup
constexpr int TN_NW = TN_NT / WAVE;
static_assert(TN_TILE == PL_TILE && TN_NT == PL_NT, "k_turn_starts walks k_turn_decide's tiles with pl_load16");

// provisional turn bytes between k_turn_classify and k_turn_decide
constexpr uint32_t TP_PENDING = 0x80u;              // set: not final
constexpr uint32_t TP_KIND = 3u;                    // 0 not accepted; 1 idle context: START iff i == F or both read-only;
                                                    // 2 Running set, num_running 0: START iff i == F
constexpr uint32_t TP_RO = 4u, TP_SW = 8u, TP_STUCK = 16u;

struct TurnArgs {
    const uint8_t* ctx_flags;       // [n_ctx] GD_CTX_*
    const uint32_t* num_running;    // [n_ctx]
    const uint32_t* request_count;  // [n_ctx], null = no limit check
    int32_t hard_limit, hard_limit_sw;
    uint32_t max_forward, chain;
};

// f(key, group, lane is the group's first) once per group of `pred` lanes sharing `key`, in every lane of the
// wave (key and group are wave-uniform).  Call it from uniform control flow only.
template <class F>
__device__ __forceinline__ void wave_groups(bool pred, uint32_t key, F&& f) {
    unsigned long long pend = __ballot(pred);
    const uint32_t lane = lane_id();
    while (pend) {
        const uint32_t lead = (uint32_t)__ffsll((long long)pend) - 1u;
        const uint32_t hk = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)lead);
        const unsigned long long grp = __ballot(pred && key == hk);
        f(hk, grp, lane == lead);
        pend &= ~grp;
    }
}

static __global__ void __launch_bounds__(BLOCK) k_turn_init(const uint32_t* __restrict__ num_running, uint32_t n_ctx,
                                                     uint32_t* __restrict__ num_running_out,
                                                     uint32_t* __restrict__ running_idx) {
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= n_ctx) return;
    num_running_out[c] = num_running[c];
    running_idx[c] = NONE32;
}

static __global__ void __launch_bounds__(BLOCK) k_turn_finish(const uint8_t* __restrict__ ctx_flags, uint32_t n_ctx,
                                                       uint32_t* __restrict__ running_idx) {
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= n_ctx) return;
    if (ctx_flags[c] & GD_CTX_HAS_RUNNING) running_idx[c] = NONE32;
}

__device__ __forceinline__ bool turn_same_key(const gd_key* __restrict__ a, const gd_key* __restrict__ b, uint32_t i) {
    const uint64_t* pa = reinterpret_cast<const uint64_t*>(a + i);
    const uint64_t* pb = reinterpret_cast<const uint64_t*>(b + i);
    return pa[1] == pb[1] && pa[0] == pb[0] && pa[2] == pb[2];   // N1 differs first between activations
}

// The frame-fed chain's adjustments, applied where the turn stage loads a message (no pass of their own): the
// decoder wrote the ttl and the flags as the wire has them.
struct TurnFrameAdj {
    int64_t ttl_age;                // Message.TimeToLive's getter: wire ttl - (UtcNow - _localCreationTime), ticks >= 0
    const uint8_t* flags_or;        // OR-ed into the decoded flags (GD_MSG_MAY_INTERLEAVE comes from C#); may be null
    uint8_t* flags_out;             // with flags_or: the merged flags, for k_turn_decide's read of the Running message's
};

// Item (w, r, lane) of a tile <-> message base + (w * TN_IT + r) * 64 + lane: a wave row is 64 consecutive
// messages, lanes in arrival order.  ADJ: adj is applied (the instantiation without it never reads it).
template <bool ADJ>
static __global__ void __launch_bounds__(TN_NT) k_turn_classify(const uint32_t* __restrict__ ctx,
                                                         const uint8_t* __restrict__ rs,
                                                         const uint8_t* __restrict__ dir,
                                                         const int64_t* __restrict__ ttl,
                                                         const uint8_t* __restrict__ fwd,
                                                         const uint8_t* __restrict__ mflags,
                                                         const gd_key* __restrict__ ta, const gd_key* __restrict__ sa,
                                                         uint32_t n, uint32_t n_ctx, TurnArgs a,
                                                         uint8_t* __restrict__ turn, uint32_t* __restrict__ first,
                                                         uint32_t* __restrict__ pkey, TurnFrameAdj adj) {
    const uint32_t base = blockIdx.x * TN_TILE;
    const uint32_t lane = lane_id(), w = threadIdx.x / WAVE;
    // every streamed load of the thread before the first use (one wait, not one per message)
    uint32_t cv[TN_IT], rv[TN_IT], dv[TN_IT], fv[TN_IT], mv[TN_IT];
    int64_t tv[TN_IT];
#pragma unroll
    for (int r = 0; r < TN_IT; ++r) {
        const uint32_t li = min(base + (w * TN_IT + r) * WAVE + lane, n - 1);
        cv[r] = ctx[li];
        rv[r] = rs ? (uint32_t)rs[li] : (uint32_t)GD_RECV_ACTIVATION;
        dv[r] = dir ? (uint32_t)dir[li] : 0u;
        tv[r] = ttl ? ttl[li] : GD_TTL_NONE;
        fv[r] = fwd ? (uint32_t)fwd[li] : 0u;
        mv[r] = mflags ? (uint32_t)mflags[li] : 0u;
        if (ADJ) {
            if (adj.flags_or) mv[r] |= (uint32_t)adj.flags_or[li];
            // a ttl with a value ages, saturating at INT64_MIN (ttl_age >= 0: it can only fall)
            if (tv[r] != GD_TTL_NONE) tv[r] = tv[r] < INT64_MIN + adj.ttl_age ? INT64_MIN : tv[r] - adj.ttl_age;
        }
    }
    uint32_t hot_key = NONE32;                          // wave-uniform: the context of the wave's first atomic
#pragma unroll
    for (int r = 0; r < TN_IT; ++r) {
        const uint32_t i = base + (w * TN_IT + r) * WAVE + lane;
        const uint32_t c = cv[r];
        const bool part = i < n && c < n_ctx && rv[r] == GD_RECV_ACTIVATION;
        uint32_t t = GD_TURN_NONE;
        bool need_first = false;
        if (part) {
            const uint32_t f = a.ctx_flags[c];
            const uint32_t state = f & GD_CTX_STATE_MASK;
            const uint32_t m = mv[r];
            if (tv[r] != GD_TTL_NONE && tv[r] <= 0) {               // Message.IsExpired
                t = GD_TURN_EXPIRED;
            } else if (dv[r] == 1u) {                               // Response (0xFF = absent = Request)
                t = state == GD_CTX_INVALID ? GD_TURN_RESPONSE_DROPPED : GD_TURN_RESPONSE;
            } else if (state == GD_CTX_INVALID) {                   // MayForward, else the transient rejection
                t = fv[r] < a.max_forward ? GD_TURN_FORWARD : GD_TURN_REJECT_TRANSIENT;
            } else {
                const uint32_t rest = (f & GD_CTX_STATELESS_WORKER ? TP_SW : 0u) | (f & GD_CTX_STUCK ? TP_STUCK : 0u);
                if (state != GD_CTX_VALID) {
                    t = TP_PENDING | rest;                          // NOT_READY: EnqueueRequest
                } else {
                    const bool ro = m & GD_MSG_READ_ONLY;
                    const bool has = f & GD_CTX_HAS_RUNNING;
                    bool inter = (m & (GD_MSG_ALWAYS_INTERLEAVE | GD_MSG_MAY_INTERLEAVE)) || (f & GD_CTX_REENTRANT) ||
                                 (has && ro && (f & GD_CTX_RUNNING_READ_ONLY));
                    if (!inter && a.chain && ta) inter = turn_same_key(ta, sa, i);
                    if (!has) {
                        // the first eligible message starts and becomes Running (its index is the output), the
                        // others interleave with it or not
                        need_first = true;
                        t = inter ? (uint32_t)GD_TURN_START : (TP_PENDING | 1u | (ro ? TP_RO : 0u) | rest);
                    } else {
                        // Running set but nothing executing: the first eligible message, interleaving or not,
                        // is accepted outright and counts as executing for the rest
                        need_first = a.num_running[c] == 0u;
                        t = inter ? (uint32_t)GD_TURN_START : (TP_PENDING | (need_first ? 2u : 0u) | rest);
                    }
                }
            }
        }
        if (i < n) {
            turn[i] = (uint8_t)t;
            if (pkey) pkey[i] = part ? c : n_ctx;
            if (ADJ && adj.flags_out) adj.flags_out[i] = (uint8_t)mv[r];
        }
        // The word only ever falls, so a (possibly stale) read that is already below i makes the atomic
        // redundant: a hot context takes atomics from the waves in flight when the batch starts, not from
        // every wave.  Every lane reads its own word before the peel (one wait, not one a group).
        const uint32_t cur = need_first ? __builtin_nontemporal_load(&first[c]) : 0u;
        wave_groups(need_first, c, [&](uint32_t hk, unsigned long long, bool lead) {
            // rows ascend in arrival order: an earlier row's minimum for the same context stands
            if (hk != hot_key) {
                if (lead && cur > i) atomicMin(&first[hk], i);
                if (hot_key == NONE32) hot_key = hk;
            }
        });
    }
}

// k STARTs of context c, combined over the workgroup: a small LDS table keyed by context (claimed by CAS, counted
// by ds_add); a context that finds its slot taken by another goes to memory directly.
constexpr uint32_t TN_SLOTS = 512;
__device__ __forceinline__ void turn_count(uint32_t* s_key, uint32_t* s_cnt, uint32_t* __restrict__ num_running_out,
                                           uint32_t c, uint32_t k) {
    const uint32_t slot = (c * 2654435761u) >> 23;
    const uint32_t old = atomicCAS(&s_key[slot], NONE32, c);
    if (old == NONE32 || old == c) atomicAdd(&s_cnt[slot], k);
    else atomicAdd(&num_running_out[c], k);
}
static_assert(TN_SLOTS == 1u << 9, "turn_count's slot is the hash's top 9 bits");

// tile_cnt[tile] = the tile's STARTs; tile_cnt[tiles] = 0 (the scan's total lands there).
static __global__ void __launch_bounds__(TN_NT) k_turn_decide(const uint32_t* __restrict__ ctx,
                                                       const uint8_t* __restrict__ mflags, uint32_t n, uint32_t n_ctx,
                                                       TurnArgs a, const uint32_t* __restrict__ first,
                                                       const uint32_t* __restrict__ rank,
                                                       const uint32_t* __restrict__ roff, uint8_t* __restrict__ turn,
                                                       uint32_t* __restrict__ num_running_out,
                                                       uint32_t* __restrict__ wkey, uint32_t* __restrict__ tile_cnt,
                                                       uint32_t tiles) {
    __shared__ uint32_t s_wcnt[TN_NW];
    __shared__ uint32_t s_key[TN_SLOTS], s_cnt[TN_SLOTS];
    for (uint32_t k = threadIdx.x; k < TN_SLOTS; k += TN_NT) {
        s_key[k] = NONE32;
        s_cnt[k] = 0;
    }
    __syncthreads();
    const uint32_t base = blockIdx.x * TN_TILE;
    const uint32_t lane = lane_id(), w = threadIdx.x / WAVE;
    uint32_t cv[TN_IT], pv[TN_IT];
#pragma unroll
    for (int r = 0; r < TN_IT; ++r) {
        const uint32_t li = min(base + (w * TN_IT + r) * WAVE + lane, n - 1);
        cv[r] = ctx[li];
        pv[r] = turn[li];
    }
    uint32_t hot_key = NONE32, hot_cnt = 0, starts = 0;   // wave-uniform
#pragma unroll
    for (int r = 0; r < TN_IT; ++r) {
        const uint32_t i = base + (w * TN_IT + r) * WAVE + lane;
        const uint32_t c = cv[r];
        uint32_t t = i < n ? pv[r] : (uint32_t)GD_TURN_NONE;
        if (t & TP_PENDING) {                           // a participating message: c < n_ctx
            const uint32_t kind = t & TP_KIND;
            bool accept = false;
            if (kind) {
                const uint32_t fi = first[c];
                accept = fi == i;
                // Running's read-only flag from the running message itself
                if (!accept && kind == 1u && (t & TP_RO) && fi < n) accept = mflags[fi] & GD_MSG_READ_ONLY;
            }
            if (accept) {
                t = GD_TURN_START;
            } else {
                const int64_t limit = t & TP_SW ? a.hard_limit_sw : a.hard_limit;
                bool over = false;
                if (rank && limit > 0) over = (int64_t)a.request_count[c] - (int64_t)(rank[i] - roff[c]) > limit;
                t = over ? GD_TURN_REJECT_OVERLOADED : (t & TP_STUCK ? GD_TURN_STUCK : GD_TURN_WAIT);
            }
            turn[i] = (uint8_t)t;
        }
        const bool start = t == GD_TURN_START;
        if (wkey && i < n) wkey[i] = t == GD_TURN_WAIT ? c : n_ctx;
        starts += (uint32_t)__popcll(__ballot(start));
        wave_groups(start, c, [&](uint32_t hk, unsigned long long grp, bool lead) {
            const uint32_t k = (uint32_t)__popcll(grp);
            if (hot_key == NONE32) hot_key = hk;
            if (hk == hot_key) hot_cnt += k;            // carried across the rows: one add a wave
            else if (lead) turn_count(s_key, s_cnt, num_running_out, hk, k);
        });
    }
    if (lane == 0) {
        if (hot_cnt) turn_count(s_key, s_cnt, num_running_out, hot_key, hot_cnt);
        s_wcnt[w] = starts;
    }
    __syncthreads();
    // the workgroup's counts: one global add a context it held
    for (uint32_t k = threadIdx.x; k < TN_SLOTS; k += TN_NT)
        if (s_cnt[k]) atomicAdd(&num_running_out[s_key[k]], s_cnt[k]);
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < TN_NW; ++k) s += s_wcnt[k];
        tile_cnt[blockIdx.x] = s;
        if (blockIdx.x == 0) tile_cnt[tiles] = 0;
    }
}

// start_idx[0 .. n_start): the START messages in arrival order.  Thread t of tile b holds messages
// b * TN_TILE + t * 16 + 0 .. 15, so (tile, wave, lane, byte) order is batch order.  tile_off: the exclusive
// scan of k_turn_decide's counts (tile_off[tiles] = n_start); cap: start_idx's entries.
static __global__ void __launch_bounds__(TN_NT) k_turn_starts(const uint8_t* __restrict__ turn, uint32_t n,
                                                       uint32_t wide, const uint32_t* __restrict__ tile_off,
                                                       uint32_t tiles, uint32_t* __restrict__ start_idx,
                                                       uint32_t cap, uint32_t* __restrict__ n_start) {
    __shared__ uint32_t s_wcnt[TN_NW];
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_start = tile_off[tiles];
    const uint32_t tile_base = tile_off[blockIdx.x];
    if (tile_off[blockIdx.x + 1] == tile_base) return;  // the whole workgroup
    const uint32_t i0 = blockIdx.x * TN_TILE + threadIdx.x * PL_IT;
    uint32_t tw[4];
    pl_load16(turn, i0, n, wide != 0, (uint32_t)GD_TURN_NONE, tw);
    uint32_t m = pl_eq_mask(tw, GD_TURN_START);
    const uint32_t lane = lane_id(), w = threadIdx.x / WAVE;
    uint32_t total;
    const uint32_t pre = pl_wave_prefix((uint32_t)__popc(m), lane, total);
    if (lane == 0) s_wcnt[w] = total;
    __syncthreads();
    uint32_t j = tile_base + pre;
#pragma unroll
    for (int k = 0; k < TN_NW; ++k)
        if ((uint32_t)k < w) j += s_wcnt[k];
    for (; m; m &= m - 1u, ++j)
        if (j < cap) start_idx[j] = i0 + ((uint32_t)__ffs((int)m) - 1u);   // always true when the scan is right
}

}  // namespace gd
