// gd_workers.h -- gfx950 device code of the stateless-worker stage: the worker sets of
// ActivationDirectory (Catalog/ActivationDirectory.cs:86-158: RecordNewTarget, RemoveTarget, FindTargets) as one
// open-addressing table in HBM, and StatelessWorkerDirector.SelectActivationCore
// (Placement/StatelessWorkerDirector.cs:31-62) for a batch.
//
// The table.  GrainId -> set, keyed by the 24-B GrainId of category Grain: the directory's 32-B Slot (gd_common.h),
// its home (home_slot of the Jenkins hash), its states, its claim and its election word -- gd_dirbatch.h's
// claim_walk and rehash_place over DirSlots, as the gateway's tables use them.  Beside each slot, 2 + slot_capacity
// words: {count, max_local, the ctx list in List<ActivationData> order}.  A set whose list empties is tombstoned.
//
// The batch model of the select (one legal interleaving of the reference; graindispatch.h has the contract):
// messages are addressed in batch order and each is delivered before the next is addressed, so a worker picked
// while inactive executes for the rest of the batch, a worker the batch creates stays in state Create, and nothing
// completes inside the batch.  Per set, with c entries, MaxLocal m, a of them idle at the batch start and
// room = max(0, m - c): the message of stable rank k in its set is IDLE on the k-th idle entry (k < a), NEW
// (a <= k < a + room), else RANDOM over the final list of c + room entries.
//
// Launches:
//   select  k_wk_find (plain-load walk: the slot, or SLOT_RETRY for a grain with no set; counts those),
//           k_wk_claim passes (gated on that count, then as the gateway's), the stable bucketing over slots
//           (bucket_device: perm, offsets, the inverse permutation = each message's rank), k_wk_sets (one wave a
//           touched slot: a set the batch created gets its words; the idle entries are compacted by ballot and
//           prefix popcount and handed to the set's first messages), k_wk_classify (pick, the NEW flags),
//           scan_device (the NEW ranks), k_wk_finish (NEW: number, append, list; RANDOM: the gather),
//           k_wk_commit (the counts)
//   add     k_wk_find, k_wk_claim passes, the bucketing, k_wk_sets (new sets only), k_wk_add_apply, k_wk_add_commit
//   remove  k_wk_find (no claims), the bucketing, k_wk_remove_sets (one wave a touched slot: the list in LDS, the
//           set's pairs in batch order, the survivors compacted back)
//   lookup  k_wk_lookup (one wave a key)
//   rebuild k_wk_rehash into a zeroed table
// No per-message atomic touches a per-set word: ranks come from the bucketing, NEW numbers from a scan, and each
// appended entry has its own list position.  Every store is a plain vector store or a device-scope atomic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "gd_common.h"
#include "gd_dirbatch.h"
#include "gd_hash.h"
#include "graindispatch.h"

namespace gd {

constexpr uint32_t WK_PASSES = REG_PASSES;       // claim passes of the device forms
constexpr uint32_t WK_ERR_FULL = 2u;             // DevCounters::err (claim_walk's bit)
constexpr uint32_t WK_SET_NT = WAVE;             // the set passes: one wave a table slot
constexpr uint32_t WK_HDR = 2;                   // words before a set's list: count, max_local

struct WkTab {
    Slot* slots;
    unsigned long long mask;
    DevCounters* ctr;
    uint32_t* last;                   // election words (word 0 of each slot is used)
    uint32_t* side;                   // [mask + 1][WK_HDR + sc]
    uint32_t sc;                      // slot_capacity
};
__device__ __forceinline__ uint32_t* wk_set(const WkTab& t, unsigned long long s) {
    return t.side + s * (unsigned long long)(WK_HDR + t.sc);
}

// System.Random.Next(maxValue) on the internal sample `draw` (what Next() returned): Sample() = draw * (1.0 / Int32.MaxValue),
// then (int)(Sample() * maxValue).  Two double roundings, no fused multiply-add.
__device__ __forceinline__ uint32_t wk_random_index(uint32_t draw, uint32_t C) {
    const double sample = __dmul_rn((double)draw, 1.0 / 2147483647.0);
    const uint32_t r = (uint32_t)(int32_t)__dmul_rn(sample, (double)C);
    return min(r, C - 1u);
}

struct WkSetShape {
    uint32_t c, room;
};
__device__ __forceinline__ WkSetShape wk_shape(const uint32_t* sd, uint32_t sc) {
    const uint32_t c = min(sd[0], sc), m = min(sd[1], sc);
    return WkSetShape{c, m > c ? m - c : 0u};
}

// ------------------------------------------------------------------ find, claim
// One lane a key.  A key takes part when its category is Grain and its max_local (nullable array) is at most sc.
// slot_of: the set's slot; SLOT_RETRY when the grain has no set and claim_missing (the claim passes create it);
// NONE32 otherwise.  pre8 (nullable) receives pre_other for a key of another category, else pre_held: what the
// later kernels leave in place for a message they do not reach.  pre_ctx (nullable) receives NONE32.
static __global__ void __launch_bounds__(BLOCK) k_wk_find(const gd_key* __restrict__ keys, uint32_t n, WkTab t,
                                                   const int32_t* __restrict__ max_local, uint32_t claim_missing,
                                                   uint32_t* __restrict__ slot_of, uint8_t* __restrict__ is_new,
                                                   uint32_t* miss, uint8_t* __restrict__ pre8, uint32_t pre_other,
                                                   uint32_t pre_held, uint32_t* __restrict__ pre_ctx) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool missed = false;
    if (i < n) {
        const uint64_t tcd = keys[i].type_code_data;
        const bool grain = (uint32_t)(tcd >> 56) == CAT_GRAIN;
        uint32_t s = NONE32;
        if (grain && !(max_local && max_local[i] > (int32_t)t.sc)) {
            uint4 b;
            s = find_slot(t.slots, t.mask, t.ctr->max_probe, keys[i].n0, keys[i].n1, tcd, b);
            if (s == NONE32 && claim_missing) {
                s = SLOT_RETRY;
                missed = true;
            }
        }
        slot_of[i] = s;
        is_new[i] = 0;
        if (pre8) pre8[i] = (uint8_t)(grain ? pre_held : pre_other);
        if (pre_ctx) pre_ctx[i] = NONE32;
    }
    count_deferred(miss, missed);
}

// A claim pass over the items left SLOT_RETRY (k_wk_find's misses, or the previous pass's deferred).  gate: the
// count that has to be non-zero for the pass to run; retry: this pass's deferred.  An item that ends on an entry
// of this batch votes ~i: the first message of a new set decides its MaxLocal.
static __global__ void __launch_bounds__(BLOCK) k_wk_claim(const gd_key* __restrict__ keys, uint32_t n, WkTab t,
                                                    uint32_t* __restrict__ slot_of, uint8_t* __restrict__ is_new,
                                                    uint32_t pass, const uint32_t* __restrict__ gate, uint32_t* retry) {
    if (gate && *gate == 0) return;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pd = 0;
    bool reused = false;
    if (i < n && slot_of[i] == SLOT_RETRY) {
        reg_claim_item(i, keys, t.slots, t.mask, t.ctr, slot_of, is_new, nullptr, TableArgs{}, retry, pd, reused,
                       claim_tag(pass), t.last);
        const uint32_t s = slot_of[i];
        if (s < SLOT_RETRY && is_new[i]) atomicMax(&t.last[s], ~i);
    }
    claim_counters(t.ctr, pd, reused);
}

// The device forms' last gated pass left items deferred: the batch is flagged.
static __global__ void __launch_bounds__(WAVE) k_wk_settled(DevCounters* ctr, const uint32_t* __restrict__ unsettled) {
    if (threadIdx.x == 0 && *unsettled) atomicOr(&ctr->err, ERR_UNSETTLED);
}

// ------------------------------------------------------------------ the per-set pass (select, add)
struct WkTurns {
    uint32_t n_ctx;
    const uint8_t* ctx_flags;
    const uint32_t* num_running;
    const uint32_t* wait_offsets;     // nullable: every waiting list empty
};
// ActivationData.IsInactive (ActivationData.cs:689-703) behind the Valid test of SelectActivationCore (:49).
__device__ __forceinline__ bool wk_idle(const WkTurns& w, uint32_t ctx) {
    if (ctx >= w.n_ctx) return false;
    if ((w.ctx_flags[ctx] & GD_CTX_STATE_MASK) != GD_CTX_VALID) return false;
    if ((int32_t)w.num_running[ctx] > 0) return false;
    return !w.wait_offsets || w.wait_offsets[ctx + 1] == w.wait_offsets[ctx];
}

// One wave a table slot; a slot none of the batch's items ended on leaves at once.  A set this batch created
// (PENDING) gets count 0 and the MaxLocal of its first item (the election word), goes LIVE, and its word is
// cleared.  select: the idle entries in list order; the j-th goes to the set's j-th message (d_ctx), their number
// to acnt[slot].
static __global__ void __launch_bounds__(BLOCK) k_wk_sets(WkTab t, const uint32_t* __restrict__ offsets,
                                                       const uint32_t* __restrict__ perm, uint32_t n,
                                                       const int32_t* __restrict__ max_local, uint32_t default_ml,
                                                       uint32_t select, WkTurns w, uint32_t* __restrict__ acnt,
                                                       uint32_t* __restrict__ d_ctx) {
    const unsigned long long s = (unsigned long long)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    if (s > t.mask) return;
    const uint32_t b0 = offsets[s], cnt = offsets[s + 1] - b0;
    if (cnt == 0) return;
    uint32_t* sd = wk_set(t, s);
    const bool fresh = slot_state(t.slots[s].meta) == SLOT_PENDING;
    uint32_t c = 0;
    if (fresh) {
        const uint32_t first = ~t.last[s];
        int32_t m = max_local && first < n ? max_local[first] : 0;
        if (m <= 0) m = (int32_t)default_ml;
        if (lane == 0) {
            sd[0] = 0;
            sd[1] = (uint32_t)m;
            t.slots[s].act = 0;
            t.slots[s].meta = make_meta(SLOT_LIVE, 0);
            t.last[s] = 0;
        }
    } else {
        c = min(sd[0], t.sc);
    }
    if (select) {
        uint32_t a = 0;
        for (uint32_t j0 = 0; j0 < c; j0 += WAVE) {
            const uint32_t j = j0 + lane;
            const uint32_t ctx = j < c ? sd[WK_HDR + j] : NONE32;
            const bool idle = j < c && wk_idle(w, ctx);
            const unsigned long long m = __ballot(idle);
            const uint32_t pos = a + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (idle && pos < cnt) d_ctx[perm[b0 + pos]] = ctx;
            a += (uint32_t)__popcll(m);
        }
        if (lane == 0) acnt[s] = a;
    }
    live_delta(t.ctr, fresh && lane == 0, false);
}

// ------------------------------------------------------------------ select
// One lane a message (and one for flag[n] = 0, where the scan's total lands).  pick for every message that has a
// slot; flag[i] = the message creates a worker.
static __global__ void __launch_bounds__(BLOCK) k_wk_classify(uint32_t n, WkTab t, const uint32_t* __restrict__ slot_of,
                                                       const uint32_t* __restrict__ rank,
                                                       const uint32_t* __restrict__ offsets,
                                                       const uint32_t* __restrict__ acnt,
                                                       const uint32_t* __restrict__ draw, uint8_t* __restrict__ pick,
                                                       uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > n) return;
    uint32_t f = 0;
    if (i < n) {
        const uint32_t s = slot_of[i];
        if (s < SLOT_RETRY) {
            const uint32_t k = rank[i] - offsets[s], a = acnt[s];
            const WkSetShape sh = wk_shape(wk_set(t, s), t.sc);
            uint32_t p;
            if (k < a) {
                p = GD_WK_IDLE;
            } else if (k - a < sh.room) {
                p = GD_WK_NEW;
                f = 1;
            } else if (sh.c + sh.room == 1u) {
                p = GD_WK_RANDOM;                            // local.Count == 1: the draw is not read
            } else {
                p = draw && draw[i] < 0x7FFFFFFFu ? GD_WK_RANDOM : GD_WK_HELD;
            }
            pick[i] = (uint8_t)p;
        }
    }
    flag[i] = f;
}

// pos: the exclusive scan of the flags.  NEW: the worker's number, its place in the set's list and in new_idx.
// RANDOM: the entry of the final list -- one the set had, or the number of the NEW message that appends it.
static __global__ void __launch_bounds__(BLOCK) k_wk_finish(uint32_t n, WkTab t, const uint32_t* __restrict__ slot_of,
                                                     const uint32_t* __restrict__ rank,
                                                     const uint32_t* __restrict__ offsets,
                                                     const uint32_t* __restrict__ perm,
                                                     const uint32_t* __restrict__ acnt,
                                                     const uint32_t* __restrict__ draw,
                                                     const uint32_t* __restrict__ pos, uint32_t ctx_base,
                                                     const uint8_t* __restrict__ pick, uint32_t* __restrict__ d_ctx,
                                                     uint32_t* __restrict__ new_idx, uint32_t* __restrict__ n_new) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0 && n_new) *n_new = pos[n];
    if (i >= n) return;
    const uint32_t s = slot_of[i];
    if (s >= SLOT_RETRY) return;
    const uint32_t p = pick[i];
    if (p != GD_WK_NEW && p != GD_WK_RANDOM) return;
    uint32_t* sd = wk_set(t, s);
    const uint32_t b0 = offsets[s], k = rank[i] - b0, a = acnt[s];
    const WkSetShape sh = wk_shape(sd, t.sc);
    if (p == GD_WK_NEW) {
        const uint32_t g = pos[i], ctx = ctx_base + g;
        d_ctx[i] = ctx;
        sd[WK_HDR + sh.c + (k - a)] = ctx;                   // c + (k - a) < c + room <= sc
        if (new_idx) new_idx[g] = i;
    } else {
        const uint32_t C = sh.c + sh.room;
        const uint32_t r = C == 1u ? 0u : wk_random_index(draw[i], C);
        // r >= c: the (r - c)-th worker this batch appends, made by the set's message of rank a + (r - c)
        d_ctx[i] = r < sh.c ? sd[WK_HDR + r] : ctx_base + pos[perm[b0 + a + (r - sh.c)]];
    }
}

// One lane a table slot: a touched set's count takes the workers the batch appended.
static __global__ void __launch_bounds__(BLOCK) k_wk_commit(WkTab t, const uint32_t* __restrict__ offsets,
                                                     const uint32_t* __restrict__ acnt) {
    const unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (s > t.mask) return;
    const uint32_t cnt = offsets[s + 1] - offsets[s];
    if (cnt == 0) return;
    uint32_t* sd = wk_set(t, s);
    const WkSetShape sh = wk_shape(sd, t.sc);
    const uint32_t a = acnt[s];
    sd[0] = sh.c + min(sh.room, cnt > a ? cnt - a : 0u);
}

// ------------------------------------------------------------------ add
// RecordNewTarget (ActivationDirectory.cs:86-93): item i of rank k in its set lands at list position count + k.
static __global__ void __launch_bounds__(BLOCK) k_wk_add_apply(const uint32_t* __restrict__ ctx, uint32_t n, WkTab t,
                                                        const uint32_t* __restrict__ slot_of,
                                                        const uint32_t* __restrict__ rank,
                                                        const uint32_t* __restrict__ offsets,
                                                        uint8_t* __restrict__ out_status) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slot_of[i];
    if (s >= SLOT_RETRY) return;
    uint32_t* sd = wk_set(t, s);
    const unsigned long long at = (unsigned long long)min(sd[0], t.sc) + (rank[i] - offsets[s]);
    if (at < t.sc) sd[WK_HDR + at] = ctx[i];
    out_status[i] = (uint8_t)(at < t.sc ? GD_WK_ADDED : GD_WK_FULL);
}
static __global__ void __launch_bounds__(BLOCK) k_wk_add_commit(WkTab t, const uint32_t* __restrict__ offsets) {
    const unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (s > t.mask) return;
    const uint32_t cnt = offsets[s + 1] - offsets[s];
    if (cnt == 0) return;
    uint32_t* sd = wk_set(t, s);
    sd[0] = (uint32_t)min((unsigned long long)min(sd[0], t.sc) + cnt, (unsigned long long)t.sc);
}

// ------------------------------------------------------------------ remove
// One wave a table slot, the list in LDS.  The set's pairs in batch order (list.Remove, ActivationDirectory.cs:
// 116-147): the first entry still present that equals the ctx goes (NONE32 marks it), the survivors are written
// back in order; an emptied set is tombstoned.  Work: pairs of the set x entries / 64.
static __global__ void __launch_bounds__(WK_SET_NT) k_wk_remove_sets(WkTab t, const uint32_t* __restrict__ offsets,
                                                              const uint32_t* __restrict__ perm,
                                                              const uint32_t* __restrict__ ctx,
                                                              uint8_t* __restrict__ out_removed) {
    __shared__ uint32_t s_list[GD_WK_MAX_SLOT_CAPACITY];
    const unsigned long long s = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t b0 = offsets[s], cnt = offsets[s + 1] - b0;
    if (cnt == 0) return;
    uint32_t* sd = wk_set(t, s);
    const uint32_t c = min(sd[0], t.sc);
    for (uint32_t j = lane; j < c; j += WAVE) s_list[j] = sd[WK_HDR + j];
    __syncthreads();
    for (uint32_t r = 0; r < cnt; ++r) {
        const uint32_t i = perm[b0 + r], x = ctx[i];
        bool found = false;
        for (uint32_t j0 = 0; j0 < c && !found && x != NONE32; j0 += WAVE) {
            const uint32_t j = j0 + lane;
            const unsigned long long hit = __ballot(j < c && s_list[j] == x);
            if (hit) {
                found = true;
                if (lane == 0) s_list[j0 + (uint32_t)__ffsll((long long)hit) - 1u] = NONE32;
            }
        }
        __syncthreads();
        if (lane == 0 && out_removed) out_removed[i] = found ? 1 : 0;
    }
    uint32_t kept = 0;
    for (uint32_t j0 = 0; j0 < c; j0 += WAVE) {
        const uint32_t j = j0 + lane;
        const uint32_t v = j < c ? s_list[j] : NONE32;
        const unsigned long long m = __ballot(v != NONE32);
        if (v != NONE32) sd[WK_HDR + kept + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = v;
        kept += (uint32_t)__popcll(m);
    }
    const bool gone = kept == 0;
    if (lane == 0) {
        sd[0] = kept;
        if (gone) t.slots[s].meta = make_meta(SLOT_TOMB, 0);
    }
    live_delta(t.ctr, gone && lane == 0, true);
}

// ------------------------------------------------------------------ lookup
// One wave a key: count, max_local and the list (sc words, the tail NONE32); a grain with no set reads 0, 0, empty.
static __global__ void __launch_bounds__(WK_SET_NT) k_wk_lookup(const gd_key* __restrict__ keys, WkTab t,
                                                         uint32_t* __restrict__ out_count,
                                                         uint32_t* __restrict__ out_max_local,
                                                         uint32_t* __restrict__ out_list) {
    const unsigned long long i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint64_t tcd = keys[i].type_code_data;
    uint32_t s = NONE32;
    uint4 b;
    if ((uint32_t)(tcd >> 56) == CAT_GRAIN) s = find_slot(t.slots, t.mask, t.ctr->max_probe, keys[i].n0, keys[i].n1, tcd, b);
    const uint32_t* sd = s != NONE32 ? wk_set(t, s) : nullptr;
    const uint32_t c = sd ? min(sd[0], t.sc) : 0u;
    if (lane == 0) {
        if (out_count) out_count[i] = c;
        if (out_max_local) out_max_local[i] = sd ? sd[1] : 0u;
    }
    if (out_list)
        for (uint32_t j = lane; j < t.sc; j += WAVE) out_list[i * t.sc + j] = j < c ? sd[WK_HDR + j] : NONE32;
}

// ------------------------------------------------------------------ rebuild
// Every live set of the old table, with its words and list, into the new, zeroed one.
static __global__ void __launch_bounds__(BLOCK) k_wk_rehash(const Slot* __restrict__ old_slots,
                                                     const uint32_t* __restrict__ old_side,
                                                     unsigned long long old_cap, WkTab t) {
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pd = 0;
    bool placed = false;
    const Slot sl = j < old_cap ? old_slots[j] : Slot{};
    if (j < old_cap && slot_state(sl.meta) == SLOT_LIVE) {
        const uint32_t* from = old_side + j * (unsigned long long)(WK_HDR + t.sc);
        const uint32_t words = WK_HDR + min(from[0], t.sc);
        const uint32_t d = rehash_place(DirSlots{t.slots, t.mask}, gd_key{sl.n0, sl.n1, sl.tcd}, sl.meta,
                                        [&](unsigned long long s) {
                                            t.slots[s].act = sl.act;
                                            uint32_t* to = wk_set(t, s);
                                            for (uint32_t q = 0; q < words; ++q) to[q] = from[q];
                                        });
        placed = d != NONE32;
        if (placed) pd = d;
        else atomicOr(&t.ctr->err, WK_ERR_FULL);
    }
    claim_counters(t.ctr, pd, false);
    live_delta(t.ctr, placed, false);
}

}  // namespace gd
