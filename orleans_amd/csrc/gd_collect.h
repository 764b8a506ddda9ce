// gd_collect.h -- gfx950 device code for the activation collector: Catalog/ActivationCollector.cs
// over per-context arrays -- ticket, becameIdle and a flag byte a context, quantum and nextTicket on the handle.
// The rules, step by step: include/graindispatch.h.  Context c is in bucket ticket[c] iff ticket[c] != 0 &&
// !(flags[c] & GD_COL_CANCELLED) && ticket[c] >= nextTicket: that predicate is all that is left of the reference's
// dictionary of dictionaries.
//
// List forms (one lane an item):
//   schedule   k_col_elect (atomicMin of the item index on the context's election word, gd_dirbatch.h's means),
//              k_col_schedule (the winner applies ScheduleCollection), k_col_schedule_dup (a later occurrence reads
//              the winner's status), k_col_unelect (the words back to NONE32: they are clean between calls)
//   cancel     k_col_elect, k_col_cancel, k_col_unelect
//   touch      k_col_touch alone: at one `now` TryRescheduleCollection is idempotent on a context -- the only word it
//              writes is the ticket, to 0 or to roundup(now + age), and a lane that reads either value gives the
//              answer the first occurrence gave -- so duplicates race benignly and no election is needed.
// Dense forms (streaming over n_ctx; only due or touched lanes read past the first array):
//   idle       k_col_idle: the event byte, then the ticket of an idle context
//   scans      k_col_scan<ALL>: tiles of COL_TILE contexts, a wave row = 64 consecutive contexts (512 B of tickets),
//              the COL_IT ticket loads of a lane in flight together; verdict bytes dense, the condemned counted by
//              ballots into a count a tile.  scan_device over the counts, then k_col_list writes the condemned in
//              context order (ballot ranks inside a wave row, rows and waves in order).  ScanStale over more than one
//              quantum orders by ticket first: the scan also writes a key a context (the quantum index, n_q for a
//              context that is not condemned) and the stable bucketing of those keys is the list.
//   count      k_col_count: one 64-bit atomic a workgroup
// COL_NT / COL_IT are the pump's and the turn stage's tile (4096); alternatives were not measured.
// Every store is a plain vector store.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_common.h"
#include "gd_hash.h"
#include "gd_scan.h"
#include "graindispatch.h"

namespace gd {

constexpr int COL_NT = 256;
constexpr int COL_IT = 16;
constexpr int COL_NW = COL_NT / WAVE;
constexpr uint32_t COL_TILE = COL_NT * COL_IT;       // 4096 contexts per workgroup

struct ColArgs {
    int64_t* ticket;
    int64_t* became_idle;
    const int64_t* keep_alive;      // null: never
    const int64_t* age;
    uint8_t* flags;
    int64_t quantum, next, now;     // next: nextTicket as the call starts
    uint32_t n_ctx;
};

// MakeTicketFromDateTime's rounding (:371)
__device__ __forceinline__ int64_t col_roundup(int64_t t, int64_t q) { return ((t - 1) / q + 1) * q; }

// ScheduleCollection (:83-108) on a context's words in registers; `next` is the nextTicket :372 compares with.
__device__ __forceinline__ uint32_t col_schedule(int64_t& ticket, uint32_t& fl, int64_t age, int64_t now, int64_t q,
                                                 int64_t next) {
    if (fl & GD_COL_EXEMPT) return GD_COL_SKIPPED_EXEMPT;
    if (age == 0) return GD_COL_SKIPPED_NO_LIMIT;
    if (age < q) return GD_COL_THROWS_TIMEOUT;
    const int64_t t = col_roundup(now + age, q);
    if (t < next) return GD_COL_THROWS_EARLY;
    if (ticket != 0) return GD_COL_THROWS_TICKETED;
    ticket = t;
    fl &= ~GD_COL_CANCELLED;
    return GD_COL_SCHEDULED;
}

// TryRescheduleCollection (:128-164) on context c.  The exempt test comes first in the reference; a zero ticket
// gives the same answer and the same state either way, so the ticket alone is read for most contexts.
__device__ __forceinline__ uint32_t col_reschedule(const ColArgs& a, uint32_t c) {
    const int64_t t = a.ticket[c];
    if (t == 0) return GD_COL_FALSE;
    const uint32_t fl = a.flags[c];
    if (fl & GD_COL_EXEMPT) return GD_COL_FALSE;
    if (t % a.quantum != 0) return GD_COL_THROWS;
    if (t < a.next) {
        a.ticket[c] = 0;
        return GD_COL_FALSE;
    }
    const int64_t age = a.age[c];
    if (age < a.quantum) return GD_COL_THROWS;
    const int64_t nt = col_roundup(a.now + age, a.quantum);
    if (nt < a.next) return GD_COL_THROWS;
    if (nt == t) return GD_COL_TRUE;
    if (fl & GD_COL_CANCELLED) {
        a.ticket[c] = 0;
        return GD_COL_FALSE;
    }
    a.ticket[c] = nt;
    return GD_COL_TRUE;
}

// ---- list forms --------------------------------------------------------------------------------
static __global__ void __launch_bounds__(BLOCK) k_col_elect(const uint32_t* __restrict__ ctx, uint32_t n, uint32_t n_ctx,
                                                     uint32_t* __restrict__ win) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = ctx[i];
    if (c < n_ctx) atomicMin(&win[c], i);
}

static __global__ void __launch_bounds__(BLOCK) k_col_unelect(const uint32_t* __restrict__ ctx, uint32_t n,
                                                       uint32_t n_ctx, uint32_t* __restrict__ win) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = ctx[i];
    if (c < n_ctx) win[c] = NONE32;
}

static __global__ void __launch_bounds__(BLOCK) k_col_schedule(ColArgs a, const uint32_t* __restrict__ ctx, uint32_t n,
                                                        const uint32_t* __restrict__ win,
                                                        uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = ctx[i];
    if (c >= a.n_ctx) {
        if (status) status[i] = GD_COL_OUT_OF_RANGE;
        return;
    }
    if (win[c] != i) return;
    int64_t t = a.ticket[c];
    uint32_t fl = a.flags[c];
    const uint32_t st = col_schedule(t, fl, a.age[c], a.now, a.quantum, a.next);
    if (st == GD_COL_SCHEDULED) {
        a.ticket[c] = t;
        a.flags[c] = (uint8_t)fl;
    }
    if (status) status[i] = (uint8_t)st;
}

static __global__ void __launch_bounds__(BLOCK) k_col_schedule_dup(const uint32_t* __restrict__ ctx, uint32_t n,
                                                            uint32_t n_ctx, const uint32_t* __restrict__ win,
                                                            uint8_t* status) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = ctx[i];
    if (c >= n_ctx) return;
    const uint32_t w = win[c];
    if (w == i || w >= n) return;
    const uint32_t s = status[w];                       // a winner's byte: written by the launch before, not by this one
    status[i] = (uint8_t)(s == GD_COL_SCHEDULED ? GD_COL_THROWS_TICKETED : s);
}

static __global__ void __launch_bounds__(BLOCK) k_col_cancel(ColArgs a, const uint32_t* __restrict__ ctx, uint32_t n,
                                                      const uint32_t* __restrict__ win, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = ctx[i];
    uint32_t r = 0;
    if (c < a.n_ctx && win[c] == i) {
        const uint32_t fl = a.flags[c];
        const int64_t t = a.ticket[c];
        r = !(fl & GD_COL_EXEMPT) && t != 0 && t >= a.next && !(fl & GD_COL_CANCELLED);
        if (r) a.flags[c] = (uint8_t)(fl | GD_COL_CANCELLED);
    }
    if (out) out[i] = (uint8_t)r;
}

__device__ __forceinline__ bool col_turn_takes_part(uint32_t t) { return t >= GD_TURN_START && t <= GD_TURN_REJECT_TRANSIENT; }
static_assert(GD_TURN_START == 1 && GD_TURN_WAIT == 2 && GD_TURN_REJECT_OVERLOADED == 3 && GD_TURN_STUCK == 4 &&
                  GD_TURN_FORWARD == 5 && GD_TURN_REJECT_TRANSIENT == 6,
              "the turn bytes of a Request / OneWay that reached ReceiveRequest are 1 .. 6");

static __global__ void __launch_bounds__(BLOCK) k_col_touch(ColArgs a, const uint8_t* __restrict__ ctx_flags,
                                                     const uint32_t* __restrict__ ctx, const uint8_t* __restrict__ turn,
                                                     uint32_t n, uint8_t* __restrict__ ok) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t c = ctx[i];
        uint32_t r = GD_COL_NO_PART;
        if (c < a.n_ctx && (!turn || col_turn_takes_part(turn[i])) && (ctx_flags[c] & GD_CTX_STATE_MASK) == GD_CTX_VALID)
            r = col_reschedule(a, c);
        if (ok) ok[i] = (uint8_t)r;
    }
}

// ---- dense forms -------------------------------------------------------------------------------
static __global__ void __launch_bounds__(BLOCK) k_col_idle(ColArgs a, const uint8_t* __restrict__ event,
                                                    uint8_t* __restrict__ ok) {
    for (uint64_t c = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; c < a.n_ctx; c += (uint64_t)gridDim.x * BLOCK) {
        uint32_t r = GD_COL_NO_PART;
        if (event[c] & GD_PUMP_BECAME_IDLE) {
            a.became_idle[c] = a.now;
            r = col_reschedule(a, (uint32_t)c);
        }
        if (ok) ok[c] = (uint8_t)r;
    }
}

struct ColScan {
    uint8_t* ctx_flags;
    const uint32_t* num_running;
    const uint32_t* woff;           // null: no waiting lists
    int64_t next1;                  // ScanStale: nextTicket after the dequeues
    int64_t age_all;                // ScanAll's age limit
    uint32_t n_q;
    uint8_t* verdict;               // [n_ctx], dense
    uint32_t* qkey;                 // [n_ctx] or null: the quantum index of a condemned context, else n_q
};

// Item (w, r, lane) of a tile <-> context base + (w * COL_IT + r) * 64 + lane.  tile_cnt[tile] = its condemned;
// tile_cnt[tiles] = 0 (the scan's total lands there).
template <bool ALL>
static __global__ void __launch_bounds__(COL_NT) k_col_scan(ColArgs a, ColScan s, uint32_t* __restrict__ tile_cnt,
                                                     uint32_t tiles) {
    __shared__ uint32_t s_w[COL_NW];
    const uint32_t lane = lane_id(), w = threadIdx.x / WAVE;
    const uint64_t base = (uint64_t)blockIdx.x * COL_TILE + (uint64_t)w * COL_IT * WAVE + lane;
    int64_t tv[COL_IT];
#pragma unroll
    for (int r = 0; r < COL_IT; ++r) {
        const uint64_t c = base + (uint32_t)r * WAVE;
        tv[r] = c < a.n_ctx ? a.ticket[c] : 0;
    }
    uint32_t cnt = 0;
#pragma unroll
    for (int r = 0; r < COL_IT; ++r) {
        const uint64_t c = base + (uint32_t)r * WAVE;
        const int64_t t = tv[r];
        uint32_t v = 0, key = s.n_q;
        if (c < a.n_ctx) {
            bool cand = t != 0 && t >= a.next;
            if (!ALL) cand = cand && t <= a.now && (t - a.next) % a.quantum == 0;
            uint32_t fl = cand ? (uint32_t)a.flags[c] : (uint32_t)GD_COL_CANCELLED;
            if (!(fl & GD_COL_CANCELLED)) {
                const uint32_t cf = s.ctx_flags[c];
                const int64_t age = a.age[c];
                if ((cf & GD_CTX_STATE_MASK) != GD_CTX_VALID) v = GD_COL_BAD_STATE;
                else if (a.keep_alive && a.keep_alive[c] >= a.now) v = GD_COL_KEPT_ALIVE;
                else if ((int32_t)s.num_running[c] > 0 || (s.woff && s.woff[c + 1] != s.woff[c])) v = GD_COL_ACTIVE;
                else if (a.now - a.became_idle[c] < (ALL ? s.age_all : age)) v = GD_COL_NOT_STALE;
                else v = GD_COL_COLLECT;
                int64_t t2 = ALL ? t : 0;
                if (!ALL || v == GD_COL_COLLECT) fl |= GD_COL_CANCELLED;
                if (v == GD_COL_COLLECT) {
                    s.ctx_flags[c] = (uint8_t)((cf & ~GD_CTX_STATE_MASK) | GD_CTX_NOT_READY);
                    if (!ALL) key = (uint32_t)((t - a.next) / a.quantum);
                } else if (!ALL && v != GD_COL_BAD_STATE) {
                    if (col_schedule(t2, fl, age, a.now, a.quantum, s.next1) != GD_COL_SCHEDULED) v |= GD_COL_NOT_ADDED;
                }
                if (!ALL) a.ticket[c] = t2;
                if (!ALL || v == GD_COL_COLLECT) a.flags[c] = (uint8_t)fl;
            }
            s.verdict[c] = (uint8_t)v;
            if (s.qkey) s.qkey[c] = key;
        }
        cnt += (uint32_t)__popcll(__ballot(v == GD_COL_COLLECT));
    }
    if (lane == 0) s_w[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < COL_NW; ++k) sum += s_w[k];
        tile_cnt[blockIdx.x] = sum;
        if (blockIdx.x == 0) tile_cnt[tiles] = 0;
    }
}

// The condemned in context order: tile_off = the exclusive scan of tile_cnt (tiles + 1 entries).
static __global__ void __launch_bounds__(COL_NT) k_col_list(const uint8_t* __restrict__ verdict, uint32_t n_ctx,
                                                     const uint32_t* __restrict__ tile_off, uint32_t tiles,
                                                     uint32_t* __restrict__ out_ctx, uint32_t* __restrict__ out_n) {
    __shared__ uint32_t s_w[COL_NW];
    if (blockIdx.x == 0 && threadIdx.x == 0) *out_n = tile_off[tiles];
    const uint32_t lane = lane_id(), w = threadIdx.x / WAVE;
    const uint64_t base = (uint64_t)blockIdx.x * COL_TILE + (uint64_t)w * COL_IT * WAVE + lane;
    unsigned long long m[COL_IT];
    uint32_t cnt = 0;
#pragma unroll
    for (int r = 0; r < COL_IT; ++r) {
        const uint64_t c = base + (uint32_t)r * WAVE;
        m[r] = __ballot(c < n_ctx && verdict[c] == GD_COL_COLLECT);
        cnt += (uint32_t)__popcll(m[r]);
    }
    if (lane == 0) s_w[w] = cnt;
    __syncthreads();
    uint32_t off = tile_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < COL_NW; ++k)
        if ((uint32_t)k < w) off += s_w[k];
#pragma unroll
    for (int r = 0; r < COL_IT; ++r) {
        if ((m[r] >> lane) & 1ull)
            out_ctx[off + (uint32_t)__popcll(m[r] & ((1ull << lane) - 1ull))] = (uint32_t)(base + (uint32_t)r * WAVE);
        off += (uint32_t)__popcll(m[r]);
    }
}

// *out_n = offsets[n_q]: the contexts the bucketing put before the trailing bucket
static __global__ void k_col_total(const uint32_t* __restrict__ offsets, uint32_t n_q, uint32_t* __restrict__ out_n) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out_n = offsets[n_q];
}

static __global__ void __launch_bounds__(BLOCK) k_col_count(ColArgs a, int64_t shortest, int64_t recency,
                                                     unsigned long long* __restrict__ out) {
    __shared__ uint32_t s_w[BLOCK / WAVE];
    uint32_t cnt = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; c < a.n_ctx; c += (uint64_t)gridDim.x * BLOCK) {
        const int64_t t = a.ticket[c];
        if (t == 0 || t < a.next) continue;
        if (shortest != 0 && shortest - (t - a.now) > recency) continue;
        if (!(a.flags[c] & GD_COL_CANCELLED)) ++cnt;
    }
    cnt = block_reduce<OpAdd>(cnt, s_w);
    if (threadIdx.x == 0 && cnt) atomicAdd(out, (unsigned long long)cnt);
}

}  // namespace gd
