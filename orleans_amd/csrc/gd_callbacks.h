// gd_callbacks.h -- gfx950 device code of the callback table: InsideRuntimeClient's `callbacks`
// dictionary, CorrelationId -> CallbackData, as one open-addressing table in HBM.  SendRequestMessage's TryAdd
// (InsideRuntimeClient.cs:205-218), ReceiveResponse -> CallbackData.DoCallback (:569-627, CallbackData.cs:126-157),
// the response timers (CallbackData.cs:69-109,179-212) and BreakOutstandingMessagesToDeadSilo (:726-735).
//
// The table.  One 16-B slot an entry {id i64, handle u32, meta u32}; meta = state:8 | resend count:8 | target silo:16
// (0xFFFF = none).  The deadlines are an int64 array of their own, slot for slot, which only the timer scan reads.
// Capacity is a power of two >= CB_GROUP; a key's home is the first slot of an aligned group of CB_GROUP = 4 slots
// (one 64-B atom), group = mulhi(mix64(id), groups) -- CorrelationIds come from a counter, so their low bits are
// not a hash; chains run linearly from there and wrap.  A read-only probe (cb_find) reads one whole group a round.
//
// States, claims and elections are gd_dirbatch.h's: EMPTY ends a chain, TOMB keeps it going and is the first
// choice of an add, CLAIMED / PENDING exist only inside an add, and the `~i` first-wins word (one per slot) both
// names a fresh claim's claimer and elects the batch item that commits.  The add and the rebuild run that
// header's claim_walk and rehash_place over CbSlots, this table's policy: the 8-B key, cb_home, cb_meta.
//
// respond.  Ids do not interact, so a batch is the sequential loop once each id's own responses are ordered.
// Among an id's responses that reach the table (not gatewayed back, not masked by `turn`) and find the entry at
// the batch start, with k = max(max_resend_count - resend_count, 0): f = min(rank of the first that is not a
// transient rejection, k); rank < f: RESEND, rank == f: FIRE, rank > f: NO_CALLBACK.  The kernels reach it by
// rounds: every unresolved item votes atomicMax(~i) on its slot's word, the elected (lowest) one resolves --
// resend: count + 1, target none; fire: the slot becomes a tombstone -- and the others see the tombstone (all
// NO_CALLBACK at once) or vote again on the slot's second word (two words a slot, alternating by round, so a
// round's votes never meet the previous winner's clearing store).  max_resend_count == 0: one round, losers are
// NO_CALLBACK at once.  Rounds needed: at most k + 2.
//
// Launches:
//   add          k_cb_claim pass 0, passes 1.. (read-back driven, or CB_PASSES - 1 gated ones), k_cb_commit (elects,
//                writes handle / deadline / LIVE, reports out_added)
//   lookup       k_cb_find
//   set_target   k_cb_find (last wins: atomicMax(1 + i)), k_cb_set_target
//   respond      k_cb_find_resp (rules 1-3, round 0's votes), k_cb_resolve rounds, [k_cb_fire_count, scan_device,
//                k_cb_fire_list]
//   expire / break_silo   k_cb_scan_mark, scan_device, k_cb_scan_emit (applies only if the count fits `cap`)
//   rebuild      k_cb_rebuild into a zeroed table
// Every store is a plain vector store or a device-scope atomic.  Tile shapes (256 threads, one item a thread; the
// fire list 4,096 bytes a workgroup as k_turn_starts) are the neighbouring kernels'; alternatives were not measured.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "gd_common.h"
#include "gd_dirbatch.h"
#include "gd_place.h"
#include "graindispatch.h"

namespace gd {

struct alignas(16) CbSlot {
    int64_t id;
    uint32_t handle;
    uint32_t meta;      // state:8 | resend:8 | silo:16
};
static_assert(sizeof(CbSlot) == 16, "callback slot must be 16 bytes");

constexpr uint32_t CB_GROUP = 4;                 // slots a probe round: one 64-B atom
constexpr uint32_t CB_SILO_NONE = 0xFFFFu;
constexpr uint32_t CB_PASSES = REG_PASSES;       // add: claim passes of the device form
constexpr uint32_t CB_ROUNDS = 8;                // respond: resolve rounds of the device form
constexpr uint32_t CB_ERR_FULL = 2u, CB_ERR_SILO = 4u;   // CbCounters::err bits (+ ERR_UNSETTLED)

// live / tomb are kept as striped deltas, 64 B apart: a wave adds its count into stripe blockIdx % CB_STRIPES
// (one word from every XCD serialised: 16M adds spent 3 ms of k_cb_commit on it), the host sums the stripes of a
// read-back.
constexpr uint32_t CB_STRIPES = 64;
constexpr uint32_t CB_STRIPE_U32 = 16;
struct CbCounters {
    uint32_t err, pad[3];
    uint32_t retry[CB_PASSES];       // add: items pass p deferred
    uint32_t unres[CB_ROUNDS];       // respond: items round r left unresolved
    uint32_t pad2[8];
    uint32_t stripe[CB_STRIPES][CB_STRIPE_U32];   // [k][0] live delta, [k][1] tomb delta (mod 2^32)
};
static_assert(offsetof(CbCounters, stripe) % 64 == 0, "stripes start a 64-B line");

GD_HD uint32_t cb_state(uint32_t m) { return m >> 24; }
GD_HD uint32_t cb_resend(uint32_t m) { return (m >> 16) & 0xFFu; }
GD_HD uint32_t cb_silo(uint32_t m) { return m & 0xFFFFu; }
GD_HD uint32_t cb_meta(uint32_t state, uint32_t resend, uint32_t silo) {
    return (state << 24) | ((resend & 0xFFu) << 16) | (silo & 0xFFFFu);
}
// the ABI's silo (0xFFFFFFFF = none) <-> the 16-bit field
GD_HD uint32_t cb_silo_in(uint32_t s) { return s == 0xFFFFFFFFu ? CB_SILO_NONE : s; }
GD_HD uint32_t cb_silo_out(uint32_t s) { return s == CB_SILO_NONE ? 0xFFFFFFFFu : s; }

// splitmix64's finalizer: every input bit reaches the top bits the multiply-shift keeps
GD_HD uint64_t cb_mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}
__device__ __forceinline__ unsigned long long cb_home(int64_t id, unsigned long long mask) {
    return __umul64hi(cb_mix64((uint64_t)id), (mask + 1ull) / CB_GROUP) * CB_GROUP;
}

struct CbTab {
    CbSlot* slots;
    int64_t* deadline;
    unsigned long long mask;
    CbCounters* ctr;
};

// The live slot of `id`, or NONE32: one 64-B group a round.  For kernels that do not change the table's states.
__device__ __forceinline__ uint32_t cb_find(const CbSlot* __restrict__ slots, unsigned long long mask, int64_t id) {
    const unsigned long long groups = (mask + 1ull) / CB_GROUP;
    unsigned long long s = cb_home(id, mask);
    for (unsigned long long r = 0; r < groups; ++r) {
        const uint4* p = reinterpret_cast<const uint4*>(slots + s);
        uint4 q[CB_GROUP];
#pragma unroll
        for (uint32_t k = 0; k < CB_GROUP; ++k) q[k] = p[k];
#pragma unroll
        for (uint32_t k = 0; k < CB_GROUP; ++k) {
            const uint32_t st = cb_state(q[k].w);
            if (st == SLOT_EMPTY) return NONE32;
            if (st == SLOT_LIVE && (int64_t)((uint64_t)q[k].x | ((uint64_t)q[k].y << 32)) == id) return (uint32_t)(s + k);
        }
        s = (s + CB_GROUP) & mask;
    }
    return NONE32;
}

// live / tomb deltas of the wave's flagged lanes, one atomic a word a wave.  Every lane of the wave calls it.
__device__ __forceinline__ void cb_count(CbCounters* ctr, bool flag, int live_d, int tomb_d) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & (WAVE - 1)) != 0 || !m) return;
    const uint32_t c = (uint32_t)__popcll(m);
    uint32_t* st = ctr->stripe[blockIdx.x % CB_STRIPES];
    if (live_d) atomicAdd(st, live_d > 0 ? c : 0u - c);
    if (tomb_d) atomicAdd(st + 1, tomb_d > 0 ? c : 0u - c);
}

// ------------------------------------------------------------------ add
// The table to claim_walk and rehash_place (gd_dirbatch.h, DirSlots); PENDING's tag lies in the silo field.
struct CbSlots {
    using Key = int64_t;
    CbSlot* slots;
    unsigned long long mask;
    __device__ __forceinline__ unsigned long long home(int64_t id) const { return cb_home(id, mask); }
    __device__ __forceinline__ uint32_t* meta(unsigned long long s) const { return &slots[s].meta; }
    static __device__ __forceinline__ uint32_t state(uint32_t meta) { return cb_state(meta); }
    static __device__ __forceinline__ uint32_t tag(uint32_t meta) { return cb_silo(meta); }
    static __device__ __forceinline__ uint32_t claimed() { return cb_meta(SLOT_CLAIMED, 0, 0); }
    static __device__ __forceinline__ uint32_t pending(uint32_t tag) { return cb_meta(SLOT_PENDING, 0, tag); }
    __device__ __forceinline__ void put(unsigned long long s, int64_t id) const {
        slots[s].id = id;
        slots[s].handle = NONE32;
    }
    __device__ __forceinline__ bool holds(unsigned long long s, int64_t id) const { return slots[s].id == id; }
    static __device__ __forceinline__ bool same(int64_t a, int64_t b) { return a == b; }
};
static_assert(CB_ERR_FULL == 2u, "claim_walk's table-full bit");

// Pass 0: every item; pass p >= 1: the items pass p - 1 deferred, and only if it deferred any (gate = its count;
// null: the host read it).  Counts its own deferred items into retry[pass % CB_PASSES], zeroed by the host.
static __global__ void __launch_bounds__(BLOCK) k_cb_claim(const int64_t* __restrict__ ids, uint32_t n, CbTab tab,
                                                    uint32_t* __restrict__ slot_of, uint8_t* __restrict__ is_new,
                                                    uint32_t pass, const uint32_t* __restrict__ gate,
                                                    uint32_t* __restrict__ last) {
    if (gate && *gate == 0) return;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool reused = false;
    if (i < n && (pass == 0 || slot_of[i] == SLOT_RETRY)) {
        uint32_t pd = 0;                                     // this table keeps no max_probe
        const bool claimed = claim_walk(CbSlots{tab.slots, tab.mask}, i, ids, &tab.ctr->err, slot_of, is_new,
                                        &tab.ctr->retry[pass % CB_PASSES], pd, reused, claim_tag(pass), last);
        // the election (k_cb_commit); a claimer voted when it claimed
        if (is_new[i] && !claimed) atomicMax(&last[slot_of[i]], ~i);
    }
    cb_count(tab.ctr, reused, 0, -1);
}

// The elected item of each new entry (it holds the slot's word) publishes it and clears the word; out_added.
// unsettled (device form): the last gated pass's count.
static __global__ void __launch_bounds__(BLOCK) k_cb_commit(const uint32_t* __restrict__ handles,
                                                     const int64_t* __restrict__ deadlines, uint32_t n, CbTab tab,
                                                     const uint32_t* __restrict__ slot_of,
                                                     const uint8_t* __restrict__ is_new, uint32_t* __restrict__ last,
                                                     const uint32_t* __restrict__ unsettled,
                                                     uint8_t* __restrict__ out_added) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0 && unsettled && *unsettled) atomicOr(&tab.ctr->err, ERR_UNSETTLED);
    bool w = false;
    if (i < n) {
        const uint32_t s = slot_of[i];
        if (is_new[i] && s < SLOT_RETRY) {
            w = last[s] == ~i;
            if (w) {
                last[s] = 0;                                 // losers read ~winner or 0: never their own
                tab.slots[s].handle = handles[i];
                tab.deadline[s] = deadlines[i];
                tab.slots[s].meta = cb_meta(SLOT_LIVE, 0, CB_SILO_NONE);   // not addressed yet, ResendCount 0
            }
        }
        if (out_added) out_added[i] = w ? 1 : 0;
    }
    cb_count(tab.ctr, w, 1, 0);
}

// ------------------------------------------------------------------ lookup, set_target
// slot_of (optional) and the lookup outputs (each optional); last_wins (set_target): atomicMax(1 + i) on the
// found slot's word.
static __global__ void __launch_bounds__(BLOCK) k_cb_find(const int64_t* __restrict__ ids, uint32_t n, CbTab tab,
                                                   uint32_t* __restrict__ slot_of, uint32_t* __restrict__ last_wins,
                                                   uint32_t* __restrict__ out_handle, uint32_t* __restrict__ out_resend,
                                                   uint32_t* __restrict__ out_silo, uint8_t* __restrict__ out_found) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = cb_find(tab.slots, tab.mask, ids[i]);
    if (slot_of) slot_of[i] = s;
    if (last_wins && s != NONE32) atomicMax(&last_wins[s], i + 1u);
    uint32_t handle = NONE32, meta = cb_meta(SLOT_EMPTY, 0, CB_SILO_NONE);
    if (s != NONE32 && (out_handle || out_resend || out_silo)) {
        handle = tab.slots[s].handle;
        meta = tab.slots[s].meta;
    }
    if (out_handle) out_handle[i] = handle;
    if (out_resend) out_resend[i] = cb_resend(meta);
    if (out_silo) out_silo[i] = cb_silo_out(cb_silo(meta));
    if (out_found) out_found[i] = s != NONE32 ? 1 : 0;
}

static __global__ void __launch_bounds__(BLOCK) k_cb_set_target(const uint32_t* __restrict__ silo, uint32_t n,
                                                         CbTab tab, const uint32_t* __restrict__ slot_of,
                                                         uint32_t* __restrict__ last) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slot_of[i];
    if (s == NONE32 || last[s] != i + 1u) return;
    last[s] = 0;
    uint32_t v = silo[i];
    if (v != 0xFFFFFFFFu && v >= CB_SILO_NONE) {
        atomicOr(&tab.ctr->err, CB_ERR_SILO);                // silo index above 0xFFFE
        v = 0xFFFFFFFFu;
    }
    const uint32_t m = tab.slots[s].meta;
    tab.slots[s].meta = cb_meta(SLOT_LIVE, cb_resend(m), cb_silo_in(v));
}

// ------------------------------------------------------------------ respond
constexpr uint8_t CB_CLS_DONE = 0, CB_CLS_TRANSIENT = 1, CB_CLS_OTHER = 2;

struct CbResp {
    const int64_t* ids;
    const uint8_t *result, *rejection, *flags, *turn;    // each nullable
    uint8_t *outcome, *oflags;
    uint32_t* handle;
};

// Rules 1-3 (InsideRuntimeClient.cs:571-600,610,622-626) and round 0's votes.
static __global__ void __launch_bounds__(BLOCK) k_cb_find_resp(CbResp a, uint32_t n, CbTab tab,
                                                        uint32_t* __restrict__ slot_of, uint8_t* __restrict__ cls,
                                                        uint32_t* __restrict__ word) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t id = a.ids[i];
    const uint32_t res = a.result ? a.result[i] : 0u;
    const bool rej = res == 2u;
    const uint32_t rt = rej && a.rejection ? a.rejection[i] : 0u;
    const uint32_t fl = a.flags ? a.flags[i] : 0u;
    const bool part = !a.turn || a.turn[i] == GD_TURN_RESPONSE;
    uint32_t outcome = GD_CB_NONE, of = 0, s = NONE32;
    uint8_t c = CB_CLS_DONE;
    if (part) {
        if (rej && (fl & GD_RESP_TARGET_NOT_ME)) {
            outcome = GD_CB_GATEWAY_BACK;
        } else {
            if (rej && (rt == 0u || rt == 3u) && !(fl & GD_RESP_HAS_CACHE_HEADER)) of = GD_CB_INVALIDATE_CACHE;
            s = cb_find(tab.slots, tab.mask, id);
            if (s == NONE32) {
                outcome = GD_CB_NO_CALLBACK;
            } else {
                c = rej && rt == 0u ? CB_CLS_TRANSIENT : CB_CLS_OTHER;
                atomicMax(&word[s], ~i);
            }
        }
    }
    a.outcome[i] = (uint8_t)outcome;
    a.oflags[i] = (uint8_t)of;
    a.handle[i] = NONE32;
    slot_of[i] = s;
    cls[i] = c;
}

// One round: the elected item of each slot (the lowest unresolved index) resolves by rules 4-5
// (CallbackData.cs:135-149, Dispatcher.cs:581-589); the others find the slot fired (NO_CALLBACK) or vote on
// `next`.  gate (nullable): the previous round's unresolved count; unres: this round's.
static __global__ void __launch_bounds__(BLOCK) k_cb_resolve(CbResp a, uint32_t n, CbTab tab,
                                                      const uint32_t* __restrict__ slot_of, uint8_t* __restrict__ cls,
                                                      uint32_t* __restrict__ cur, uint32_t* __restrict__ next,
                                                      uint32_t max_resend, const uint32_t* __restrict__ gate,
                                                      uint32_t* __restrict__ unres) {
    if (gate && *gate == 0) return;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool fired = false, pending = false;
    const uint8_t c = i < n ? cls[i] : CB_CLS_DONE;
    if (c != CB_CLS_DONE) {
        const uint32_t s = slot_of[i];
        CbSlot* sl = tab.slots + s;
        const uint32_t meta = __hip_atomic_load(&sl->meta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool live = cb_state(meta) == SLOT_LIVE;
        uint32_t outcome = GD_CB_NO_CALLBACK;                // the entry fired in an earlier round
        if (cur[s] == ~i) {
            cur[s] = 0;                                      // the others read ~i or 0: never their own
            if (live) {
                a.handle[i] = sl->handle;
                if (c == CB_CLS_TRANSIENT && cb_resend(meta) < max_resend) {
                    outcome = GD_CB_RESEND;                  // MayResend: ResendCount + 1, the target cleared
                    __hip_atomic_store(&sl->meta, cb_meta(SLOT_LIVE, cb_resend(meta) + 1u, CB_SILO_NONE),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    outcome = GD_CB_FIRE;                    // alreadyFired, unregister
                    __hip_atomic_store(&sl->meta, cb_meta(SLOT_TOMB, 0, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    fired = true;
                }
            }
        } else if (live && max_resend != 0u) {
            atomicMax(&next[s], ~i);                         // an earlier response of the id is still ahead
            pending = true;
        }                                                    // max_resend 0: the elected one fires
        if (!pending) {
            a.outcome[i] = (uint8_t)outcome;
            cls[i] = CB_CLS_DONE;
        }
    }
    count_deferred(unres, pending);
    cb_count(tab.ctr, fired, -1, 1);
}

// The device form ran fewer rounds than max_resend_count + 2 could need: a batch still unresolved is flagged.
static __global__ void __launch_bounds__(WAVE) k_cb_settled(CbCounters* ctr, uint32_t round) {
    if (threadIdx.x == 0 && ctr->unres[round]) atomicOr(&ctr->err, ERR_UNSETTLED);
}

// fire_idx: the stable compaction of the FIRE outcomes, as k_turn_starts (thread t of tile b holds bytes
// b * PL_TILE + t * PL_IT + 0 .. 15).  tile_cnt[tiles] = 0: the scan's total lands there.
static __global__ void __launch_bounds__(PL_NT) k_cb_fire_count(const uint8_t* __restrict__ outcome, uint32_t n,
                                                         uint32_t wide, uint32_t* __restrict__ tile_cnt,
                                                         uint32_t tiles) {
    __shared__ uint32_t s_wcnt[PL_NW];
    const uint32_t i0 = blockIdx.x * PL_TILE + threadIdx.x * PL_IT;
    uint32_t w[4];
    pl_load16(outcome, i0, n, wide != 0, (uint32_t)GD_CB_NONE, w);
    uint32_t total;
    (void)pl_wave_prefix((uint32_t)__popc(pl_eq_mask(w, GD_CB_FIRE)), lane_id(), total);
    if (lane_id() == 0) s_wcnt[threadIdx.x / WAVE] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int k = 0; k < PL_NW; ++k) t += s_wcnt[k];
        tile_cnt[blockIdx.x] = t;
        if (blockIdx.x == 0) tile_cnt[tiles] = 0;
    }
}
static __global__ void __launch_bounds__(PL_NT) k_cb_fire_list(const uint8_t* __restrict__ outcome, uint32_t n,
                                                        uint32_t wide, const uint32_t* __restrict__ tile_off,
                                                        uint32_t tiles, uint32_t* __restrict__ fire_idx,
                                                        uint32_t* __restrict__ n_fire) {
    __shared__ uint32_t s_wcnt[PL_NW];
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_fire = tile_off[tiles];
    const uint32_t tile_base = tile_off[blockIdx.x];
    if (tile_off[blockIdx.x + 1] == tile_base) return;      // the whole workgroup
    const uint32_t i0 = blockIdx.x * PL_TILE + threadIdx.x * PL_IT;
    uint32_t w[4];
    pl_load16(outcome, i0, n, wide != 0, (uint32_t)GD_CB_NONE, w);
    uint32_t m = pl_eq_mask(w, GD_CB_FIRE);
    const uint32_t lane = lane_id(), wv = threadIdx.x / WAVE;
    uint32_t total;
    const uint32_t pre = pl_wave_prefix((uint32_t)__popc(m), lane, total);
    if (lane == 0) s_wcnt[wv] = total;
    __syncthreads();
    uint32_t j = tile_base + pre;
#pragma unroll
    for (int k = 0; k < PL_NW; ++k)
        if ((uint32_t)k < wv) j += s_wcnt[k];
    for (; m; m &= m - 1u, ++j)
        if (j < n) fire_idx[j] = i0 + ((uint32_t)__ffs((int)m) - 1u);
}

// ------------------------------------------------------------------ expire, break_silo
struct CbScan {
    uint32_t by_silo;            // 0: deadline <= now (expire); 1: target silo == silo (break_silo)
    int64_t now;
    uint32_t silo;               // 16-bit field value
    uint32_t max_resend, resend_on_timeout;
    int64_t period;
};
__device__ __forceinline__ bool cb_scan_pred(const CbScan& a, uint32_t meta, const int64_t* deadline,
                                             unsigned long long j) {
    if (cb_state(meta) != SLOT_LIVE) return false;
    return a.by_silo ? cb_silo(meta) == a.silo : deadline[j] <= a.now;
}
// flag[j] = the slot is due; flag[cap] = 0 (the scan's total lands there)
static __global__ void __launch_bounds__(BLOCK) k_cb_scan_mark(CbTab tab, CbScan a, uint32_t* __restrict__ flag) {
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j > tab.mask + 1ull) return;
    flag[j] = j <= tab.mask && cb_scan_pred(a, tab.slots[j].meta, tab.deadline, j) ? 1u : 0u;
}
// pos: the exclusive scan of the flags.  *n_out = the due entries; they are applied and listed only if they fit
// `cap` (CallbackData.OnFail: ResendOnTimeout && resendFunc -> resend, else alreadyFired / unregister).
static __global__ void __launch_bounds__(BLOCK) k_cb_scan_emit(CbTab tab, CbScan a, const uint32_t* __restrict__ pos,
                                                        uint32_t cap, int64_t* __restrict__ out_id,
                                                        uint32_t* __restrict__ out_handle,
                                                        uint8_t* __restrict__ out_kind, uint32_t* __restrict__ n_out) {
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t total = pos[tab.mask + 1ull];
    if (j == 0) *n_out = total;
    bool removed = false;
    if (total <= cap && j <= tab.mask && pos[j + 1] != pos[j]) {
        CbSlot* sl = tab.slots + j;
        const uint32_t meta = sl->meta, p = pos[j];
        uint32_t kind;
        if (a.resend_on_timeout && cb_resend(meta) < a.max_resend) {
            kind = GD_CB_RESEND;
            sl->meta = cb_meta(SLOT_LIVE, cb_resend(meta) + 1u, CB_SILO_NONE);
            if (!a.by_silo) tab.deadline[j] += a.period;     // the timer's repeat period
        } else {
            kind = a.by_silo ? GD_CB_SILO_FAILED : GD_CB_TIMEOUT;
            sl->meta = cb_meta(SLOT_TOMB, 0, 0);
            removed = true;
        }
        out_id[p] = sl->id;
        out_handle[p] = sl->handle;
        out_kind[p] = (uint8_t)kind;
    }
    cb_count(tab.ctr, removed, -1, 1);
}

// ------------------------------------------------------------------ rebuild
// Every live entry of the old table into the new, zeroed one.
static __global__ void __launch_bounds__(BLOCK) k_cb_rebuild(const CbSlot* __restrict__ old_slots,
                                                      const int64_t* __restrict__ old_deadline,
                                                      unsigned long long old_cap, CbTab tab) {
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= old_cap) return;
    const CbSlot sl = old_slots[j];
    if (cb_state(sl.meta) != SLOT_LIVE) return;
    const uint32_t d = rehash_place(CbSlots{tab.slots, tab.mask}, sl.id, sl.meta, [&](unsigned long long s) {
        tab.slots[s].handle = sl.handle;
        tab.deadline[s] = old_deadline[j];
    });
    if (d == NONE32) atomicOr(&tab.ctr->err, CB_ERR_FULL);
}

}  // namespace gd
