// gd_dirbatch.h -- gfx950 device code for the batches that change a directory table: AddSingleActivation
// (GrainDirectoryPartition.cs:304-326, GrainInfo :110-124), AddActivation (upsert), Merge's claims,
// RemoveActivation (:335-363, Force), the ActivationDirectory's TryAdd / TryRemove, lookup and rehash.
//
// The protocol, in one place: the claim (claim_walk) and the rebuild's placement (rehash_place) are templates
// over a table policy, DirSlots here for every table of 32-B slots (the directory, the activation directory, the
// gateway's two) and CbSlots (gd_callbacks.h) for the callback table's 16-B slots.
//
// Slot states (gd_common.h, the meta's high half).  EMPTY ends a chain; TOMB keeps it going and is free
// for reuse; LIVE holds a published entry.  A claim turns the key's first free slot -- its chain's first
// tombstone, else the EMPTY slot ending it -- into CLAIMED with one CAS (the arbiter: a key is never placed
// twice), writes the key and then PENDING with the launch's tag in the silo field; the commit makes it
// LIVE.  CLAIMED never outlives its launch, PENDING never outlives its batch (a failed merge undoes its
// claims, k_reg_abort).  Every reader tests the state before the key, so a tombstone keeps its key words.
//
// claim_tag.  "Claimed in this launch" is read off the meta alone: CLAIMED, or PENDING carrying this
// launch's tag (claim_tag(pass); k_reg_find_take's claims carry 0).  The key of such a slot is not
// published to the launch's other items; a PENDING slot of an earlier launch had its key published by
// that launch's end.  So a claim needs no release fence (an agent-scope release writes the XCD's L2 back,
// per wave) and a walk no acquire loads (an agent-scope acquire invalidates it): metas are read and
// swapped with relaxed device-coherent atomics, keys with plain loads.
//
// The election word (`last`): one u32 per table slot, zero between batches, in one of two encodings.
//   ~i     first wins (register, unregister, the activation directory's add and remove): atomicMax(~i), so
//          the lowest batch index holds the word.  During the claims it also names a fresh slot's
//          claimer: an item that meets an unpublished claim reads keys[~word] and joins it (its twin)
//          or walks on (another key); only a word still zero defers the item to the next pass
//          (SLOT_RETRY, no waiting: the claimer may be a lane of the same wave).  The commit of the
//          elected item clears the word (reg_elected, unreg_elected_commit).
//   1 + i  last wins (upsert's k_up_last, the activation directory's set_flags; merge's duplicate check
//          k_dup_mark): atomicMax(1 + i); k_up_clear zeroes the batch's words afterwards.  These batches
//          run their claims with last = nullptr, where every item meeting an unpublished claim defers
//          (k new keys on one chain: k passes).
//
// retry counters.  DevCounters::retry counts the items a read-back-driven pass deferred; the host zeroes
// it before each pass (claim_passes).  An asynchronous batch counts into its own REG_PASSES words
// (gd_handle::reg_retry), zero at allocation: k_reg_find_take counts into word 0 and zeroes words
// 1 .. REG_PASSES-1, gated pass p counts into word p and runs only if word p - 1 is not zero,
// k_reg_commit_elect flags ERR_UNSETTLED if the last pass's word is not zero and zeroes word 0 for the
// next batch.
//
// Launches of a batch:
//   synchronous register   k_reg_find_take, read-back; k_reg_claim passes 1.. with `last` until none
//                          defers (read-back each); k_reg_commit_elect[_cx]; k_reg_report.
//   asynchronous register  k_reg_find_take; k_reg_claim_gated passes 1 .. REG_PASSES[_SMALL]-1;
//                          k_reg_commit_elect[_cx]; k_reg_report.  No read-back.
//   unregister             k_unreg_cas alone when nobody asks which item removed; else
//                          k_unreg_find_elect, k_unreg_commit_elect[_cx].
//   upsert                 k_reg_claim passes 0.. with last = nullptr; k_up_last; k_up_apply; k_up_clear.
//   merge                  k_reg_claim passes 0.. with last = nullptr; k_dup_mark; k_up_clear;
//                          k_merge_apply (or k_reg_abort), gd_dirops.h.
//   activation directory   add: k_reg_claim passes 0.. with `last`; k_reg_commit_elect; k_reg_report.
//                          remove: k_ad_find with `last`; k_unreg_commit_elect.
//                          set_flags: k_ad_find; k_up_last; k_ad_setflags; k_up_clear (gd_actdir.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_common.h"
#include "gd_probe.h"

namespace gd {

constexpr uint32_t SLOT_RETRY = 0xFFFFFFFEu;    // slot_of: deferred to the next claim pass
// PENDING's tag of claim launch `pass`
__device__ __forceinline__ uint32_t claim_tag(uint32_t pass) { return (pass + 1u) & 0xFFFFu; }
// The claim passes an asynchronous batch enqueues (k_reg_find_take is pass 0).  k_reg_find_take settles
// one new grain of each group colliding on a first free slot; a claim pass settles every item it runs
// except those that read a fresh claim's election word before it was written, so the passes after the
// first are a margin for that window, wider in a large batch (300,000 new grains in a 2M-slot table have
// needed more than 3).
constexpr uint32_t REG_PASSES = 12;
constexpr uint32_t REG_PASSES_SMALL = 4;    // ... for a batch of at most 2^16 items
constexpr uint8_t REG_CANDIDATE = 2;        // is_new: reg_find_item left a free slot to take
constexpr uint32_t ERR_UNSETTLED = 64u;     // DevCounters::err: an asynchronous batch's claims did not settle

// ------------------------------------------------------------------ counters, one atomic a wave
// The claims' counter updates (one per item queued ~10^4 same-address atomics behind a 1 % registration
// batch: 0.12 ms of it at cfg 2).  Every lane of the wave calls it.
__device__ __forceinline__ void claim_counters(DevCounters* ctr, uint32_t pdist, bool reused) {
    for (int off = WAVE / 2; off > 0; off >>= 1) pdist = max(pdist, (uint32_t)__shfl_xor(pdist, off, WAVE));
    const unsigned long long m = __ballot(reused);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        // max_probe only grows: a wave whose distance is not past it (nearly all) skips the atomic
        if (pdist && pdist > __hip_atomic_load(&ctr->max_probe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&ctr->max_probe, pdist);
        if (m) atomicAdd(ctr_stripe(ctr) + 1, ~(unsigned long long)__popcll(m) + 1ull);   // tomb - reused
    }
}
// The deferred items' count (every lane of the wave calls it).
__device__ __forceinline__ void count_deferred(uint32_t* retry, bool deferred) {
    const unsigned long long dm = __ballot(deferred);
    if ((threadIdx.x & (WAVE - 1)) == 0 && dm) atomicAdd(retry, (uint32_t)__popcll(dm));
}
// live (+1 an insert, or -1 and tomb +1 a removal) for the wave's flagged lanes.  Every lane of the wave
// calls it.
__device__ __forceinline__ void live_delta(DevCounters* ctr, bool flag, bool removal) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & (WAVE - 1)) != 0 || !m) return;
    const unsigned long long c = (unsigned long long)__popcll(m);
    unsigned long long* st = ctr_stripe(ctr);        // folded into live / tomb by k_ctr_fold
    atomicAdd(st, removal ? ~c + 1ull : c);
    if (removal) atomicAdd(st + 1, c);
}

// ------------------------------------------------------------------ the claim
// What differs between the tables that share the claim walk and the rehash (claim_walk, rehash_place): the
// key and its home, the slot's words, the meta's layout.  This one is the 32-B Slot keyed by 24 B: the
// directory, the activation directory and the gateway's two tables.  CbSlots (gd_callbacks.h) is the other.
struct DirSlots {
    using Key = gd_key;
    Slot* slots;
    unsigned long long mask;
    __device__ __forceinline__ unsigned long long home(const gd_key& k) const {
        return home_slot(uniform_hash(k.n0, k.n1, k.type_code_data), mask);
    }
    __device__ __forceinline__ uint32_t* meta(unsigned long long s) const { return &slots[s].meta; }
    static __device__ __forceinline__ uint32_t state(uint32_t meta) { return slot_state(meta); }
    static __device__ __forceinline__ uint32_t tag(uint32_t meta) { return slot_silo(meta); }
    static __device__ __forceinline__ uint32_t claimed() { return make_meta(SLOT_CLAIMED, 0); }
    static __device__ __forceinline__ uint32_t pending(uint32_t tag) { return make_meta(SLOT_PENDING, tag); }
    // the key and a null value
    __device__ __forceinline__ void put(unsigned long long s, const gd_key& k) const {
        Slot& sl = slots[s];
        sl.n0 = k.n0;
        sl.n1 = k.n1;
        sl.tcd = k.type_code_data;
        sl.act = NONE32;
    }
    __device__ __forceinline__ bool holds(unsigned long long s, const gd_key& k) const {
        const uint64_t k0 = slots[s].n0, k1 = slots[s].n1, k2 = slots[s].tcd;
        return k0 == k.n0 && k1 == k.n1 && k2 == k.type_code_data;
    }
    static __device__ __forceinline__ bool same(const gd_key& a, const gd_key& b) {
        return a.n0 == b.n0 && a.n1 == b.n1 && a.type_code_data == b.type_code_data;
    }
};

// One item: find the key's slot or claim a free one (slot_of, is_new = the entry is this batch's).  Returns
// whether this item made the claim.  err: the table's error word (bit 2: no free slot).
// last is nullable: upsert and merge pass nullptr, because their word holds 1 + index (last wins), and an
// election in ~i beside it would cost them a launch.
template <typename P>
__device__ __forceinline__ bool claim_walk(const P t, uint32_t i, const typename P::Key* __restrict__ keys,
                                           uint32_t* err, uint32_t* __restrict__ slot_of,
                                           uint8_t* __restrict__ is_new, uint32_t* retry, uint32_t& pdist, bool& reused,
                                           uint32_t tag, uint32_t* __restrict__ last) {
    const typename P::Key key = keys[i];
    unsigned long long s = t.home(key);
    unsigned long long dist = 0;
    uint32_t res = NONE32;
    uint8_t fresh = 0;
    bool claimed = false;
    // The key's first tombstone, reused when the chain does not hold the key (a directory under
    // continuous RemoveActivation / AddSingleActivation churn does not fill with tombstones until a
    // rehash).  Every item of one key meets the same first free slot, and a claim is a CAS, so a key is
    // never placed twice.  An item that loses its free slot (the tombstone, or the empty slot ending the
    // chain) to another item of the launch walks on from that slot in the same pass: it meets the winner's
    // claim there -- its twin's: join it; another key's: the chain's next free slot is the next try.  (Deferred
    // to the next pass instead, k new grains of a batch sharing a chain took k passes, and an asynchronous
    // batch has REG_PASSES_SMALL.)
    unsigned long long tomb_s = ~0ull, tomb_dist = 0;
    uint32_t tomb_meta = 0;
    for (;;) {
        const uint32_t meta = __hip_atomic_load(t.meta(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t st = P::state(meta);
        // the chain ends (an empty slot, or the whole table walked) without a copy of the key
        const bool ends = st == SLOT_EMPTY || dist > t.mask;
        if (ends && st != SLOT_EMPTY && tomb_s == ~0ull) {
            atomicOr(err, 2u);                               // no free slot: the table is full
            break;
        }
        bool won = false;
        const bool tomb = tomb_s != ~0ull;
        const unsigned long long c = tomb ? tomb_s : s, d = tomb ? tomb_dist : dist;
        if (ends) {
            // claim slot c for the key: the claimer's index in the slot's election word (readable by this
            // launch's walks), the key, then PENDING with this launch's tag (read as unpublished by this
            // launch's other items; published to later launches by the kernel boundary)
            uint32_t expected = tomb ? tomb_meta : meta;
            uint32_t* mp = t.meta(c);
            won = __hip_atomic_compare_exchange_strong(mp, &expected, P::claimed(), __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
            if (won) {
                if (last) atomicMax(&last[c], ~i);
                t.put(c, key);
                __hip_atomic_store(mp, P::pending(tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        // The winner's writes above stay inside the loop: the wave's losers of the same slot read the election
        // word in their next iteration.  Without this join the winner's block only leads out of the loop, and
        // a divergent wave runs such a block after its last lane has left the loop -- after the losers had
        // read a zero word and deferred, one settled item a wave and pass.  The builtin emits no instruction:
        // it is a convergent call the compiler does not duplicate, which keeps the join one block of the
        // loop.  That is a property of code generation, not of the memory model, and correctness does not
        // rest on it (a loser that reads a zero word defers, as before): a compiler that moves the block out
        // again brings back the k-passes behaviour silently, and tests/test_gpu_dir_chains.py's asynchronous
        // cases (20 new grains on one tombstoned chain in 4 passes) then fail with GD_ETIMEOUT.
        __builtin_amdgcn_wave_barrier();
        if (won) {
            pdist = (uint32_t)d;                             // max_probe: claim_counters
            reused = tomb;                                   // tomb - 1: claim_counters
            res = (uint32_t)c;
            fresh = 1;
            claimed = true;
            break;
        }
        if (ends) {
            // lost slot c: walk on from it (an empty slot that was lost is read again as it is)
            s = c;
            dist = d;
            tomb_s = ~0ull;
            continue;
        }
        const bool unpublished = st == SLOT_CLAIMED || (st == SLOT_PENDING && P::tag(meta) == tag);
        if (unpublished) {
            // claimed in this launch: its key is not published to this launch, but its claimer is (the slot's
            // election word, written right after the claim): the key's twin -- join it -- or another key's
            // claim -- walk on.  Only a claim whose word is not yet visible defers the item (no wait: the
            // claimer may be a lane of this wave).
            const uint32_t w = last ? __hip_atomic_load(&last[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            if (w == 0) {
                res = SLOT_RETRY;
                atomicAdd(retry, 1u);
                break;
            }
            if (P::same(keys[~w], key)) {
                res = (uint32_t)s;
                fresh = 1;
                break;
            }
        }
        if (st == SLOT_TOMB && tomb_s == ~0ull) {
            tomb_s = s;
            tomb_meta = meta;
            tomb_dist = dist;
        }
        if (!unpublished && (st == SLOT_LIVE || st == SLOT_PENDING)) {   // a key published before this launch
            if (t.holds(s, key)) {
                res = (uint32_t)s;
                fresh = (st == SLOT_PENDING) ? 1 : 0;
                break;
            }
        }
        s = (s + 1) & t.mask;
        ++dist;
    }
    slot_of[i] = res;
    is_new[i] = fresh;
    return claimed;
}

// The walk over a 32-B-slot table, behind the IsValidSilo check of AddSingleActivation / AddActivation
// (GrainDirectoryPartition.cs:279,310): vals / vt (vals nullable), an item whose silo is not valid is skipped
// (slot_of = NONE32).
__device__ __forceinline__ void reg_claim_item(uint32_t i, const gd_key* __restrict__ keys, Slot* slots,
                                               unsigned long long mask, DevCounters* ctr,
                                               uint32_t* __restrict__ slot_of, uint8_t* __restrict__ is_new,
                                               const gd_val* __restrict__ vals, const TableArgs& vt, uint32_t* retry,
                                               uint32_t& pdist, bool& reused, uint32_t tag,
                                               uint32_t* __restrict__ last) {
    if (vals && !tab_silo_valid(vt, vals[i].silo)) {
        slot_of[i] = NONE32;
        is_new[i] = 0;
        return;
    }
    (void)claim_walk(DirSlots{slots, mask}, i, keys, &ctr->err, slot_of, is_new, retry, pdist, reused, tag, last);
}

// A known-distinct live entry into a zeroed table (the rebuilds: no key is compared): the first EMPTY slot from
// the key's home on, claimed by CAS; payload(s) stores what put() left null; then the meta.  Returns the probe
// distance, or NONE32 when the table has no empty slot.
template <typename P, typename F>
__device__ __forceinline__ uint32_t rehash_place(const P t, const typename P::Key& key, uint32_t meta, F payload) {
    unsigned long long s = t.home(key);
    for (unsigned long long dist = 0; dist <= t.mask; ++dist) {
        uint32_t expected = 0;                               // EMPTY
        if (__hip_atomic_compare_exchange_strong(t.meta(s), &expected, P::claimed(), __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT)) {
            t.put(s, key);
            payload(s);
            __hip_atomic_store(t.meta(s), meta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return (uint32_t)dist;
        }
        s = (s + 1) & t.mask;
    }
    return NONE32;
}

// A read-back-driven claim pass.  pass 0: every item; later passes: the items the previous one deferred.
// last: see claim_walk; set, an item that ends with a new entry (claimed it, or found it PENDING)
// elects itself.
static __global__ void __launch_bounds__(BLOCK) k_reg_claim(const gd_key* __restrict__ keys, uint32_t n, Slot* slots,
                                                     unsigned long long mask, DevCounters* ctr,
                                                     uint32_t* __restrict__ slot_of,
                                                     uint8_t* __restrict__ is_new, uint32_t pass,
                                                     const gd_val* __restrict__ vals, TableArgs vt,
                                                     uint32_t* __restrict__ last = nullptr) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pd = 0;
    bool reused = false;
    if (i < n && (pass == 0 || slot_of[i] == SLOT_RETRY)) {
        reg_claim_item(i, keys, slots, mask, ctr, slot_of, is_new, vals, vt, &ctr->retry, pd, reused,
                       claim_tag(pass), last);
        if (last && is_new[i]) atomicMax(&last[slot_of[i]], ~i);
    }
    claim_counters(ctr, pd, reused);
}

// The claim pass of an asynchronous batch (gd_dir_register_device_async): pass p >= 1 runs only when
// pass p - 1 deferred items (gate = its retry word; all lanes read the same word), so the host enqueues
// its passes without reading a count back.
static __global__ void __launch_bounds__(BLOCK) k_reg_claim_gated(const gd_key* __restrict__ keys, uint32_t n,
                                                           Slot* slots, unsigned long long mask, DevCounters* ctr,
                                                           uint32_t* __restrict__ slot_of,
                                                           uint8_t* __restrict__ is_new,
                                                           const gd_val* __restrict__ vals, TableArgs vt,
                                                           const uint32_t* __restrict__ gate, uint32_t* retry,
                                                           uint32_t* __restrict__ last, uint32_t pass) {
    if (*gate == 0) return;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pd = 0;
    bool reused = false;
    if (i < n && slot_of[i] == SLOT_RETRY) {
        reg_claim_item(i, keys, slots, mask, ctr, slot_of, is_new, vals, vt, retry, pd, reused, claim_tag(pass),
                       last);
        if (is_new[i]) atomicMax(&last[slot_of[i]], ~i);    // the election (k_reg_commit_elect)
    }
    claim_counters(ctr, pd, reused);
}

// ------------------------------------------------------------------ find + take: a register batch's pass 0
// The walk with plain loads, four slots a step (the claim passes walk each chain with agent-scope atomic
// loads, two dependent L2 round trips a slot: 0.08 ms for a 10^4-item batch at cfg 2): the item's existing
// entry, or the first free slot of its chain and that slot's meta (seen[i], is_new REG_CANDIDATE).
// Other items of the launch claim slots meanwhile: a slot CLAIMED or PENDING holds a key unpublished to
// this launch, whose claimer the slot's election word names -- this key's twin: join it (is_new 1) -- or
// another key: walk on; a claim not yet recorded defers the item (SLOT_RETRY).  A stale EMPTY or
// tombstone in a cached line only makes the take's CAS fail (the CAS is the arbiter).
__device__ __forceinline__ void reg_find_item(uint32_t i, const gd_key* __restrict__ keys,
                                              const Slot* __restrict__ slots, unsigned long long mask,
                                              DevCounters* ctr, uint32_t* __restrict__ slot_of,
                                              uint8_t* __restrict__ is_new, uint32_t* __restrict__ seen,
                                              const gd_val* __restrict__ vals, const TableArgs& vt,
                                              uint32_t* __restrict__ last) {
    if (vals && !tab_silo_valid(vt, vals[i].silo)) {
        slot_of[i] = NONE32;
        is_new[i] = 0;
        return;
    }
    const uint64_t n0 = keys[i].n0, n1 = keys[i].n1, tcd = keys[i].type_code_data;
    unsigned long long s = home_slot(uniform_hash(n0, n1, tcd), mask);
    unsigned long long free_s = ~0ull;
    uint32_t free_meta = 0, res = NONE32;
    uint8_t st_out = 0;
    // four slots (one 128-B line) a step: homes are 8-slot aligned, so a chain is mostly one or two steps
    bool done = false;
    for (unsigned long long dist = 0; !done && dist <= mask; dist += 4) {
        uint4 q[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4* p = reinterpret_cast<const uint4*>(slots + ((s + k) & mask));
            q[2 * k] = p[0];
            q[2 * k + 1] = p[1];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (done) continue;
            const uint4 a = q[2 * k], b = q[2 * k + 1];
            const uint32_t st = slot_state(b.w);
            const unsigned long long sk = (s + k) & mask;
            if (st == SLOT_EMPTY) {
                if (free_s == ~0ull) {
                    free_s = sk;
                    free_meta = b.w;
                }
                done = true;
            } else if (st == SLOT_CLAIMED || st == SLOT_PENDING) {
                const uint32_t w = __hip_atomic_load(&last[sk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (w == 0) {
                    res = SLOT_RETRY;                    // a claim of this launch not yet recorded
                    done = true;
                } else {
                    const gd_key& c = keys[~w];
                    if (c.n0 == n0 && c.n1 == n1 && c.type_code_data == tcd) {
                        res = (uint32_t)sk;              // the twin's claim: join it
                        st_out = 1;
                        done = true;
                    }                                    // else another key's claim: walk on
                }
            } else {
                if (st == SLOT_TOMB && free_s == ~0ull) {
                    free_s = sk;
                    free_meta = b.w;
                }
                if (st == SLOT_LIVE && ((uint64_t)a.x | ((uint64_t)a.y << 32)) == n0 &&
                    ((uint64_t)a.z | ((uint64_t)a.w << 32)) == n1 && ((uint64_t)b.x | ((uint64_t)b.y << 32)) == tcd) {
                    res = (uint32_t)sk;                  // registered already
                    done = true;
                }
            }
        }
        s = (s + 4) & mask;
    }
    if (res == NONE32 && st_out != 1) {
        if (free_s == ~0ull) {
            atomicOr(&ctr->err, 2u);                     // no free slot: the table is full
        } else {
            res = (uint32_t)free_s;
            seen[i] = free_meta;
            st_out = REG_CANDIDATE;
        }
    }
    slot_of[i] = res;
    is_new[i] = st_out;
}

// One CAS on the slot reg_find_item left (pd / reused for claim_counters; deferred: the item lost the CAS
// and goes to the next claim pass).
__device__ __forceinline__ void reg_take_item(uint32_t i, const gd_key* __restrict__ keys, Slot* slots,
                                              unsigned long long mask, uint32_t* __restrict__ slot_of,
                                              uint8_t* __restrict__ is_new, const uint32_t* __restrict__ seen,
                                              uint32_t* __restrict__ last, uint32_t& pd, bool& reused,
                                              bool& deferred) {
    if (is_new[i] == REG_CANDIDATE) {
        const uint32_t t = slot_of[i];
        uint32_t expected = seen[i];
        uint32_t* mp = &slots[t].meta;
        if (__hip_atomic_compare_exchange_strong(mp, &expected, make_meta(SLOT_CLAIMED, 0), __ATOMIC_RELAXED,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            // No item of this launch reads the key of a slot another item claimed (a walk that meets the
            // claim reads the election word, a CAS loser defers below), so the key needs no release here:
            // the kernel's end publishes it to the passes and commit that read it (an agent-scope release
            // fence writes the XCD's L2 back, per wave: 2.2 ns an item at cfg 3's 100M registrations, 72 ms
            // a 33M batch)
            atomicMax(&last[t], ~i);                     // the election (k_reg_commit_elect), and the claimer
            const uint64_t n0 = keys[i].n0, n1 = keys[i].n1, tcd = keys[i].type_code_data;
            Slot& sl = slots[t];
            sl.n0 = n0;
            sl.n1 = n1;
            sl.tcd = tcd;
            sl.act = NONE32;
            __hip_atomic_store(mp, make_meta(SLOT_PENDING, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long home = home_slot(uniform_hash(n0, n1, tcd), mask);
            pd = (uint32_t)((t - home) & mask);
            reused = slot_state(seen[i]) == SLOT_TOMB;
            is_new[i] = 1;
        } else {
            // taken meanwhile (another new grain homed nearby, or this key's twin, whose key this launch
            // has not published): the full protocol in the next claim pass
            slot_of[i] = SLOT_RETRY;
            is_new[i] = 0;
            deferred = true;
        }
    }
}
// Each item walks with plain loads and takes its free slot at once; an item whose walk meets a claim of
// this launch not yet recorded, or that loses its CAS, defers to the claim passes (counted in *retry).
// zero (asynchronous batches): the gated passes' counters.
static __global__ void __launch_bounds__(BLOCK) k_reg_find_take(const gd_key* __restrict__ keys, uint32_t n,
                                                         Slot* slots, unsigned long long mask, DevCounters* ctr,
                                                         const gd_val* __restrict__ vals, TableArgs vt,
                                                         uint32_t* __restrict__ slot_of, uint8_t* __restrict__ is_new,
                                                         uint32_t* __restrict__ seen, uint32_t* retry, uint32_t* zero,
                                                         uint32_t* __restrict__ last) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (zero && i < REG_PASSES - 1) zero[i] = 0;         // the gated passes' counters (asynchronous batches)
    uint32_t pd = 0;
    bool reused = false, deferred = false;
    if (i < n) {
        reg_find_item(i, keys, slots, mask, ctr, slot_of, is_new, seen, vals, vt, last);
        if (slot_of[i] == SLOT_RETRY) deferred = true;
        else if (is_new[i] == 1) atomicMax(&last[slot_of[i]], ~i);      // joined its twin's claim
        else reg_take_item(i, keys, slots, mask, slot_of, is_new, seen, last, pd, reused, deferred);
    }
    count_deferred(retry, deferred);
    claim_counters(ctr, pd, reused);
}

// ------------------------------------------------------------------ commit and report (first wins)
// Item i is elected when it holds its slot's word (~i): it clears the word for the next batch; win[i]
// (i or NONE32) is for k_reg_report.
__device__ __forceinline__ bool reg_elected(uint32_t i, uint32_t n, const uint32_t* __restrict__ slot_of,
                                            const uint8_t* __restrict__ is_new, uint32_t* __restrict__ last,
                                            uint32_t* __restrict__ win) {
    if (i >= n) return false;
    bool w = false;
    if (is_new[i]) {
        const uint32_t s = slot_of[i];
        w = last[s] == ~i;
        if (w) last[s] = 0;                              // losers read ~winner or 0: never their own
    }
    win[i] = w ? i : NONE32;
    return w;
}
__device__ __forceinline__ void reg_commit_item(uint32_t i, const uint32_t* __restrict__ slot_of,
                                                const gd_val* __restrict__ vals, Slot* slots, DevCounters* ctr,
                                                uint32_t* __restrict__ vtag, uint32_t op) {
    Slot& sl = slots[slot_of[i]];
    if (vals[i].silo > 0xFFFEu) atomicOr(&ctr->err, 4u);   // silo index out of range (device-side values)
    sl.act = vals[i].act;
    sl.meta = make_meta(SLOT_LIVE, vals[i].silo);
    // GrainInfo.AddSingleActivation: SingleInstance = true, VersionTag = rand.Next() (:110-124)
    if (vtag) vtag[slot_of[i]] = VTAG_SINGLE | version_tag(op, uniform_hash(sl.n0, sl.n1, sl.tcd));
}
// unsettled (optional, asynchronous batches): the last gated pass's deferred count -- a batch still
// unsettled flags ERR_UNSETTLED -- and retry0, zeroed here for the next batch (k_reg_find_take counts into
// it).  vtag is optional (the activation directory has none).
static __global__ void __launch_bounds__(BLOCK) k_reg_commit_elect(const uint32_t* __restrict__ slot_of,
                                                            const uint8_t* __restrict__ is_new,
                                                            const gd_val* __restrict__ vals, uint32_t n, Slot* slots,
                                                            DevCounters* ctr, uint32_t* __restrict__ vtag, uint32_t op,
                                                            uint32_t* __restrict__ last, uint32_t* __restrict__ win,
                                                            const uint32_t* __restrict__ unsettled,
                                                            uint32_t* __restrict__ retry0) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0 && unsettled) {
        if (*unsettled) atomicOr(&ctr->err, ERR_UNSETTLED);
        *retry0 = 0;                                     // k_reg_find_take's counter, for the next batch
    }
    const bool w = reg_elected(i, n, slot_of, is_new, last, win);
    if (w) reg_commit_item(i, slot_of, vals, slots, ctr, vtag, op);
    live_delta(ctr, w, false);
}

static __global__ void __launch_bounds__(BLOCK) k_reg_report(const uint32_t* __restrict__ slot_of,
                                                      const uint32_t* __restrict__ win, uint32_t n,
                                                      const Slot* slots, gd_val* __restrict__ out_vals,
                                                      uint8_t* __restrict__ out_inserted) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slot_of[i];
    if (s >= SLOT_RETRY) {
        if (out_vals) out_vals[i] = gd_val{NONE32, NONE32};
        if (out_inserted) out_inserted[i] = 0;
        return;
    }
    const Slot sl = slots[s];
    if (out_vals) out_vals[i] = gd_val{sl.act, slot_silo(sl.meta)};
    if (out_inserted) out_inserted[i] = (win[i] == i) ? 1 : 0;
}

// ------------------------------------------------------------------ last wins (gd_dir_upsert)
// The last batch item of each slot wins (batch order), then writes its value: the word holds 1 + the
// winning index.
static __global__ void __launch_bounds__(BLOCK) k_up_last(const uint32_t* __restrict__ slot_of, uint32_t n,
                                                   uint32_t* __restrict__ last) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || slot_of[i] >= SLOT_RETRY) return;
    atomicMax(&last[slot_of[i]], i + 1);
}
static __global__ void __launch_bounds__(BLOCK) k_up_apply(const uint32_t* __restrict__ slot_of,
                                                    const uint8_t* __restrict__ is_new, const gd_val* __restrict__ vals,
                                                    uint32_t n, const uint32_t* __restrict__ last, Slot* slots,
                                                    DevCounters* ctr, uint8_t* __restrict__ out_inserted,
                                                    uint32_t* __restrict__ vtag, uint32_t op) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slot_of[i];
    uint8_t ins = 0;
    if (s < SLOT_RETRY && last[s] == i + 1) {
        Slot& sl = slots[s];
        // GrainInfo.AddActivation (:89-108): a new tag unless the same activation is refreshed on the
        // same silo; the entry is no longer in single-instance mode
        const bool same = !is_new[i] && sl.act == vals[i].act && slot_silo(sl.meta) == vals[i].silo;
        if (vtag && !same) vtag[s] = version_tag(op, uniform_hash(sl.n0, sl.n1, sl.tcd));
        sl.act = vals[i].act;
        sl.meta = make_meta(SLOT_LIVE, vals[i].silo);
        if (is_new[i]) {
            atomicAdd(&ctr->live, 1ull);
            ins = 1;
        }
    }
    out_inserted[i] = ins;
}
// Zeroes the words of every slot the batch's items ended on (either encoding).
static __global__ void __launch_bounds__(BLOCK) k_up_clear(const uint32_t* __restrict__ slot_of, uint32_t n,
                                                    uint32_t* __restrict__ last) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n && slot_of[i] < SLOT_RETRY) last[slot_of[i]] = 0;
}

// ------------------------------------------------------------------ RemoveActivation
// Find the live entry whose single activation matches; the find also elects the first matching item of
// the batch (atomicMax(~i)), the commit tombstones the slot for the elected item and clears the word.
__device__ __forceinline__ void unreg_find_elect_item(uint32_t i, const gd_key* __restrict__ keys,
                                                      const uint32_t* __restrict__ acts, const Slot* slots,
                                                      unsigned long long mask, const DevCounters* ctr,
                                                      uint32_t* __restrict__ slot_of, uint32_t* __restrict__ last) {
    uint4 b;
    uint32_t res = find_slot(slots, mask, ctr->max_probe, keys[i].n0, keys[i].n1, keys[i].type_code_data, b);
    if (res != NONE32 && b.z != acts[i]) res = NONE32;     // the grain's entry holds another activation
    slot_of[i] = res;
    if (res != NONE32) atomicMax(&last[res], ~i);
}
static __global__ void __launch_bounds__(BLOCK) k_unreg_find_elect(const gd_key* __restrict__ keys,
                                                            const uint32_t* __restrict__ acts, uint32_t n,
                                                            const Slot* slots, unsigned long long mask,
                                                            const DevCounters* ctr, uint32_t* __restrict__ slot_of,
                                                            uint32_t* __restrict__ last) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) unreg_find_elect_item(i, keys, acts, slots, mask, ctr, slot_of, last);
}
__device__ __forceinline__ bool unreg_elected_commit(uint32_t i, uint32_t n, const uint32_t* __restrict__ slot_of,
                                                     Slot* slots, uint32_t* __restrict__ last,
                                                     uint8_t* __restrict__ out_removed) {
    if (i >= n) return false;
    const uint32_t s = slot_of[i];
    const bool rm = s != NONE32 && last[s] == ~i;
    if (rm) {
        slots[s].meta = make_meta(SLOT_TOMB, 0);
        last[s] = 0;
    }
    if (out_removed) out_removed[i] = rm ? 1 : 0;
    return rm;
}
static __global__ void __launch_bounds__(BLOCK) k_unreg_commit_elect(const uint32_t* __restrict__ slot_of, uint32_t n,
                                                              Slot* slots, DevCounters* ctr,
                                                              uint32_t* __restrict__ last,
                                                              uint8_t* __restrict__ out_removed) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    live_delta(ctr, unreg_elected_commit(i, n, slot_of, slots, last, out_removed), true);
}

// ------------------------------------------------------------------ lookup, rehash
static __global__ void __launch_bounds__(BLOCK) k_dir_lookup(const gd_key* __restrict__ keys, uint32_t n, TableArgs tab,
                                                      gd_val* __restrict__ out_vals, uint8_t* __restrict__ found) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t n0 = keys[i].n0, n1 = keys[i].n1, tcd = keys[i].type_code_data;
    uint32_t act, meta;
    const bool hit = probe(tab.slots, tab.mask, tab.ctr->max_probe, uniform_hash(n0, n1, tcd), n0, n1, tcd, act, meta);
    out_vals[i] = hit ? gd_val{act, slot_silo(meta)} : gd_val{NONE32, NONE32};
    found[i] = hit ? 1 : 0;
}

// Rebuild: every live entry of the old table into the new one (keys are distinct,
// so a claimer never needs to compare keys).
static __global__ void __launch_bounds__(BLOCK) k_rehash(const Slot* __restrict__ old_slots, unsigned long long old_cap,
                                                  Slot* slots, unsigned long long mask, DevCounters* ctr,
                                                  const uint32_t* __restrict__ old_vtag, uint32_t* __restrict__ vtag) {
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pd = 0;
    bool placed = false;
    const Slot sl = j < old_cap ? old_slots[j] : Slot{};
    if (j < old_cap && slot_state(sl.meta) == SLOT_LIVE) {
        const DirSlots t{slots, mask};
        const uint32_t d = rehash_place(t, gd_key{sl.n0, sl.n1, sl.tcd}, sl.meta, [&](unsigned long long s) {
            slots[s].act = sl.act;
            if (vtag) vtag[s] = old_vtag[j];
        });
        placed = d != NONE32;
        if (placed) pd = d;
        else atomicOr(&ctr->err, 2u);
    }
    // one max_probe / live update a wave (one an entry queued 10^6 same-address atomics at cfg 2)
    claim_counters(ctr, pd, false);
    live_delta(ctr, placed, false);
}

}  // namespace gd
