// gd_probe.h -- the probes of the directory: the linear probe of the open-addressing table
// (GrainDirectoryPartition.cs:385-441) and the walks of its compact indexes (16-B, 8-B, direct table;
// gd_cx.h builds and maintains them).
#pragma once
#include "gd_hash.h"

namespace gd {

// ---- compact probe indexes (gd_cx.h builds and maintains them) -------------------------------
// Narrow copies of the directory table for the probe, slot for slot: index slot j mirrors table slot
// j (round 6), so a key's entry sits at the same probe distance from the same home (home_slot) as in
// the table, the table's max_probe bounds the index walk too, the build is one streaming pass
// (k_cx_project), and a directory change re-projects only the slots it touched (k_cx_sync) instead
// of rebuilding.  A read covers the aligned 64-B group holding the home slot; the walk starts at the
// home's offset in it and stops at the first empty slot (the table's own rule).
// An index covers a subset of the keys; every other key is probed in the directory itself, per
// message (route_m_core's fallback lanes), so a Guid key or an extra grain class no longer turns the
// index off table-wide.
//   16-B index: keys with N0 = 0 (GrainId.GetGrainId(typeCode, long), GrainId.cs:72-77) whose
//   TypeCodeData is in a 256-slot type set (open addressing, CX_NO_TYPE empty; staged in LDS by the
//   route kernel).  Slot {N1, act, meta = silo | type slot << 16 | CX_LIVE}; meta 0 = empty table
//   slot, CX_TOMB = a tombstone, or a live entry the index does not hold (matches no key).
constexpr uint32_t CX_GROUP = 4;
constexpr uint32_t CX_LIVE = 1u << 24;
constexpr uint32_t CX_TOMB = 1u << 25;
constexpr uint32_t CX_TYPES = 256;
constexpr unsigned long long CX_NO_TYPE = ~0ull;
struct CxArgs {
    const uint4* slots;
    unsigned long long cap;        // = the table's capacity
    const unsigned long long* types;
};
__host__ __device__ __forceinline__ uint32_t cx_type_home(uint64_t tcd) {
    return fmix32((uint32_t)tcd ^ fmix32((uint32_t)(tcd >> 32))) & (CX_TYPES - 1);
}
//   8-B index: keys with N0 = 0, N1 < 2^32 and one of up to CX8_TYPES TypeCodeData (the most
//   populous at the build, passed in the kernel arguments).  Slot {N1 low word, y}: y = u << ab | a,
//   a = the activation (all ab bits set: GD_ACT_MULTI; all but the lowest: an activation too wide
//   for ab bits -- probe the directory), u = type index << sb | (silo + 1) (all 32 - ab bits set: a
//   silo or type too wide -- probe the directory).  y = 0: empty; u = 0 (y = 1): a tombstone or a
//   live entry the index does not hold.
constexpr uint32_t CX8_GROUP = 8;
constexpr uint32_t CX8_TYPES = 8;
struct Cx8Args {
    const uint4* slots;            // two 8-B slots an uint4
    unsigned long long cap;        // = the table's capacity
    uint64_t tcd[CX8_TYPES];       // the types it holds, index order
    uint32_t ntypes;
    uint32_t ab;                   // activation bits
    uint32_t sb;                   // silo + 1 bits
    uint32_t pad;
};
// Type index of tcd in the staged type set, or -1.
__device__ __forceinline__ int cx_type_index(const unsigned long long* s_types, uint64_t tcd) {
    uint32_t t = cx_type_home(tcd);
    for (uint32_t k = 0; k < CX_TYPES; ++k) {
        const unsigned long long v = s_types[t];
        if (v == tcd) return (int)t;
        if (v == CX_NO_TYPE) return -1;
        t = (t + 1) & (CX_TYPES - 1);
    }
    return -1;
}
// The 8-B index's type index of a key, or -1 when the index does not hold it.
__device__ __forceinline__ int cx8_type(const Cx8Args& c, uint64_t n0, uint64_t n1, uint64_t tcd) {
    if (n0 != 0 || (n1 >> 32) != 0) return -1;
    if (c.ntypes <= 1) return c.ntypes && tcd == c.tcd[0] ? 0 : -1;   // one grain class (a uniform branch)
    int t = -1;
#pragma unroll
    for (int k = (int)CX8_TYPES - 1; k >= 0; --k)
        if ((uint32_t)k < c.ntypes && c.tcd[k] == tcd) t = k;
    return t;
}

//   Direct table (GD_DIRECT_INDEX, gd_cx.h k_cxd_build): while the 8-B index is pure (one grain class, N0 = 0,
//   N1 < 2^32, every live entry held, none redirected) an entry's identity is its low N1 word, so dense
//   N1s are indexed directly: tab[N1] = the 8-B slot's payload word y (same ab / sb), 0 = empty.  No key
//   word, no hash, no probe chain: the array position is the key.
#ifndef GD_DIRECT_INDEX
#define GD_DIRECT_INDEX 1
#endif
struct CxdArgs {
    const uint32_t* tab;           // d entries
    uint32_t d;                    // (largest live N1 + 1) rounded up to 16
    uint32_t ab, sb;               // the 8-B index's bit split
    uint64_t tcd;                  // its one grain class
};

// Directory entry -> route result (LookUpActivations + IsValidSilo + the single-activation choice).
__device__ __forceinline__ void entry_result(const TableArgs& tab, uint32_t a, uint32_t silo_of, uint32_t& silo,
                                             uint32_t& act, uint8_t& status) {
    if (a == GD_ACT_MULTI) {                       // several activations: the C# random choice
        status = GD_ROUTE_MULTI_ACT;               // (RandomPlacementDirector.cs:33-53)
    } else if (tab_silo_valid(tab, silo_of)) {
        act = a;
        silo = silo_of;                            // ActivationAddress.Silo (Message.cs:629-639)
        status = GD_ROUTE_OK;
    } else {
        status = GD_ROUTE_MISS;                    // IsValidSilo filtered it (GrainDirectoryPartition.cs:431)
    }
}

// An 8-B index payload word y of an entry the index holds (no redirect) -> route result.
__device__ __forceinline__ void cx8_decode(uint32_t ab, uint32_t sb, const TableArgs& tab, uint32_t y, uint32_t& silo,
                                           uint32_t& act, uint8_t& status) {
    const uint32_t am = (1u << ab) - 1u, u = y >> ab, a = y & am;
    entry_result(tab, a == am ? GD_ACT_MULTI : a, (u & ((1u << sb) - 1u)) - 1u, silo, act, status);
}

// The table's max_probe, read when a walk first leaves its home group (rare): kernels on the index do not
// load it at their start, where the scalar load would share lgkmcnt with the LDS ring staging.
__device__ __forceinline__ uint32_t lazy_max_probe(const TableArgs& tab) {
    return __hip_atomic_load(&tab.ctr->max_probe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The 16-B index's walk from the home's group q (RG slots, already read): the entry of (want = 0x100 |
// type slot, n1) or a miss (status left as is).  A key's entry lies within max_probe slots of its home;
// homes are HOME_ALIGN-aligned, so a walk starts at its group's first slot.
static_assert(HOME_ALIGN % CX_GROUP == 0 && HOME_ALIGN % CX8_GROUP == 0, "index groups start at homes");
template <int RG>
__device__ __forceinline__ void cx16_walk(const CxArgs& c, const TableArgs& tab, uint32_t want, uint64_t n1,
                                          unsigned long long home, uint4 (&q)[RG], uint32_t& silo, uint32_t& act,
                                          uint8_t& status) {
    unsigned long long g = home;
    uint32_t last = 0;
    bool done = false;
    for (uint32_t base = 0;; base += RG) {
#pragma unroll
        for (int k = 0; k < RG; ++k) {
            if (done) continue;
            const uint4 v = q[k];
            if (v.w == 0) {
                done = true;                                            // miss
            } else if ((v.w >> 16) == want && ((uint64_t)v.x | ((uint64_t)v.y << 32)) == n1) {
                entry_result(tab, v.z, slot_silo(v.w), silo, act, status);
                done = true;
            }
        }
        if (done) return;
        if (base == 0) last = lazy_max_probe(tab);
        if (base + RG > last) return;                                   // past every entry's reach: miss
        g += RG;
        if (g >= c.cap) g = 0;
#pragma unroll
        for (int k = 0; k < RG; ++k) q[k] = c.slots[g + k];
    }
}

// The 8-B index's walk from the home's group q (8 slots as 4 uint4, already read), for the key's low
// N1 word and type index qt.  Returns true when a redirect entry matched: the directory must answer.
// Per slot only the tests (empty; key; live with this type or a redirect); the hit is decoded once.
__device__ __forceinline__ bool cx8_walk(const Cx8Args& c, const TableArgs& tab, uint32_t key, uint32_t qt,
                                         unsigned long long home, uint4 (&q)[CX8_GROUP / 2], uint32_t& silo,
                                         uint32_t& act, uint8_t& status) {
    const uint32_t umax = ~0u >> c.ab;
    unsigned long long g = home;
    uint32_t last = 0;
    bool done = false;
    uint32_t hit = 0;
    for (uint32_t base = 0;; base += CX8_GROUP) {
#pragma unroll
        for (int k = 0; k < (int)CX8_GROUP; ++k) {
            if (done) continue;
            const uint4 v = q[k / 2];
            const uint32_t x = (k & 1) ? v.z : v.x, y = (k & 1) ? v.w : v.y;
            const uint32_t u = y >> c.ab;
            if (y == 0) {
                done = true;                                            // miss
            } else if (x == key && u != 0 && (u == umax || (u >> c.sb) == qt)) {
                done = true;
                hit = y;
            }
        }
        if (done) break;
        if (base == 0) last = lazy_max_probe(tab);
        if (base + CX8_GROUP > last) return false;                      // past every entry's reach: miss
        g += CX8_GROUP;
        if (g >= c.cap) g = 0;
        const uint4* qp = c.slots + (g >> 1);
#pragma unroll
        for (int k = 0; k < (int)CX8_GROUP / 2; ++k) q[k] = qp[k];
    }
    if (hit == 0) return false;
    const uint32_t am = (1u << c.ab) - 1u, u = hit >> c.ab, a = hit & am;
    if (u == umax || a == am - 1u) return true;                         // redirect: the directory answers
    cx8_decode(c.ab, c.sb, tab, hit, silo, act, status);
    return false;
}

// cx8_walk over a pure index (PURE route_m_core: one class, every live entry held, none redirected): a
// slot matches on its key word (a hole, y = 1, never -- live slots have y >= 2), no redirect is decoded,
// and the bound is the workgroup's staged max_probe.  With the fallback probe compiled out of the kernel
// and no max_probe load in the walk, k_route at cfg 2 runs 0.287 against 0.292 ms.
__device__ __forceinline__ void cx8_walk_pure(const Cx8Args& c, const TableArgs& tab, uint32_t key,
                                              unsigned long long home, uint4 (&q)[CX8_GROUP / 2], uint32_t mp,
                                              uint32_t& silo, uint32_t& act, uint8_t& status) {
    unsigned long long g = home;
    bool done = false;
    uint32_t hit = 0;
    for (uint32_t base = 0;; base += CX8_GROUP) {
#pragma unroll
        for (int k = 0; k < (int)CX8_GROUP; ++k) {
            if (done) continue;
            const uint4 v = q[k / 2];
            const uint32_t x = (k & 1) ? v.z : v.x, y = (k & 1) ? v.w : v.y;
            if (y == 0) {
                done = true;                                            // miss
            } else if (x == key && y > 1u) {
                done = true;
                hit = y;
            }
        }
        if (done || base + CX8_GROUP > mp) break;                       // found, empty, or past every entry
        g += CX8_GROUP;
        if (g >= c.cap) g = 0;
        const uint4* qp = c.slots + (g >> 1);
#pragma unroll
        for (int k = 0; k < (int)CX8_GROUP / 2; ++k) q[k] = qp[k];
    }
    if (hit != 0) cx8_decode(c.ab, c.sb, tab, hit, silo, act, status);
}

// Linear probe of the open-addressing directory for a live entry with this key.
__device__ __forceinline__ bool probe(const Slot* slots, unsigned long long mask, uint32_t max_probe,
                                      uint32_t h, uint64_t n0, uint64_t n1, uint64_t tcd,
                                      uint32_t& act, uint32_t& meta) {
    unsigned long long s = home_slot(h, mask);
    for (uint32_t p = 0; p <= max_probe; ++p) {
        const uint4* q = reinterpret_cast<const uint4*>(slots + s);
        const uint4 a = q[0];
        const uint4 b = q[1];
        const uint32_t st = slot_state(b.w);
        if (st == SLOT_EMPTY) return false;
        const uint64_t k0 = (uint64_t)a.x | ((uint64_t)a.y << 32);
        const uint64_t k1 = (uint64_t)a.z | ((uint64_t)a.w << 32);
        const uint64_t k2 = (uint64_t)b.x | ((uint64_t)b.y << 32);
        if (st == SLOT_LIVE && k0 == n0 && k1 == n1 && k2 == tcd) {
            act = b.z;
            meta = b.w;
            return true;
        }
        s = (s + 1) & mask;
    }
    return false;
}

// probe() for the batches that go on to change the entry: the slot of the key's live entry, or NONE32;
// b = the last slot read's second half {tcd, act, meta}, the entry's own on a hit.
__device__ __forceinline__ uint32_t find_slot(const Slot* __restrict__ slots, unsigned long long mask,
                                              uint32_t max_probe, uint64_t n0, uint64_t n1, uint64_t tcd, uint4& b) {
    unsigned long long s = home_slot(uniform_hash(n0, n1, tcd), mask);
    for (uint32_t p = 0; p <= max_probe; ++p) {
        const uint4* q = reinterpret_cast<const uint4*>(slots + s);
        const uint4 a = q[0];
        b = q[1];
        const uint32_t st = slot_state(b.w);
        if (st == SLOT_EMPTY) break;
        if (st == SLOT_LIVE && ((uint64_t)a.x | ((uint64_t)a.y << 32)) == n0 &&
            ((uint64_t)a.z | ((uint64_t)a.w << 32)) == n1 && ((uint64_t)b.x | ((uint64_t)b.y << 32)) == tcd)
            return (uint32_t)s;
        s = (s + 1) & mask;
    }
    return NONE32;
}

}  // namespace gd
