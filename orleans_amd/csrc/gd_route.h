// gd_route.h -- the route kernels (hot path, per message, all integer, HBM-bound, no MFMA):
//   K0+K1+K2  k_route*       Jenkins hash of the 24-B GrainId, ring search over an LDS-staged snapshot
//                            (gd_hash.h), probe of the directory or of one of its indexes (gd_probe.h).
// The batches that change the directory table (register, upsert, unregister, rehash): gd_dirbatch.h.
#pragma once
#include "gd_probe.h"

namespace gd {

// ------------------------------------------------------------------ K0+K1+K2: route
// One message: ring owner (ring staged in LDS) and, PROBE, the directory entry.
template <int MODE, bool PROBE>
__device__ __forceinline__ void route_one(uint64_t n0, uint64_t n1, uint64_t tcd, const RingArgs& ring,
                                          const uint32_t* s_pts, const uint32_t* s_own, const TableArgs& tab,
                                          uint32_t max_probe, uint32_t& silo, uint32_t& act, uint8_t& status) {
    const uint32_t cat = (uint32_t)(tcd >> 56);
    act = NONE32;
    if (cat == CAT_SYSTEM_TARGET) {                        // LocalGrainDirectory.cs:480-485
        silo = ring.my_silo;
        status = GD_ROUTE_SYSTEM_TARGET;
    } else if (is_membership(n0, n1, tcd)) {               // :487-503
        silo = ring.seed_silo;
        status = GD_ROUTE_MEMBERSHIP;
    } else if (cat == CAT_KEYEXT_GRAIN || cat == CAT_GEO_CLIENT) {  // UniqueKey.cs:279-281
        silo = NONE32;
        status = GD_ROUTE_KEYEXT;
    } else {
        const uint32_t h = uniform_hash(n0, n1, tcd);
        silo = s_own[ring_position<MODE>(s_pts, ring.n, ring.top, h)];
        status = GD_ROUTE_OK;
        if constexpr (PROBE) {
            uint32_t a, meta;
            if (probe(tab.slots, tab.mask, max_probe, h, n0, n1, tcd, a, meta)) {
                if (a == GD_ACT_MULTI) {
                    status = GD_ROUTE_MULTI_ACT;           // RandomPlacementDirector.cs:33-53, in C#
                } else if (!tab_silo_valid(tab, slot_silo(meta))) {
                    status = GD_ROUTE_MISS;                // LookUpActivations filters it (:431): no address
                } else {
                    act = a;
                    silo = slot_silo(meta);                // ActivationAddress.Silo (Message.cs:629-639)
                }
            } else {
                status = GD_ROUTE_MISS;                    // Dispatcher.cs:742 slow path
            }
        }
    }
}

// One message per thread.  PROBE=false gives CalculateTargetSilo only.
template <int MODE, bool PROBE>
static __global__ void __launch_bounds__(BLOCK) k_route(const gd_key* __restrict__ keys, uint32_t n, RingArgs ring,
                                                 TableArgs tab, uint32_t* __restrict__ out_silo,
                                                 uint32_t* __restrict__ out_act,
                                                 uint8_t* __restrict__ out_status) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_ring[];
    uint32_t* s_pts = s_ring;
    uint32_t* s_own = s_ring + ring.n;
    stage_ring(ring, s_pts, s_own);
    const uint32_t max_probe = PROBE ? tab.ctr->max_probe : 0;

    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t* kp = reinterpret_cast<const uint64_t*>(keys + i);
    uint32_t silo, act;
    uint8_t status;
    route_one<MODE, PROBE>(kp[0], kp[1], kp[2], ring, s_pts, s_own, tab, max_probe, silo, act, status);
    out_silo[i] = silo;
    if constexpr (PROBE) {
        out_act[i] = act;
        out_status[i] = status;
    }
}

template <bool NT, typename T>
__device__ __forceinline__ T ld(const T* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT, typename T>
__device__ __forceinline__ void st(T* p, T v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// The route kernel proper: M messages per thread (coalesced: message
// base + j*BLOCK + tid), all M first probes issued before any is inspected so
// that each lane keeps M random 32-B slot reads in flight.  NT streams the key
// reads (and with NT_SIDE the silo / status writes) non-temporally so they do not
// push the table out of the caches it shares with them.
// N1W: 0 = 24-B keys; 8 / 4 = the keys arrive as N1 alone (u64 / u32 each; N0 = 0, TypeCodeData =
// tcd_u for all), the forms a compact exchange header round delivers (k_key_desc, gd_shard.h).
// The per-thread part: messages base + j * STRIDE, j < M; lds_act (optional) gets act too.
// CX: probe the compact index (cx, its type set staged in s_types) instead of the directory, RG slots
// (16 B each) a read: CX_GROUP (one 64-B atom, the layout's group) or 1 (16 B, for hot key sets).
// CX8: probe the 8-B index (cx8) instead, one 64-B group (8 slots) a read.
// PURE (with CX8, k_route_m): the index is pure (gd_engine.h cx8_pure) -- a key it does not hold is in no
// entry, so there is no directory fallback at all; mp = the table's max_probe, staged by the caller.
template <int MODE, int M, int STRIDE, bool NT, int N1W, bool NT_SIDE = false, bool CX = false,
          int RG_CX = (int)CX_GROUP, bool CX8 = false, bool PURE = false>
__device__ __forceinline__ void route_m_core(const gd_key* __restrict__ keys, uint32_t n, uint32_t base,
                                             const RingArgs& ring, const uint32_t* s_pts, const uint32_t* s_own,
                                             const TableArgs& tab, uint32_t max_probe,
                                             uint32_t* __restrict__ out_silo, uint32_t* __restrict__ out_act,
                                             uint8_t* __restrict__ out_status, uint64_t tcd_u,
                                             uint32_t* lds_act, uint32_t lds_stride, const CxArgs* cx = nullptr,
                                             const unsigned long long* s_types = nullptr,
                                             const Cx8Args* cx8 = nullptr, uint32_t mp = 0) {

    uint64_t n0[M], n1[M], tcd[M];
    uint32_t h[M], silo[M], act[M];
    uint8_t status[M];
    bool need[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const uint32_t i = base + j * STRIDE;
        n0[j] = n1[j] = tcd[j] = 0;
        if (i < n) {
            if constexpr (N1W == 8) {
                n1[j] = ld<NT>(reinterpret_cast<const uint64_t*>(keys) + i);
                tcd[j] = tcd_u;
            } else if constexpr (N1W == 4) {
                n1[j] = ld<NT>(reinterpret_cast<const uint32_t*>(keys) + i);
                tcd[j] = tcd_u;
            } else {
                const uint64_t* kp = reinterpret_cast<const uint64_t*>(keys + i);
                n0[j] = ld<NT>(kp);
                n1[j] = ld<NT>(kp + 1);
                tcd[j] = ld<NT>(kp + 2);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const uint32_t cat = (uint32_t)(tcd[j] >> 56);
        act[j] = NONE32;
        need[j] = false;
        h[j] = 0;
        if (cat == CAT_SYSTEM_TARGET) {                        // LocalGrainDirectory.cs:480-485
            silo[j] = ring.my_silo;
            status[j] = GD_ROUTE_SYSTEM_TARGET;
        } else if (is_membership(n0[j], n1[j], tcd[j])) {     // :487-503
            silo[j] = ring.seed_silo;
            status[j] = GD_ROUTE_MEMBERSHIP;
        } else if (cat == CAT_KEYEXT_GRAIN || cat == CAT_GEO_CLIENT) {  // UniqueKey.cs:279-281
            silo[j] = NONE32;
            status[j] = GD_ROUTE_KEYEXT;
        } else {
            h[j] = uniform_hash(n0[j], n1[j], tcd[j]);
            status[j] = GD_ROUTE_MISS;
            need[j] = true;
        }
    }
    if constexpr (CX || CX8) {
        static_assert(!(CX && CX8), "one index form a launch");
        static_assert(RG_CX == 1 || RG_CX == (int)CX_GROUP, "16-B index reads: one slot or one group");
        // Lanes whose key the index holds walk the index from the home's group; the others (fb: an N0 !=
        // 0 key, a type or N1 the index does not hold, or a redirect entry) probe the directory itself.
        constexpr int QW = CX ? RG_CX : (int)CX8_GROUP / 2;
        uint32_t want[M];
        bool fb[M];
        unsigned long long s[M];
        uint4 q[M][QW];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            want[j] = 0;
            fb[j] = false;
            s[j] = home_slot(h[j], tab.mask);
            if (need[j]) {
                if constexpr (CX) {
                    const int t = n0[j] == 0 ? cx_type_index(s_types, tcd[j]) : -1;
                    want[j] = t < 0 ? 0u : (0x100u | (uint32_t)t);
                } else {
                    const int t = cx8_type(*cx8, n0[j], n1[j], tcd[j]);
                    want[j] = t < 0 ? 0u : 1u + (uint32_t)t;
                }
                fb[j] = !PURE && want[j] == 0;
            }
            if (want[j]) {
                if constexpr (CX) {
                    const uint4* qp = cx->slots + (s[j] & ~(unsigned long long)(RG_CX - 1));
#pragma unroll
                    for (int g = 0; g < QW; ++g) q[j][g] = qp[g];
                } else {
                    const uint4* qp = cx8->slots + ((s[j] & ~(unsigned long long)(CX8_GROUP - 1)) >> 1);
#pragma unroll
                    for (int g = 0; g < QW; ++g) q[j][g] = qp[g];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < M; ++j)
            if (need[j]) silo[j] = s_own[ring_position<MODE>(s_pts, ring.n, ring.top, h[j])];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            if (!want[j]) continue;
            if constexpr (CX) cx16_walk<RG_CX>(*cx, tab, want[j], n1[j], s[j], q[j], silo[j], act[j], status[j]);
            else if constexpr (PURE) cx8_walk_pure(*cx8, tab, (uint32_t)n1[j], s[j], q[j], mp, silo[j], act[j], status[j]);
            else fb[j] = cx8_walk(*cx8, tab, (uint32_t)n1[j], want[j] - 1u, s[j], q[j], silo[j], act[j], status[j]);
        }
        if constexpr (!PURE) {
#pragma unroll
            for (int j = 0; j < M; ++j) {
                if (!fb[j]) continue;
                uint32_t a, meta;
                if (probe(tab.slots, tab.mask, lazy_max_probe(tab), h[j], n0[j], n1[j], tcd[j], a, meta))
                    entry_result(tab, a, slot_silo(meta), silo[j], act[j], status[j]);   // else MISS (Dispatcher.cs:742)
            }
        }
    } else {
    // first probe of every message, all in flight together; the ring search (LDS) runs under them.
    // A round reads the whole aligned group of SLOT_GROUP slots (home_slot) and walks it in order.
    constexpr int RG = (int)SLOT_GROUP;
    unsigned long long s[M];
    uint4 q[M][2 * RG];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        s[j] = home_slot(h[j], tab.mask);
        if (need[j]) {
            const uint4* qp = reinterpret_cast<const uint4*>(tab.slots + s[j]);
#pragma unroll
            for (int g = 0; g < 2 * RG; ++g) q[j][g] = qp[g];
        }
    }
#pragma unroll
    for (int j = 0; j < M; ++j)
        if (need[j]) silo[j] = s_own[ring_position<MODE>(s_pts, ring.n, ring.top, h[j])];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        if (!need[j]) continue;
        bool done = false;
        for (uint32_t p = 0;;) {
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                if (done) continue;
                const uint4 a = q[j][2 * g], b = q[j][2 * g + 1];
                const uint32_t stt = slot_state(b.w);
                const uint64_t k0 = (uint64_t)a.x | ((uint64_t)a.y << 32);
                const uint64_t k1 = (uint64_t)a.z | ((uint64_t)a.w << 32);
                const uint64_t k2 = (uint64_t)b.x | ((uint64_t)b.y << 32);
                if (stt == SLOT_EMPTY) {
                    done = true;                                  // miss
                } else if (stt == SLOT_LIVE && k0 == n0[j] && k1 == n1[j] && k2 == tcd[j]) {
                    if (b.z == GD_ACT_MULTI) {                    // several activations: the C# random
                        status[j] = GD_ROUTE_MULTI_ACT;           // choice (RandomPlacementDirector.cs:33-53)
                    } else if (tab_silo_valid(tab, slot_silo(b.w))) {
                        act[j] = b.z;
                        silo[j] = slot_silo(b.w);                 // ActivationAddress.Silo (Message.cs:629-639)
                        status[j] = GD_ROUTE_OK;
                    }                                             // else: IsValidSilo filtered it (:431) -> MISS
                    done = true;
                } else if (++p > max_probe) {
                    done = true;                                  // miss: Dispatcher.cs:742 slow path
                }
            }
            if (done) break;
            s[j] = (s[j] + RG) & tab.mask;
            const uint4* qp = reinterpret_cast<const uint4*>(tab.slots + s[j]);
#pragma unroll
            for (int g = 0; g < 2 * RG; ++g) q[j][g] = qp[g];
        }
    }
    }
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const uint32_t i = base + j * STRIDE;
        if (i < n) {
            st<NT || NT_SIDE>(out_silo + i, silo[j]);      // silo / status: not read again on the device
            out_act[i] = act[j];                            // act: the bucketing's input, next (temporal)
            st<NT || NT_SIDE>(out_status + i, status[j]);
            if (lds_act) lds_act[(size_t)i * lds_stride] = act[j];
        }
    }
}

// Micro-batch route over keys in pinned host memory: one-wave workgroups, so the host reads (and
// the host stores of silo / status) of a 4,096-message batch spread over 64 CUs.
constexpr int MB_ROUTE_BLOCK = 64;

// CX8: through the 8-B index (when it is current: gd_microbatch_run re-captures its graphs when the
// index is rebuilt or goes stale), the directory otherwise.
template <int MODE, bool CX8 = false>
static __global__ void __launch_bounds__(MB_ROUTE_BLOCK) k_mb_route(const gd_key* __restrict__ keys, uint32_t n,
                                                            RingArgs ring, TableArgs tab,
                                                            uint32_t* __restrict__ out_silo,
                                                            uint32_t* __restrict__ out_act,
                                                            uint8_t* __restrict__ out_status,
                                                            uint32_t* __restrict__ act_host,
                                                            unsigned long long* ts, Cx8Args cx8 = Cx8Args{}) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_ring[];
    uint32_t* s_pts = s_ring;
    uint32_t* s_own = s_ring + ring.n;
    unsigned long long t = 0;
    mb_mark(ts, 0, t);
    stage_ring(ring, s_pts, s_own);
    mb_mark(ts, 1, t);
    // act goes to HBM for the sort and, from these 64 workgroups, to the host block as well
    route_m_core<MODE, 1, MB_ROUTE_BLOCK, false, 0, false, false, (int)CX_GROUP, CX8>(
        keys, n, blockIdx.x * MB_ROUTE_BLOCK + threadIdx.x, ring, s_pts, s_own, tab,
        CX8 ? 0u : tab.ctr->max_probe, out_silo, out_act, out_status, 0, act_host, act_host ? 1u : 0u, nullptr,
        nullptr, &cx8);
    mb_mark(ts, 2, t);
    if (ts) {
        __threadfence_system();
        mb_mark(ts, 3, t);
    }
}

// src_out (optional, the exchange's receive side): message i's sender rank, from the per-sender
// receive counts rcnt[world] (k_recv_src's job, done here beside the probe's own writes).
template <int MODE, int M, bool NT, int N1W = 0, bool CX = false, int RG_CX = (int)CX_GROUP, bool CX8 = false,
          bool PURE = false>
static __global__ void __launch_bounds__(BLOCK) k_route_m(const gd_key* __restrict__ keys, uint32_t n, RingArgs ring,
                                                   TableArgs tab, uint32_t* __restrict__ out_silo,
                                                   uint32_t* __restrict__ out_act,
                                                   uint8_t* __restrict__ out_status, uint64_t tcd_u, uint32_t xcd,
                                                   const uint32_t* __restrict__ rcnt = nullptr, uint32_t world = 0,
                                                   uint32_t* __restrict__ src_out = nullptr, CxArgs cx = CxArgs{},
                                                   Cx8Args cx8 = Cx8Args{}) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_ring[];
    __shared__ uint32_t s_soff[257];
    __shared__ unsigned long long s_types[CX ? CX_TYPES : 1];
    __shared__ uint32_t s_mp;
    uint32_t* s_pts = s_ring;
    uint32_t* s_own = s_ring + ring.n;
    if constexpr (CX)
        for (uint32_t t = threadIdx.x; t < CX_TYPES; t += BLOCK) s_types[t] = cx.types[t];
    if (PURE && threadIdx.x == 0) s_mp = lazy_max_probe(tab);   // the walks' bound, one load beside the ring
    if (src_out && threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t q = 0; q < world; ++q) {
            s_soff[q] = run;
            run += rcnt[q];
        }
        s_soff[world] = run;
    }
    stage_ring(ring, s_pts, s_own);                    // its barrier publishes s_soff (and s_types) too
    // xcd: each XCD routes a contiguous message range (xcd_tile), so the act it writes is the act the
    // same XCD's histogram and scatter workgroups read next (their XCD tile ranges match)
    const uint32_t blk = xcd_tile(blockIdx.x, gridDim.x, xcd);
    route_m_core<MODE, M, BLOCK, NT, N1W, true, CX, RG_CX, CX8, PURE>(
        keys, n, blk * (BLOCK * M) + threadIdx.x, ring, s_pts, s_own, tab, (CX || CX8) ? 0u : tab.ctr->max_probe,
        out_silo, out_act, out_status, tcd_u, nullptr, 0, &cx, s_types, &cx8, PURE ? s_mp : 0u);
    if (src_out) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const uint32_t i = blk * (BLOCK * M) + j * BLOCK + threadIdx.x;
            if (i >= n) continue;
            uint32_t lo = 0, hi = world;               // largest q with s_soff[q] <= i
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_soff[mid] <= i) lo = mid;
                else hi = mid;
            }
            st<true>(src_out + i, lo);
        }
    }
}

#if GD_DIRECT_INDEX
// k_route_m's DIRECT form (launched as "k_route"): the pure 8-B index stood in for by the direct table
// (CxdArgs).  A lane whose key passes the PURE path's class checks and has N1 < d reads tab[N1] with one
// 4-B temporal load; a non-zero word is the entry (cx8_decode: GD_ACT_MULTI, IsValidSilo at route time).
// Only the lanes that do not end GD_ROUTE_OK -- N0 != 0, another class, N1 >= d, an empty word, an
// invalid silo, several activations -- compute the Jenkins hash and search the ring, for the owner silo
// the other forms report with those statuses; a hit needs neither.  Key stream, silo / status stores and
// XCD ranges as k_route_m's; act stays a temporal store and M follows route_mode (both measured,
// profiles/r07_direct_index_ab.json).
template <int MODE, int M, bool NT, int N1W>
static __global__ void __launch_bounds__(BLOCK) k_route_d(const gd_key* __restrict__ keys, uint32_t n, RingArgs ring,
                                                   TableArgs tab, uint32_t* __restrict__ out_silo,
                                                   uint32_t* __restrict__ out_act,
                                                   uint8_t* __restrict__ out_status, uint64_t tcd_u, uint32_t xcd,
                                                   const uint32_t* __restrict__ rcnt, uint32_t world,
                                                   uint32_t* __restrict__ src_out, CxdArgs d) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_ring[];
    __shared__ uint32_t s_soff[257];
    uint32_t* s_pts = s_ring;
    uint32_t* s_own = s_ring + ring.n;
    if (src_out && threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t q = 0; q < world; ++q) {
            s_soff[q] = run;
            run += rcnt[q];
        }
        s_soff[world] = run;
    }
    stage_ring(ring, s_pts, s_own);                    // its barrier publishes s_soff too
    const uint32_t base = xcd_tile(blockIdx.x, gridDim.x, xcd) * (BLOCK * M) + threadIdx.x;
    uint64_t n0[M], n1[M], tcd[M];
    uint32_t y[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const uint32_t i = base + j * BLOCK;
        n0[j] = n1[j] = tcd[j] = 0;
        if (i < n) {
            if constexpr (N1W == 8) {
                n1[j] = ld<NT>(reinterpret_cast<const uint64_t*>(keys) + i);
                tcd[j] = tcd_u;
            } else if constexpr (N1W == 4) {
                n1[j] = ld<NT>(reinterpret_cast<const uint32_t*>(keys) + i);
                tcd[j] = tcd_u;
            } else {
                const uint64_t* kp = reinterpret_cast<const uint64_t*>(keys + i);
                n0[j] = ld<NT>(kp);
                n1[j] = ld<NT>(kp + 1);
                tcd[j] = ld<NT>(kp + 2);
            }
        }
    }
    // every message's table word in flight before any is decoded (the special categories below never
    // look at theirs)
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const bool in = base + j * BLOCK < n && n0[j] == 0 && tcd[j] == d.tcd && n1[j] < (uint64_t)d.d;
        y[j] = in ? d.tab[(uint32_t)n1[j]] : 0u;
    }
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const uint32_t i = base + j * BLOCK;
        if (i >= n) continue;
        const uint32_t cat = (uint32_t)(tcd[j] >> 56);
        uint32_t silo, act = NONE32;
        uint8_t status;
        if (cat == CAT_SYSTEM_TARGET) {                        // LocalGrainDirectory.cs:480-485
            silo = ring.my_silo;
            status = GD_ROUTE_SYSTEM_TARGET;
        } else if (is_membership(n0[j], n1[j], tcd[j])) {     // :487-503
            silo = ring.seed_silo;
            status = GD_ROUTE_MEMBERSHIP;
        } else if (cat == CAT_KEYEXT_GRAIN || cat == CAT_GEO_CLIENT) {  // UniqueKey.cs:279-281
            silo = NONE32;
            status = GD_ROUTE_KEYEXT;
        } else {
            silo = 0;
            status = GD_ROUTE_MISS;
            if (y[j] != 0) cx8_decode(d.ab, d.sb, tab, y[j], silo, act, status);
            if (status != GD_ROUTE_OK)                         // the owner silo: hash and ring search, these lanes only
                silo = s_own[ring_position<MODE>(s_pts, ring.n, ring.top, uniform_hash(n0[j], n1[j], tcd[j]))];
        }
        st<true>(out_silo + i, silo);                          // silo / status: not read again on the device
        out_act[i] = act;                                      // act: the bucketing's input, next (temporal)
        st<true>(out_status + i, status);
        if (src_out) {
            uint32_t lo = 0, hi = world;                       // largest q with s_soff[q] <= i
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_soff[mid] <= i) lo = mid;
                else hi = mid;
            }
            st<true>(src_out + i, lo);
        }
    }
}
#endif  // GD_DIRECT_INDEX

// The route's memory bound (gd_route_bound_device, a diagnostic, not a route): k_route_m<…, CX8>'s XCD
// mapping, ring-sized LDS, key reads, home hash, one 64-B group read of the 8-B index per message and
// silo / act / status writes -- without the ring search, the class checks, the walk past the home group,
// the redirect decode and the directory fallback; M messages a thread (2: the fastest measured).  On the
// route's own index and key stream it is the time k_route cannot go under without reading or writing less.
template <int M, bool NT>
static __global__ void __launch_bounds__(BLOCK) k_route_bound(const gd_key* __restrict__ keys, uint32_t n,
                                                       unsigned long long mask, Cx8Args cx8,
                                                       uint32_t* __restrict__ out_silo,
                                                       uint32_t* __restrict__ out_act,
                                                       uint8_t* __restrict__ out_status, uint32_t xcd) {
    const uint32_t base = xcd_tile(blockIdx.x, gridDim.x, xcd) * (BLOCK * M) + threadIdx.x;
    uint64_t n1[M];
    uint4 q[M][CX8_GROUP / 2];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const uint32_t i = base + j * BLOCK;
        uint64_t n0 = 0, tcd = 0;
        n1[j] = 0;
        if (i < n) {
            const uint64_t* kp = reinterpret_cast<const uint64_t*>(keys + i);
            n0 = ld<NT>(kp);
            n1[j] = ld<NT>(kp + 1);
            tcd = ld<NT>(kp + 2);
        }
        const unsigned long long s = home_slot(uniform_hash(n0, n1[j], tcd), mask);
        const uint4* qp = cx8.slots + ((s & ~(unsigned long long)(CX8_GROUP - 1)) >> 1);
#pragma unroll
        for (int g = 0; g < (int)CX8_GROUP / 2; ++g) q[j][g] = qp[g];
    }
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const uint32_t i = base + j * BLOCK;
        uint32_t hit = 0;
#pragma unroll
        for (int k = 0; k < (int)CX8_GROUP; ++k) {
            const uint4 v = q[j][k / 2];
            const uint32_t x = (k & 1) ? v.z : v.x, y = (k & 1) ? v.w : v.y;
            if (hit == 0 && y != 0 && x == (uint32_t)n1[j]) hit = y;
        }
        if (i < n) {
            st<true>(out_silo + i, (hit >> cx8.ab) - 1u);
            out_act[i] = hit & ((1u << cx8.ab) - 1u);
            st<true>(out_status + i, (uint8_t)(hit == 0));
        }
    }
}

// The owner's probe over received chunks grouped by region (gd_route_multi with regions, SURVEY 8 e):
// workgroup b takes region g = b % 8.  Workgroups are dispatched round-robin over the 8 XCDs (b -> XCD
// b % 8), so all of one XCD's workgroups probe one eighth of the table (home_slot's top bits) and its
// 4-MB L2 serves that eighth alone (tools/ubench_random.hip: 16M probes of a 64-MB table 0.344 ->
// 0.224 ms).  The region's messages are W segments, one per sender (seg: k_region_segments); the
// G = gridDim.x / 8 workgroups of a region take its blocks of BLOCK messages grid-stride.
template <int MODE, int N1W>
static __global__ void __launch_bounds__(BLOCK) k_route_region(const gd_key* __restrict__ keys, uint32_t n, RingArgs ring,
                                                        TableArgs tab, uint32_t* __restrict__ out_silo,
                                                        uint32_t* __restrict__ out_act,
                                                        uint8_t* __restrict__ out_status, uint64_t tcd_u,
                                                        const uint32_t* __restrict__ seg, uint32_t world) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_ring[];
    __shared__ uint32_t s_beg[257], s_pre[257];
    uint32_t* s_pts = s_ring;
    uint32_t* s_own = s_ring + ring.n;
    const uint32_t g = blockIdx.x % N_REGIONS, G = gridDim.x / N_REGIONS;
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t q = 0; q < world; ++q) {
            const uint32_t b = seg[q * (N_REGIONS + 1) + g], e = seg[q * (N_REGIONS + 1) + g + 1];
            s_beg[q] = b;
            s_pre[q] = run;
            run += e - b;
        }
        s_pre[world] = run;
    }
    stage_ring(ring, s_pts, s_own);                   // its barrier publishes s_beg / s_pre too
    const uint32_t total = s_pre[world];
    const uint32_t max_probe = tab.ctr->max_probe;
    for (uint32_t k = blockIdx.x / N_REGIONS; k * BLOCK < total; k += G) {
        const uint32_t e = k * BLOCK + threadIdx.x;
        uint32_t i = n;                                // past the region: route_m_core skips it
        if (e < total) {
            uint32_t lo = 0, hi = world;               // largest q with s_pre[q] <= e
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_pre[mid] <= e) lo = mid;
                else hi = mid;
            }
            i = s_beg[lo] + (e - s_pre[lo]);
        }
        route_m_core<MODE, 1, BLOCK, false, N1W, true>(keys, n, i, ring, s_pts, s_own, tab, max_probe, out_silo,
                                                      out_act, out_status, tcd_u, nullptr, 0);
    }
}

// GetPrimaryTargetSilo(uint key) over raw ring keys.
template <int MODE>
static __global__ void __launch_bounds__(BLOCK) k_ring_hashes(const uint32_t* __restrict__ hashes, uint32_t n,
                                                       RingArgs ring, uint32_t* __restrict__ out_silo) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_ring[];
    uint32_t* s_pts = s_ring;
    uint32_t* s_own = s_ring + ring.n;
    stage_ring(ring, s_pts, s_own);
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    out_silo[i] = s_own[ring_position<MODE>(s_pts, ring.n, ring.top, hashes[i])];
}

}  // namespace gd
