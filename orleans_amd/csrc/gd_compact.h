// gd_compact.h -- the compact route: messages given as (class id, N1) records, results packed
// as act u32 / silo u16 / status u8.  A record is the key {N0 = 0, N1, TypeCodeData = classes[cls]}: the
// kernel forms it in registers from a class table staged in LDS beside the ring and takes the same probe
// forms as the 24-B route (gd_route.h) through the same device functions (gd_hash.h, gd_probe.h).
#pragma once
#include "gd_route.h"

namespace gd {

constexpr uint32_t COMPACT_CLASSES = 256;      // class ids are one byte
constexpr uint32_t NO_SILO16 = 0xFFFFu;        // GD_NO_SILO16
constexpr uint8_t ROUTE_BAD_CLASS = 8;         // GD_ROUTE_BAD_CLASS

// The probe form of a launch: the 24-B route's own (route_form, eng_route.hip).
enum CompactForm : int {
    CF_DIRECTORY = 0,      // the directory table
    CF_INDEX16 = 1,        // the 16-B index, one 64-B group a read
    CF_INDEX16_SLOT = 2,   // the 16-B index, one slot a read
    CF_INDEX8 = 3,         // the 8-B index, the directory behind it
    CF_INDEX8_PURE = 4,    // the pure 8-B index: no directory behind it
    CF_DIRECT = 5,         // the direct table standing in for the pure 8-B index
};

// The packed silo: GD_NO_SILO -> NO_SILO16; an index that does not fit (0xFFFF..0xFFFFFFFE) -> NO_SILO16
// and *wide set.
__host__ __device__ __forceinline__ uint32_t pack_silo16(uint32_t silo, bool& wide) {
    wide = silo >= NO_SILO16 && silo != NONE32;
    return silo >= NO_SILO16 ? NO_SILO16 : silo;
}

// A wave's count of silos too wide for 16 bits: one atomic a wave that has any (none, normally).
__device__ __forceinline__ void count_wide(bool wide, uint32_t* __restrict__ n_wide) {
    const unsigned long long b = __ballot(wide);
    if (b != 0 && n_wide != nullptr && (threadIdx.x & (WAVE - 1)) == 0) atomicAdd(n_wide, (uint32_t)__popcll(b));
}

// One record a thread: a wave reads 64 consecutive class bytes and N1s and writes 64 consecutive acts (256 B,
// temporal: the bucketing's histogram reads them next), silos (128 B) and statuses (64 B), whole runs each.
// cls == nullptr: every message is class 0.  NT: the record streams are read non-temporally (route_mode's
// rule); silo / status are always written so, as k_route_m does.  xcd: XCD-contiguous message ranges.
template <int MODE, bool NT, int N1W, int FORM>
static __global__ void __launch_bounds__(BLOCK) k_route_compact(
    const uint8_t* __restrict__ cls, const void* __restrict__ n1s, uint32_t n,
    const unsigned long long* __restrict__ classes, uint32_t n_cls, RingArgs ring, TableArgs tab,
    uint32_t* __restrict__ out_act, uint16_t* __restrict__ out_silo16, uint8_t* __restrict__ out_status,
    uint32_t* __restrict__ n_wide, uint32_t xcd, CxArgs cx, Cx8Args cx8, CxdArgs d) {
    static_assert(N1W == 4 || N1W == 8, "N1 as u32 or u64");
    constexpr bool CX = FORM == CF_INDEX16 || FORM == CF_INDEX16_SLOT;
    constexpr bool CX8 = FORM == CF_INDEX8 || FORM == CF_INDEX8_PURE;
    constexpr bool PURE = FORM == CF_INDEX8_PURE;
    extern __shared__ __attribute__((aligned(16))) uint32_t s_ring[];
    __shared__ unsigned long long s_cls[COMPACT_CLASSES];
    __shared__ unsigned long long s_types[CX ? CX_TYPES : 1];
    __shared__ uint32_t s_mp;
    uint32_t* s_pts = s_ring;
    uint32_t* s_own = s_ring + ring.n;
    for (uint32_t t = threadIdx.x; t < n_cls; t += BLOCK) s_cls[t] = classes[t];
    if constexpr (CX)
        for (uint32_t t = threadIdx.x; t < CX_TYPES; t += BLOCK) s_types[t] = cx.types[t];
    if (PURE && threadIdx.x == 0) s_mp = lazy_max_probe(tab);
    stage_ring(ring, s_pts, s_own);                    // its barrier publishes s_cls, s_types and s_mp too

    const uint32_t i = xcd_tile(blockIdx.x, gridDim.x, xcd) * BLOCK + threadIdx.x;
    const bool in = i < n;
    uint32_t c = 0;
    uint64_t n1 = 0;
    if (in) {
        if (cls) c = ld<NT>(cls + i);
        if constexpr (N1W == 8) n1 = ld<NT>(reinterpret_cast<const uint64_t*>(n1s) + i);
        else n1 = ld<NT>(reinterpret_cast<const uint32_t*>(n1s) + i);
    }
    const bool live = in && c < n_cls;                 // else: past the batch, or GD_ROUTE_BAD_CLASS
    const uint64_t tcd = live ? s_cls[c] : 0;
    const uint32_t cat = (uint32_t)(tcd >> 56);

    uint32_t y = 0;                                    // CF_DIRECT: the table word, in flight before the class checks
    if constexpr (FORM == CF_DIRECT)
        if (live && tcd == d.tcd && n1 < (uint64_t)d.d) y = d.tab[(uint32_t)n1];

    uint32_t silo = NONE32, act = NONE32;
    uint8_t status = ROUTE_BAD_CLASS;
    if (!live) {
    } else if (cat == CAT_SYSTEM_TARGET) {                        // LocalGrainDirectory.cs:480-485
        silo = ring.my_silo;
        status = GD_ROUTE_SYSTEM_TARGET;
    } else if (is_membership(0, n1, tcd)) {                       // :487-503
        silo = ring.seed_silo;
        status = GD_ROUTE_MEMBERSHIP;
    } else if (cat == CAT_KEYEXT_GRAIN || cat == CAT_GEO_CLIENT) {  // UniqueKey.cs:279-281
        status = GD_ROUTE_KEYEXT;
    } else if constexpr (FORM == CF_DIRECT) {
        silo = 0;
        status = GD_ROUTE_MISS;
        if (y != 0) cx8_decode(d.ab, d.sb, tab, y, silo, act, status);
        if (status != GD_ROUTE_OK)                                // the owner silo: hash and ring search, these lanes only
            silo = s_own[ring_position<MODE>(s_pts, ring.n, ring.top, uniform_hash(0, n1, tcd))];
    } else {
        const uint32_t h = uniform_hash(0, n1, tcd);
        status = GD_ROUTE_MISS;
        bool fb = !(CX || CX8);                                   // probe the directory itself
        if constexpr (CX || CX8) {
            // the index walk of route_m_core: a lane whose key the index does not hold (fb) falls back to the
            // directory by itself
            constexpr int QW = CX ? (FORM == CF_INDEX16 ? (int)CX_GROUP : 1) : (int)CX8_GROUP / 2;
            const unsigned long long s = home_slot(h, tab.mask);
            uint32_t want;
            if constexpr (CX) {
                const int t = cx_type_index(s_types, tcd);
                want = t < 0 ? 0u : (0x100u | (uint32_t)t);
            } else {
                const int t = cx8_type(cx8, 0, n1, tcd);
                want = t < 0 ? 0u : 1u + (uint32_t)t;
            }
            fb = !PURE && want == 0;
            uint4 q[QW];
            if (want) {
                const uint4* qp;
                if constexpr (CX) qp = cx.slots + (s & ~(unsigned long long)(QW - 1));
                else qp = cx8.slots + ((s & ~(unsigned long long)(CX8_GROUP - 1)) >> 1);
#pragma unroll
                for (int g = 0; g < QW; ++g) q[g] = qp[g];
            }
            silo = s_own[ring_position<MODE>(s_pts, ring.n, ring.top, h)];   // the ring search (LDS) under the read
            if (want) {
                if constexpr (CX) cx16_walk<QW>(cx, tab, want, n1, s, q, silo, act, status);
                else if constexpr (PURE) cx8_walk_pure(cx8, tab, (uint32_t)n1, s, q, s_mp, silo, act, status);
                else fb = cx8_walk(cx8, tab, (uint32_t)n1, want - 1u, s, q, silo, act, status);
            }
        } else {
            silo = s_own[ring_position<MODE>(s_pts, ring.n, ring.top, h)];
        }
        if (fb) {
            uint32_t a, meta;
            if (probe(tab.slots, tab.mask, lazy_max_probe(tab), h, 0, n1, tcd, a, meta))
                entry_result(tab, a, slot_silo(meta), silo, act, status);    // else MISS (Dispatcher.cs:742)
        }
    }
    bool wide;
    const uint32_t s16 = pack_silo16(silo, wide);
    if (in) {
        out_act[i] = act;                                         // the bucketing's input, next (temporal)
        st<true>(out_silo16 + i, (uint16_t)s16);                  // silo / status: not read again on the device
        st<true>(out_status + i, status);
    }
    count_wide(in && wide, n_wide);
}

// ---- the simple form (LocalLookup mode): records -> 24-B keys, the cache route, routes -> packed
// A record's key into the key scratch.  An out-of-range class gets a SystemTarget-category key: the cache
// route neither looks it up nor counts an access for it, and k_compact_pack gives it GD_ROUTE_BAD_CLASS.
template <int N1W>
static __global__ void __launch_bounds__(BLOCK) k_compact_expand(const uint8_t* __restrict__ cls,
                                                          const void* __restrict__ n1s, uint32_t n,
                                                          const unsigned long long* __restrict__ classes,
                                                          uint32_t n_cls, gd_key* __restrict__ keys) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cls ? cls[i] : 0u;
    uint64_t n1;
    if constexpr (N1W == 8) n1 = reinterpret_cast<const uint64_t*>(n1s)[i];
    else n1 = reinterpret_cast<const uint32_t*>(n1s)[i];
    uint64_t* kp = reinterpret_cast<uint64_t*>(keys + i);
    kp[0] = 0;
    kp[1] = n1;
    kp[2] = c < n_cls ? classes[c] : (uint64_t)CAT_SYSTEM_TARGET << 56;
}

static __global__ void __launch_bounds__(BLOCK) k_compact_pack(const uint8_t* __restrict__ cls, uint32_t n,
                                                        uint32_t n_cls, const uint32_t* __restrict__ silo,
                                                        uint32_t* __restrict__ act,
                                                        uint16_t* __restrict__ out_silo16,
                                                        uint8_t* __restrict__ status,
                                                        uint32_t* __restrict__ n_wide) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool wide = false;
    if (i < n) {
        uint32_t s = silo[i];
        if (cls && cls[i] >= n_cls) {
            s = NONE32;
            act[i] = NONE32;
            status[i] = ROUTE_BAD_CLASS;
        }
        out_silo16[i] = (uint16_t)pack_silo16(s, wide);
    }
    count_wide(wide, n_wide);
}

}  // namespace gd
