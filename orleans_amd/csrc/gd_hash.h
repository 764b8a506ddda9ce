// gd_hash.h -- what every kernel header of libgraindispatch starts from: the block constants, the device
// counters, the Jenkins hash of the 24-B GrainId (JenkinsHash.cs:85-105), the ring search over an
// LDS-staged snapshot (LocalGrainDirectory.cs:477-545 / ConsistentRingProvider.cs:322-372 /
// VirtualBucketsRingProvider.cs:257-293), the ring / table kernel arguments, and two workgroup helpers
// the route and the bucketing kernels share (xcd_tile, mb_mark).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_common.h"

namespace gd {

constexpr int WAVE = 64;
constexpr int BLOCK = 256;               // 4 waves
constexpr uint32_t NONE32 = 0xFFFFFFFFu;

struct DevCounters {
    uint32_t max_probe;     // largest probe distance of any entry placed so far
    uint32_t err;           // bit 1: table full
    uint32_t retry;         // items k_reg_claim deferred to a relaunch
    uint32_t pad;
    unsigned long long live;
    unsigned long long tomb;
};
// Striped deltas of live / tomb behind the counters (one allocation of CTR_BYTES): the directory batches'
// kernels add a wave's (or workgroup's) count into stripe blockIdx % CTR_STRIPES, 256 B apart, instead of
// into DevCounters itself -- device-scope atomics on one address from every XCD serialise (cfg 3's 1M-item
// batches: 1.6 of their 2.0 ms a churn step).  k_ctr_fold adds the stripes into live / tomb (and zeroes
// them) before every read-back (pull_counters).
constexpr uint32_t CTR_STRIPES = 64;
constexpr uint32_t CTR_STRIPE_U64 = 32;       // 256 B a stripe: {live delta, tomb delta, unused}
constexpr size_t CTR_HDR = 256;
constexpr size_t CTR_BYTES = CTR_HDR + (size_t)CTR_STRIPES * CTR_STRIPE_U64 * 8;
static_assert(sizeof(DevCounters) <= CTR_HDR, "counters header");
__device__ __forceinline__ unsigned long long* ctr_stripe(DevCounters* ctr) {
    return reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ctr) + CTR_HDR) +
           (size_t)(blockIdx.x % CTR_STRIPES) * CTR_STRIPE_U64;
}
static __global__ void __launch_bounds__(64) k_ctr_fold(DevCounters* ctr) {
    unsigned long long* s = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ctr) + CTR_HDR) +
                            (size_t)threadIdx.x * CTR_STRIPE_U64;
    unsigned long long l = 0, t = 0;
    if (threadIdx.x < CTR_STRIPES) {
        l = s[0];
        t = s[1];
        s[0] = 0;
        s[1] = 0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        l += __shfl_xor(l, off, 64);
        t += __shfl_xor(t, off, 64);
    }
    if (threadIdx.x == 0) {
        ctr->live += l;
        ctr->tomb += t;
    }
}

// ------------------------------------------------------------------ identity
__device__ __forceinline__ void jmix(uint32_t& a, uint32_t& b, uint32_t& c) {
    a -= b; a -= c; a ^= (c >> 13);
    b -= c; b -= a; b ^= (a << 8);
    c -= a; c -= b; c ^= (b >> 13);
    a -= b; a -= c; a ^= (c >> 12);
    b -= c; b -= a; b ^= (a << 16);
    c -= a; c -= b; c ^= (b >> 5);
    a -= b; a -= c; a ^= (c >> 3);
    b -= c; b -= a; b ^= (a << 10);
    c -= a; c -= b; c ^= (b >> 15);
}

// UniqueKey.GetUniformHashCode = JenkinsHash.ComputeHash(TypeCodeData, N0, N1)
// (UniqueKey.cs:285; JenkinsHash.cs:85-105).
__device__ __forceinline__ uint32_t uniform_hash(uint64_t n0, uint64_t n1, uint64_t tcd) {
    uint32_t a = 0x9e3779b9u, b = a, c = 0;
    a += (uint32_t)tcd;
    b += (uint32_t)(tcd >> 32);
    c += (uint32_t)n0;
    jmix(a, b, c);
    a += (uint32_t)(n0 >> 32);
    b += (uint32_t)n1;
    c += (uint32_t)(n1 >> 32);
    jmix(a, b, c);
    c += 24;
    jmix(a, b, c);
    return c;
}

// ------------------------------------------------------------------ ring
// Count of the prefix of the ring satisfying the mode's monotone predicate,
// by a branch-free power-of-two search over the LDS copy.
template <int MODE>
__device__ __forceinline__ bool ring_pred(uint32_t p, uint32_t h) {
    if constexpr (MODE == GD_RING_DIRECTORY) {
        // IsSiloNextInTheRing: siloHash <= (int)grainHash (LocalGrainDirectory.cs:1141-1144)
        return (int32_t)p <= (int32_t)h;
    } else if constexpr (MODE == GD_RING_CONSISTENT) {
        // complement of (long)siloHash >= (long)key (ConsistentRingProvider.cs:369-372)
        return (int32_t)p < 0 || p < h;
    } else {
        // complement of point >= key, uint (VirtualBucketsRingProvider.cs:276)
        return p < h;
    }
}

template <int MODE>
__device__ __forceinline__ uint32_t ring_position(const uint32_t* pts, uint32_t n, uint32_t top, uint32_t h) {
    uint32_t cnt = 0;
    for (uint32_t step = top; step > 0; step >>= 1) {
        const uint32_t c = cnt + step;
        if (c <= n && ring_pred<MODE>(pts[c - 1], h)) cnt = c;
    }
    if constexpr (MODE == GD_RING_DIRECTORY) {
        // scan from the end for the first match; none -> last silo (:521-538)
        return cnt == 0 ? n - 1 : cnt - 1;
    } else {
        // scan from the start for the first match; none -> first (:341-352 / :279-289)
        return cnt == n ? 0 : cnt;
    }
}

struct RingArgs {
    const uint32_t* pts;
    const uint32_t* own;
    uint32_t n;
    uint32_t top;       // highest power of two <= n
    uint32_t my_silo;
    uint32_t seed_silo;
};

struct TableArgs {
    const Slot* slots;
    unsigned long long mask;
    const DevCounters* ctr;
    const uint32_t* valid;     // IsValidSilo bitset over silo indices [0, n_valid) (gd_dir_set_valid_silos)
    uint32_t n_valid;          // 0: every silo valid
};

// GrainDirectoryPartition.IsValidSilo (GrainDirectoryPartition.cs:242-245): silos outside the
// configured range count as valid.
__device__ __forceinline__ bool valid_silo(const uint32_t* valid, uint32_t n_valid, uint32_t silo) {
    return n_valid == 0 || silo >= n_valid || ((valid[silo >> 5] >> (silo & 31u)) & 1u);
}
__device__ __forceinline__ bool tab_silo_valid(const TableArgs& t, uint32_t silo) {
    return valid_silo(t.valid, t.n_valid, silo);
}

// VersionTag side array (one u32 per table slot): bits 0..30 the tag (the reference draws
// rand.Next() on every change, GrainDirectoryPartition.cs:106,120,135,154; here a deterministic
// function of the change's sequence number and the grain), bit 31 = GrainInfo.SingleInstance.
constexpr uint32_t VTAG_SINGLE = 0x80000000u;
__device__ __host__ __forceinline__ uint32_t version_tag(uint32_t op, uint32_t h) {
    return fmix32(h ^ (op * 0x9E3779B9u)) & 0x7FFFFFFFu;
}

__device__ __forceinline__ void stage_ring(const RingArgs& r, uint32_t* s_pts, uint32_t* s_own) {
    for (uint32_t i = threadIdx.x; i < r.n; i += blockDim.x) {
        s_pts[i] = r.pts[i];
        s_own[i] = r.own[i];
    }
    __syncthreads();
}

__device__ __forceinline__ bool is_membership(uint64_t n0, uint64_t n1, uint64_t tcd) {
    return n0 == MEMBERSHIP_N0 && n1 == MEMBERSHIP_N1 && tcd == MEMBERSHIP_TCD;
}

// Workgroups are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8), each with its own
// L2.  With xcd != 0 block b processes tile start(b % 8) + b / 8, so every XCD owns a contiguous
// tile range: the digit-run fragments that consecutive tiles write next to each other in the
// output meet in one L2 instead of being written back as partial lines by two.
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t nb, uint32_t xcd) {
    if (!xcd) return b;
    const uint32_t x = b & 7u, k = b >> 3, q = nb >> 3, rem = nb & 7u;
    return x * q + min(x, rem) + k;
}

// GD_MB_TRACE: workgroup 0, thread 0 adds phase durations (100-MHz wall clock ticks) into ts[]
__device__ __forceinline__ void mb_mark(unsigned long long* ts, int k, unsigned long long& t) {
    if (ts && blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long now = wall_clock64();
        if (k > 0) atomicAdd(ts + k, now - t);
        t = now;
    }
}

}  // namespace gd
