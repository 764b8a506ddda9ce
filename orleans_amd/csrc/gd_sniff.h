// gd_sniff.h -- gfx950 device code for the sniff stage: batched InsideRuntimeClient.SniffIncomingMessage
// (InsideRuntimeClient.cs:253-263) -> LocalGrainDirectory.InvalidateCacheEntry (LocalGrainDirectory.cs:965-986) ->
// DirectoryCache.LookUp + RemoveActivations (:1146-1164) on the frames of a received batch.
//
// The CacheInvalidationHeader is the header's first field (Message.cs:1132-1140): int32 count, then per entry
// SiloAddress (24 B), GrainId UniqueKey (24 B + KeyExt string), ActivationId UniqueKey (24 B + KeyExt string) -- the
// field gd_forward.h's k_fwd_plan walks.  The stage walks nothing else of the frame.
//
//   k_sniff_count    one lane a frame, one wave a workgroup.  Every lane reads its frame's two lengths and mask (12 B)
//                    from global memory; a wave none of whose frames carries the header writes its outputs and ends
//                    there -- no staging, no walk.  Otherwise the frames that carry it are staged (the decoder's
//                    192-B windows, gd_frames.h; the windows of the other frames are not loaded) and their lanes
//                    walk the entries with HeaderWalk.  Writes count, status, flags, and count again into ent_off
//                    (ent_off[n] = 0) for the scan.
//   scan_device      exclusive, in place over ent_off[n + 1]: ent_off[n] = m.
//   k_sniff_extract  one lane a frame, the same cut: a wave none of whose frames has entries ends after two
//                    coalesced dwords a lane; a lane with entries walks them again and writes them at ent_off[i] + k
//                    as whole dwords into the SoA arrays.  m > ent_cap: nothing is written, ERR_SNIFF_FULL is raised.
//                    A lane-a-frame cut, not a lane-a-entry one: entry k starts where entry k - 1's two strings end,
//                    so a lane that owned entry k alone would walk entries 0 .. k - 1 first; and the counts are
//                    small (one entry a hop, MaxForwardCount hops).
//
// InvalidateCacheEntry for a batch of (grain, ActivationId) in batch order (gd_cache_invalidate*):
//   k_inv_find       the cache probe of k_cache_find a lane (cache_find_msg), the entry's class from the slot it
//                    found (the cached activation's ActivationId against the entry's), NumAccesses counted (the
//                    live count, less the keys the device cannot match), and atomicMin of k into first[slot] for the
//                    entries whose ActivationId matches.  first[] is a u32 word a cache slot, NONE32 between calls.
//   k_inv_resolve    entry k is a hit iff its slot was found and k <= first[slot] (the first matching entry removes
//                    the grain; the later ones miss): hit flags and slots for cache_touch, and out[k].
//   cache_touch      the existing scan + k_cache_touch + k_cache_advance: generations in batch order, NumAccesses++
//                    an entry, next_generation and NumHits advanced by the hit count.
//   k_inv_apply      the entry with k == first[slot] tombstones the slot as k_cache_apply does and puts first[slot]
//                    back to NONE32.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_cache.h"
#include "gd_frames.h"
#include "gd_hash.h"
#include "gd_keyext.h"

namespace gd {

// GD_SNIFF_* / GD_SNIFF_FLAG_* / GD_INV_* (include/graindispatch.h)
enum : uint32_t { SNIFF_NONE = 0, SNIFF_OK = 1, SNIFF_MALFORMED = 2 };
enum : uint32_t { SNIFF_FLAG_RETURNED = 1u, SNIFF_FLAG_UNKNOWN = 2u };
enum : uint32_t { INV_MISS = 0, INV_REMOVED = 1, INV_KEPT = 2, INV_HOST = 3, INV_NO_ID = 4 };
constexpr uint32_t H_IS_RETURNED_FROM_REMOTE_CLUSTER = 1u << 25;      // Message.cs:757
constexpr uint32_t ERR_SNIFF_FULL = 256u;    // DevCounters::err: the batch holds more than ent_cap entries
constexpr uint32_t SNIFF_BLOCK = WAVE;       // one wave a workgroup: the staging decision is the workgroup's

struct SniffOut {           // device pointers; nullptr = not wanted (count, ent_off and status required)
    uint32_t* count;
    uint32_t* ent_off;
    uint8_t* status;
    uint8_t* flags;
    uint32_t* ent_frame;
    uint32_t* ent_silo;     // 6 x u32 an entry (store_silo)
    uint64_t* ent_grain;    // 3 x u64 an entry (gd_key)
    uint64_t* ent_ext_off;
    int32_t* ent_ext_len;
    uint64_t* ent_act_id;
};

// The frame's headerLength, bodyLength and mask; false when the decoder's length conditions fail.  Fewer than 12
// bytes behind `start` is such a failure without a read: headerLength >= 4 needs them.
__device__ __forceinline__ bool sniff_head(const uint8_t* __restrict__ buf, uint64_t buf_len, uint64_t start,
                                           int32_t& hl, int32_t& bl, uint32_t& m) {
    hl = bl = 0;
    m = 0;
    if (start > buf_len || buf_len - start < 12) return false;
    const uint64_t a = start & ~3ull, dw_end = buf_len & ~3ull;
    uint32_t w0, w1, w2;
    if (a + 16 <= dw_end) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(buf + a);
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], sh = (uint32_t)(start & 3);
        w0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
        w1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
        w2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
    } else {                                                 // the buffer's last 16 bytes: byte loads
        const uint8_t* g = buf + start;
        uint32_t w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            w[k] = (uint32_t)g[4 * k] | ((uint32_t)g[4 * k + 1] << 8) | ((uint32_t)g[4 * k + 2] << 16) |
                   ((uint32_t)g[4 * k + 3] << 24);
        w0 = w[0], w1 = w[1], w2 = w[2];
    }
    hl = (int32_t)w0;
    bl = (int32_t)w1;
    m = w2;
    return !(hl < 4 || bl < 0 || (uint64_t)hl + (uint64_t)bl > buf_len - start - 8);
}

// The decoder's staging (gd_frames.h) for the frames of the wave whose bit is set in `want`: chunk q of the wave's
// 64 x 12 16-B chunks belongs to frame q / 12; clamped into [0, dw_end).  One wave a workgroup.
__device__ __forceinline__ void sniff_stage(const uint8_t* __restrict__ buf, uint64_t buf_len, uint64_t start,
                                            unsigned long long want, uint32_t (*s_win)[FRAME_ROW],
                                            unsigned long long* s_start) {
    const uint32_t lane = threadIdx.x;
    const uint64_t dw_end = buf_len & ~3ull;
    constexpr int CHUNKS = FRAME_WIN / 16;
    s_start[lane] = start;
    __syncthreads();
    if (dw_end >= 16) {
        uint4 v[CHUNKS];
#pragma unroll
        for (int it = 0; it < CHUNKS; ++it) {
            const uint32_t q = it * WAVE + lane, f = q / CHUNKS, c = q % CHUNKS;
            v[it] = make_uint4(0, 0, 0, 0);
            if ((want >> f) & 1ull) {
                const uint64_t a = (s_start[f] & ~3ull) + 16ull * c;
                v[it] = *(const uint4*)(buf + (a <= dw_end - 16 ? a : ((dw_end - 16) & ~3ull)));
            }
        }
#pragma unroll
        for (int it = 0; it < CHUNKS; ++it) {
            const uint32_t q = it * WAVE + lane, f = q / CHUNKS, c = q % CHUNKS;
            uint32_t* r = &s_win[f][4 * c];
            r[0] = v[it].x;
            r[1] = v[it].y;
            r[2] = v[it].z;
            r[3] = v[it].w;
        }
    }
    __syncthreads();
}

// The walker over a staged frame whose length conditions hold, in front of the invalidation count.
__device__ __forceinline__ void sniff_walk_init(HeaderWalk& hw, const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                uint64_t start, int32_t hl, const uint32_t* row) {
    const uint64_t dw_end = buf_len & ~3ull, a0 = start & ~3ull;
    constexpr int CHUNKS = FRAME_WIN / 16;
    uint64_t win_end = a0;
    if (dw_end >= 16 && dw_end > a0) {
        const uint64_t full = (dw_end - a0) / 16;
        win_end = a0 + 16 * (full < (uint64_t)CHUNKS ? full : (uint64_t)CHUNKS);
    }
    hw.c.row = row;
    hw.c.g = buf + start;
    hw.c.sh = (uint32_t)(start & 3);
    hw.c.lim = (start < win_end) ? (uint32_t)(win_end - start) : 0u;
    hw.bad = false;
    hw.p = 12;
    hw.end = 8u + (uint32_t)hl;
}

// ------------------------------------------------------------------ k_sniff_count
static __global__ __launch_bounds__(SNIFF_BLOCK) void k_sniff_count(const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                             const uint64_t* __restrict__ frame_off, uint32_t n,
                                                             SniffOut o) {
    __shared__ uint32_t s_win[WAVE][FRAME_ROW];
    __shared__ unsigned long long s_start[WAVE];
    const uint32_t i = blockIdx.x * SNIFF_BLOCK + threadIdx.x;
    const bool valid = i < n;
    const uint64_t start = frame_off[valid ? i : (n - 1)];
    int32_t hl, bl;
    uint32_t m;
    const bool good = sniff_head(buf, buf_len, start, hl, bl, m);
    const bool has = valid && good && (m & H_CACHE_INVALIDATION);
    uint32_t st = good ? SNIFF_NONE : SNIFF_MALFORMED, cnt = 0;
    const unsigned long long want = __ballot(has);
    if (want) {                                              // wave-uniform: the workgroup is one wave
        sniff_stage(buf, buf_len, start, want, s_win, s_start);
        if (has) {
            HeaderWalk hw;
            sniff_walk_init(hw, buf, buf_len, start, hl, s_win[threadIdx.x]);
            // the loop of k_fwd_plan (gd_forward.h): int32 count, then count x (SiloAddress, GrainId, ActivationId)
            if (hw.take(4)) {
                const int32_t c = (int32_t)hw.c.u32(12);
                if (c < 0) hw.bad = true;
                cnt = (uint32_t)c;
                for (uint32_t k = 0; k < cnt && !hw.bad; ++k) {      // an entry holds >= 80 B: the header bounds it
                    if (!hw.take(24)) break;
                    hw.key(nullptr);
                    hw.key(nullptr);
                }
            }
            st = hw.bad ? SNIFF_MALFORMED : SNIFF_OK;
            if (hw.bad) cnt = 0;
        }
    }
    if (!valid) return;
    o.count[i] = cnt;
    o.ent_off[i] = cnt;
    if (i == n - 1) o.ent_off[n] = 0;
    o.status[i] = (uint8_t)st;
    // IsReturnedFromRemoteCluster has no wire form in the reference: a frame whose mask sets its bit
    // is no frame the reference's serializer wrote, and C# decides
    if (o.flags) o.flags[i] = (uint8_t)((good && (m & H_IS_RETURNED_FROM_REMOTE_CLUSTER)) ? SNIFF_FLAG_UNKNOWN : 0u);
}

// ------------------------------------------------------------------ k_sniff_extract
static __global__ __launch_bounds__(SNIFF_BLOCK) void k_sniff_extract(const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                               const uint64_t* __restrict__ frame_off, uint32_t n,
                                                               SniffOut o, uint32_t ent_cap,
                                                               uint32_t* __restrict__ err) {
    __shared__ uint32_t s_win[WAVE][FRAME_ROW];
    __shared__ unsigned long long s_start[WAVE];
    const uint32_t total = o.ent_off[n];
    if (total > ent_cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, ERR_SNIFF_FULL);
        return;
    }
    const uint32_t i = blockIdx.x * SNIFF_BLOCK + threadIdx.x;
    const bool valid = i < n;
    const uint32_t e0 = valid ? o.ent_off[i] : 0u;
    const uint32_t cnt = valid ? o.ent_off[i + 1] - e0 : 0u;
    const unsigned long long want = __ballot(cnt != 0);
    if (!want) return;
    const uint64_t start = frame_off[valid ? i : (n - 1)];
    sniff_stage(buf, buf_len, start, want, s_win, s_start);
    if (!cnt) return;
    // cnt != 0: k_sniff_count found the frame well-formed and walked these entries inside its header
    int32_t hl, bl;
    uint32_t m;
    if (!sniff_head(buf, buf_len, start, hl, bl, m)) return;
    HeaderWalk hw;
    sniff_walk_init(hw, buf, buf_len, start, hl, s_win[threadIdx.x]);
    hw.p = 16;                                               // behind the count
    for (uint32_t k = 0; k < cnt && !hw.bad; ++k) {
        const uint32_t e = e0 + k;                           // < ent_off[i + 1] <= total <= ent_cap
        if (!hw.take(24)) break;
        const uint32_t ps = hw.p - 24;
        int32_t gx = -1, ax = -1;
        const Key3 g = hw.key(&gx);
        const uint32_t pg = hw.p;
        Key3 a = hw.key(&ax);
        if (hw.bad) break;
        if (ax >= 0) a = Key3{0, 0, 0};                      // an ActivationId with a KeyExt string equals no id of the map
        if (o.ent_frame) o.ent_frame[e] = i;
        if (o.ent_silo) {
#pragma unroll
            for (int j = 0; j < 6; ++j) o.ent_silo[6ull * e + j] = hw.c.u32(ps + 4 * j);
        }
        store_key(o.ent_grain, e, g);
        if (o.ent_ext_off) o.ent_ext_off[e] = start + pg - (uint32_t)(gx > 0 ? gx : 0);
        if (o.ent_ext_len) o.ent_ext_len[e] = gx;
        store_key(o.ent_act_id, e, a);
    }
}

// ------------------------------------------------------------------ InvalidateCacheEntry for a batch
struct InvArgs {
    const gd_key* keys;
    ExtArgs ext;                 // ext.len == nullptr: every key by its three words
    const gd_key* act_ids;
    uint32_t m;                  // the launch's size: the capacity of the arrays
    const uint32_t* d_m;         // the live count on the device, or nullptr: m
    const uint64_t* ids;         // the ActivationId map (gd_activation_ids_set): 3 x u64 an activation index
    uint64_t n_ids;
};

// Entries [0, live) are processed.  A device count above the capacity is the sniff stage's GD_EFULL: nothing is.
__device__ __forceinline__ uint32_t inv_live(uint32_t m, const uint32_t* d_m) {
    if (!d_m) return m;
    const uint32_t v = *d_m;
    return v <= m ? v : 0u;
}

static __global__ __launch_bounds__(BLOCK) void k_inv_find(InvArgs a, CacheArgs cache, uint32_t* __restrict__ first,
                                                    uint32_t* __restrict__ slot_of, uint8_t* __restrict__ cls,
                                                    CacheCounters* cctr) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t live = inv_live(a.m, a.d_m);
    // NumAccesses: every live entry but the few whose key the device cannot match.  One add of `live`, and one a wave
    // that holds such a key, not one a workgroup: adds to one address from every XCD serialise (gd_hash.h)
    if (i == 0 && live) atomicAdd(&cctr->accesses, (unsigned long long)live);
    bool access = true;
    if (i < live) {
        const uint64_t tcd = a.keys[i].type_code_data;
        bool can = true;                                     // a key the device can match (k_cache_lookup's rule)
        if (a.ext.len && is_keyext_tcd(tcd)) {
            const uint8_t* s;
            int32_t len;
            can = ext_of(a.ext, i, s, len);
        }
        uint32_t slot = NONE32, act = NONE32, meta = 0, c = INV_MISS;
        bool found = false;
        access = can;
        if (can) found = cache_find_msg(cache, a.keys, a.ext, i, slot, act, meta);
        if (found) {
            if (act == GD_ACT_MULTI) {
                c = INV_HOST;                                // the instance list is C#'s
            } else if (slot_silo(meta) == 0xFFFFu) {
                c = INV_KEPT;                                // the cached empty list: nothing to remove
            } else if ((uint64_t)act >= a.n_ids) {
                c = INV_NO_ID;
            } else {
                const uint64_t* id = a.ids + 3ull * act;
                const uint64_t i0 = id[0], i1 = id[1], i2 = id[2];
                if ((i0 | i1 | i2) == 0) {
                    c = INV_NO_ID;
                } else if (i0 == a.act_ids[i].n0 && i1 == a.act_ids[i].n1 && i2 == a.act_ids[i].type_code_data) {
                    c = INV_REMOVED;
                    atomicMin(&first[slot], i);
                } else {
                    c = INV_KEPT;
                }
            }
        }
        slot_of[i] = found ? slot : NONE32;
        cls[i] = (uint8_t)c;
    }
    const unsigned long long skipped = __ballot(!access);
    if ((threadIdx.x & (WAVE - 1)) == 0 && skipped)
        atomicAdd(&cctr->accesses, ~(unsigned long long)__popcll(skipped) + 1ull);       // minus the count, mod 2^64
}

static __global__ __launch_bounds__(BLOCK) void k_inv_resolve(uint32_t m, const uint32_t* __restrict__ d_m,
                                                       const uint32_t* __restrict__ slot_of,
                                                       const uint8_t* __restrict__ cls,
                                                       const uint32_t* __restrict__ first, uint32_t* __restrict__ hit,
                                                       uint32_t* __restrict__ cslot, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    if (i >= inv_live(m, d_m)) {                             // the scan runs over the capacity
        hit[i] = 0;
        cslot[i] = NONE32;
        return;
    }
    const uint32_t s = slot_of[i];
    const bool h = s != NONE32 && i <= first[s];
    hit[i] = h ? 1u : 0u;
    cslot[i] = h ? s : NONE32;
    out[i] = h ? cls[i] : (uint8_t)INV_MISS;
}

static __global__ __launch_bounds__(BLOCK) void k_inv_apply(uint32_t m, const uint32_t* __restrict__ d_m,
                                                     const uint32_t* __restrict__ slot_of,
                                                     const uint8_t* __restrict__ cls, uint32_t* first,
                                                     CacheSlot* slots, CacheCounters* ctr) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= inv_live(m, d_m) || cls[i] != INV_REMOVED) return;
    const uint32_t s = slot_of[i];
    if (first[s] != i) return;                               // a later matching entry of the same grain: a miss
    slots[s].meta = make_meta(SLOT_TOMB, 0);
    atomicAdd(&ctr->live, ~0ull);
    atomicAdd(&ctr->tomb, 1ull);
    first[s] = NONE32;
}

}  // namespace gd
