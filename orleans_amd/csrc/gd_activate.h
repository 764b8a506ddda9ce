// gd_activate.h -- gfx950 device code for the activation stage: what the null-context closure of
// Dispatcher.ReceiveMessage (Core/Dispatcher.cs:75-201) does before ReceiveRequest / ReceiveResponse, for a
// received batch: IsExpired (:79-85), then Catalog.GetOrCreateActivation (Catalog/Catalog.cs:443-518) under
// lock (activations) -- TryGetActivationData, or a new ActivationData recorded in the ActivationDirectory
// (RegisterMessageTarget -> RecordNewTarget, Catalog/ActivationDirectory.cs:86-93) when the message carries
// IsNewPlacement, or NonExistentActivationException.
//
// Only the messages gd_receive left GD_RECV_NULL_CONTEXT take part.  The rule is sequential in arrival order; its
// closed form, for an ActivationId absent when the batch starts, with f = the arrival index of its first
// non-expired candidate (IsNewPlacement, silo not terminating): non-expired messages before f (all of them without
// an f) are NONEXISTENT(_RESPONSE), f is CREATED, non-expired messages after f are FOUND with f's proposal.  The
// k-th candidate of the batch proposes new_ctx[k] (or ctx_base + k): proposals are sparse, as gd_route_place's.
//
// Nothing is created by a path that would need a claim to be taken back:
//   k_actv_classify  thread t of a tile holds 16 consecutive messages: one 16-B load of their receive statuses.
//                    Only a NULL_CONTEXT message loads its ttl (8 B), ActivationId (24 B), direction and
//                    IsNewPlacement bytes and probes (ad_find, one 64-B read).  Final kinds: NONE, EXPIRED, FOUND,
//                    HOST; an absent id leaves the provisional byte AV_PENDING | its NONEXISTENT kind | AV_CAND.
//                    ctx / status are copied through unless they alias the outputs; the tile's candidate count.
//   scan_device, k_actv_gather   the candidates in arrival order: idx[k], key[k], proposal[k] (k < cap_new); a
//                    proposal >= n_ctx raises the `bad` word.
//   k_actv_gate      one workgroup: n_proposed, and the gate word iff n_cand <= cap_new and no proposal was bad.
//                    Every later kernel runs under the gate.
//   k_actv_claim     the TryAdd claim protocol (claim_walk, gd_dirbatch.h) over the compacted candidates, on the
//                    activation directory's table and its election words (~k: the lowest candidate index of a slot
//                    holds the word).  Only candidates claim, so every claim has an elected item and commits.
//   k_actv_commit    the elected candidate of a slot writes {proposal, flags 0}: ActivationState.Create.  The word
//                    stays: it names the creator until the call ends.
//   k_actv_resolve   the tile walk again over the kind bytes: a pending message probes once more and compares its
//                    index with the creator's (idx[~word]): CREATED, FOUND or its NONEXISTENT kind; a closed gate
//                    gives HOST.  The tile's CREATED and NONEXISTENT counts.
//   scan_device, k_actv_list     new_idx / gone_idx: two stable compactions.
//   k_actv_clear     zeroes the election words of the candidates' slots.
// A message that does not take part costs its status byte in k_actv_classify and its kind byte in k_actv_resolve
// and k_actv_list, plus the copied outputs: no key read, no probe.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_actdir.h"
#include "gd_dirbatch.h"
#include "gd_frames.h"
#include "gd_place.h"
#include "gd_scan.h"
#include "graindispatch.h"

namespace gd {

// GD_ACTV_* (include/graindispatch.h)
enum : uint32_t {
    ACTV_NONE = 0, ACTV_FOUND = 1, ACTV_CREATED = 2, ACTV_EXPIRED = 3, ACTV_HOST = 4, ACTV_NONEXISTENT = 5,
    ACTV_NONEXISTENT_RESPONSE = 6
};
// provisional kind bytes between k_actv_classify and k_actv_resolve: the low bits hold the NONEXISTENT kind
constexpr uint32_t AV_PENDING = 0x80u, AV_CAND = 0x40u, AV_KIND = 0x3Fu;
constexpr uint32_t AV_WIDE_BYTES = 1u, AV_WIDE_CTX = 2u;    // the 1-B arrays / the ctx arrays are 16-B aligned

struct ActvIn {
    const uint32_t* ctx;
    const uint8_t* rs;
    const gd_key* ta;
    const uint8_t* dir;        // nullable: every message a Request
    const int64_t* ttl;        // nullable: none
    const uint8_t* newp;       // nullable: all 0
    int64_t ttl_age;           // the frame-fed chain's age (TurnFrameAdj), 0 otherwise
    uint32_t n, n_ctx, terminating;
};

// The call's device words: zero when the call starts.
struct ActvWords {
    uint32_t gate;             // 1: the batch is not refused
    uint32_t bad;              // a proposal >= n_ctx
    uint32_t n_cand;
    uint32_t pad;
    uint32_t retry[REG_PASSES];
};

// Bit r set: byte r of the 16 has every bit of `bits`.
__device__ __forceinline__ uint32_t av_bits_mask(const uint32_t (&w)[4], uint32_t bits) {
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < PL_IT; ++r) m |= ((((w[r >> 2] >> (8 * (r & 3))) & bits) == bits) ? 1u : 0u) << r;
    return m;
}

__device__ __forceinline__ void av_store16(uint8_t* __restrict__ p, uint32_t i0, uint32_t n, bool wide,
                                           const uint32_t (&w)[4]) {
    if (wide && i0 + PL_IT <= n) {
        *reinterpret_cast<uint4*>(p + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (uint32_t r = 0; r < (uint32_t)PL_IT && i0 + r < n; ++r) p[i0 + r] = (uint8_t)(w[r >> 2] >> (8 * (r & 3u)));
    }
}

// The tile's sum of a thread's small count into cnt[blockIdx.x]; cnt[tiles] = 0 (the scan's total lands there).
__device__ __forceinline__ void av_tile_count(uint32_t c, uint32_t* s_wcnt, uint32_t* __restrict__ cnt, uint32_t tiles) {
    uint32_t total;
    (void)pl_wave_prefix(c, lane_id(), total);
    if (lane_id() == 0) s_wcnt[threadIdx.x / WAVE] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < PL_NW; ++w) t += s_wcnt[w];
        cnt[blockIdx.x] = t;
        if (blockIdx.x == 0) cnt[tiles] = 0;
    }
}

static __global__ void __launch_bounds__(PL_NT) k_actv_classify(ActvIn a, AdArgs t, uint32_t wide,
                                                         uint8_t* __restrict__ kind, uint32_t* ctx_out,
                                                         uint8_t* st_out, uint32_t* __restrict__ tile_cnt,
                                                         uint32_t tiles, uint32_t* __restrict__ err) {
    __shared__ uint32_t s_wcnt[PL_NW];
    const uint32_t i0 = blockIdx.x * PL_TILE + threadIdx.x * PL_IT;
    const bool wb = wide & AV_WIDE_BYTES;
    uint32_t sw[4];
    pl_load16(a.rs, i0, a.n, wb, (uint32_t)RECV_UNDECODED, sw);
    if (ctx_out != a.ctx) {                              // the copy-through, ahead of the FOUND lanes' stores
        if ((wide & AV_WIDE_CTX) && i0 + PL_IT <= a.n) {
            const uint4* s = reinterpret_cast<const uint4*>(a.ctx + i0);
            uint4* d = reinterpret_cast<uint4*>(ctx_out + i0);
            const uint4 v0 = s[0], v1 = s[1], v2 = s[2], v3 = s[3];
            d[0] = v0; d[1] = v1; d[2] = v2; d[3] = v3;
        } else {
            for (uint32_t r = 0; r < (uint32_t)PL_IT && i0 + r < a.n; ++r) ctx_out[i0 + r] = a.ctx[i0 + r];
        }
    }
    uint32_t kw[4] = {0, 0, 0, 0};                       // ACTV_NONE
    uint32_t cnt = 0;
    bool found_any = false;
    for (uint32_t m = pl_eq_mask(sw, RECV_NULL_CONTEXT); m; m &= m - 1u) {
        const uint32_t r = (uint32_t)__ffs((int)m) - 1u, i = i0 + r;
        int64_t tv = a.ttl ? a.ttl[i] : GD_TTL_NONE;
        if (tv != GD_TTL_NONE && a.ttl_age) tv = tv < INT64_MIN + a.ttl_age ? INT64_MIN : tv - a.ttl_age;
        uint32_t k;
        if (tv != GD_TTL_NONE && tv <= 0) {              // Message.IsExpired, before GetOrCreateActivation
            k = ACTV_EXPIRED;
        } else {
            const uint64_t* kp = reinterpret_cast<const uint64_t*>(a.ta + i);
            uint32_t c = NONE32, fl = 0;
            if (ad_find(t, kp[0], kp[1], kp[2], c, fl)) {
                if (fl & AD_SYSTEM_TARGET) {
                    k = ACTV_HOST;                       // the reference's other dictionary: C# decides
                } else if (c >= a.n_ctx) {
                    atomicOr(err, ERR_CTX_RANGE);
                    k = ACTV_HOST;
                } else {
                    k = ACTV_FOUND;                      // TryGetActivationData, in whatever state
                    ctx_out[i] = c;
                    sw[r >> 2] = (sw[r >> 2] & ~(0xFFu << (8 * (r & 3u)))) | ((uint32_t)RECV_ACTIVATION << (8 * (r & 3u)));
                    found_any = true;
                }
            } else {
                uint32_t d = a.dir ? (uint32_t)a.dir[i] : 0u;
                const bool cand = !a.terminating && a.newp && a.newp[i] == 1;
                k = AV_PENDING | (d == DIR_RESPONSE ? ACTV_NONEXISTENT_RESPONSE : ACTV_NONEXISTENT) | (cand ? AV_CAND : 0u);
                cnt += cand ? 1u : 0u;
            }
        }
        kw[r >> 2] |= k << (8 * (r & 3u));
    }
    av_store16(kind, i0, a.n, wb, kw);
    if (st_out != a.rs || found_any) av_store16(st_out, i0, a.n, wb, sw);
    av_tile_count(cnt, s_wcnt, tile_cnt, tiles);
}

// tile_off: the exclusive scan of k_actv_classify's counts.  Candidate k < m_cap -> idx[k], keys[k], prop[k]; the
// candidates past m_cap (the batch is refused) are not written.
static __global__ void __launch_bounds__(PL_NT) k_actv_gather(const uint8_t* __restrict__ kind,
                                                       const gd_key* __restrict__ ta, uint32_t n, uint32_t n_ctx,
                                                       uint32_t wide, const uint32_t* __restrict__ tile_off,
                                                       const uint32_t* __restrict__ new_ctx, uint32_t ctx_base,
                                                       uint32_t m_cap, uint32_t* __restrict__ idx,
                                                       gd_key* __restrict__ keys, uint32_t* __restrict__ prop,
                                                       ActvWords* __restrict__ w) {
    __shared__ uint32_t s_wcnt[PL_NW];
    const uint32_t tile_base = tile_off[blockIdx.x];
    if (tile_off[blockIdx.x + 1] == tile_base) return;   // the whole workgroup
    const uint32_t i0 = blockIdx.x * PL_TILE + threadIdx.x * PL_IT;
    uint32_t kw[4];
    pl_load16(kind, i0, n, wide & AV_WIDE_BYTES, (uint32_t)ACTV_NONE, kw);
    uint32_t pend = av_bits_mask(kw, AV_PENDING | AV_CAND);
    const uint32_t lane = lane_id(), wv = threadIdx.x / WAVE;
    uint32_t total;
    const uint32_t pre = pl_wave_prefix((uint32_t)__popc(pend), lane, total);
    if (lane == 0) s_wcnt[wv] = total;
    __syncthreads();
    uint32_t j = tile_base + pre;
#pragma unroll
    for (int k = 0; k < PL_NW; ++k)
        if ((uint32_t)k < wv) j += s_wcnt[k];
    for (; pend; pend &= pend - 1u, ++j) {
        if (j >= m_cap) break;
        const uint32_t i = i0 + ((uint32_t)__ffs((int)pend) - 1u);
        const uint32_t p = new_ctx ? new_ctx[j] : ctx_base + j;
        idx[j] = i;
        keys[j] = ta[i];
        prop[j] = p;
        if (p >= n_ctx) atomicOr(&w->bad, 1u);
    }
}

// One workgroup.  n_cand: the scan's total.
static __global__ void __launch_bounds__(WAVE) k_actv_gate(const uint32_t* __restrict__ n_cand, uint32_t cap_new,
                                                    ActvWords* __restrict__ w, uint32_t* __restrict__ n_proposed,
                                                    uint32_t* __restrict__ err) {
    if (threadIdx.x != 0) return;
    const uint32_t nc = *n_cand;
    *n_proposed = nc;
    w->n_cand = nc;
    if (w->bad) atomicOr(err, ERR_CTX_RANGE);            // as gd_receive's: the call fails with GD_EINVAL
    w->gate = (nc <= cap_new && !w->bad) ? 1u : 0u;
}

// A claim pass over the candidates.  gate_retry (gated passes): the previous pass's deferred count.
static __global__ void __launch_bounds__(BLOCK) k_actv_claim(const gd_key* __restrict__ keys,
                                                      const ActvWords* __restrict__ w, Slot* slots,
                                                      unsigned long long mask, DevCounters* ctr, uint32_t* err,
                                                      uint32_t* __restrict__ slot_of, uint8_t* __restrict__ is_new,
                                                      uint32_t pass, const uint32_t* __restrict__ gate_retry,
                                                      uint32_t* retry, uint32_t* __restrict__ last) {
    if (!w->gate || (gate_retry && *gate_retry == 0)) return;
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pd = 0;
    bool reused = false;
    if (j < w->n_cand && (pass == 0 || slot_of[j] == SLOT_RETRY)) {
        (void)claim_walk(DirSlots{slots, mask}, j, keys, err, slot_of, is_new, retry, pd, reused, claim_tag(pass), last);
        if (is_new[j]) atomicMax(&last[slot_of[j]], ~j);     // the election: the lowest arrival index creates
    }
    claim_counters(ctr, pd, reused);
}

// unsettled (gated passes): the last pass's deferred count.
static __global__ void __launch_bounds__(BLOCK) k_actv_commit(const ActvWords* __restrict__ w,
                                                       const uint32_t* __restrict__ slot_of,
                                                       const uint8_t* __restrict__ is_new,
                                                       const uint32_t* __restrict__ prop, Slot* slots, DevCounters* ctr,
                                                       const uint32_t* __restrict__ last,
                                                       const uint32_t* __restrict__ unsettled, uint32_t* err) {
    if (!w->gate) return;
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j == 0 && unsettled && *unsettled) atomicOr(err, ERR_UNSETTLED);
    bool win = false;
    if (j < w->n_cand && is_new[j]) {
        const uint32_t s = slot_of[j];
        win = s < SLOT_RETRY && last[s] == ~j;
        if (win) {
            slots[s].act = prop[j];
            slots[s].meta = make_meta(SLOT_LIVE, 0);     // not Valid, no system target, no stateless worker
        }
    }
    live_delta(ctr, win, false);
}

static __global__ void __launch_bounds__(PL_NT) k_actv_resolve(const gd_key* __restrict__ ta, uint32_t n, uint32_t wide,
                                                        AdArgs t, const ActvWords* __restrict__ w,
                                                        const uint32_t* __restrict__ last,
                                                        const uint32_t* __restrict__ idx, uint8_t* __restrict__ kind,
                                                        uint32_t* __restrict__ ctx_out, uint8_t* __restrict__ st_out,
                                                        uint32_t* __restrict__ tile_new, uint32_t* __restrict__ tile_gone,
                                                        uint32_t tiles) {
    __shared__ uint32_t s_wn[PL_NW], s_wg[PL_NW];
    const uint32_t i0 = blockIdx.x * PL_TILE + threadIdx.x * PL_IT;
    const bool wb = wide & AV_WIDE_BYTES;
    uint32_t kw[4];
    pl_load16(kind, i0, n, wb, (uint32_t)ACTV_NONE, kw);
    const uint32_t pend = av_bits_mask(kw, AV_PENDING);
    const bool open = w->gate != 0;
    uint32_t cn = 0, cg = 0;
    for (uint32_t m = pend; m; m &= m - 1u) {
        const uint32_t r = (uint32_t)__ffs((int)m) - 1u, i = i0 + r, sh = 8 * (r & 3u);
        const uint32_t base = (kw[r >> 2] >> sh) & AV_KIND;
        uint32_t k = ACTV_HOST;                          // a refused batch: C# decides
        if (open) {
            k = base;
            const uint64_t* kp = reinterpret_cast<const uint64_t*>(ta + i);
            uint4 b;
            const uint32_t s = find_slot(t.slots, t.mask, t.ctr->max_probe, kp[0], kp[1], kp[2], b);
            if (s != NONE32) {                           // created by this batch: by the candidate its word names
                const uint32_t cw = last[s];
                const uint32_t creator = cw ? idx[~cw] : 0u;
                if (i >= creator) {
                    k = i == creator ? ACTV_CREATED : ACTV_FOUND;
                    ctx_out[i] = b.z;
                    st_out[i] = RECV_ACTIVATION;
                }
            }
        }
        kw[r >> 2] = (kw[r >> 2] & ~(0xFFu << sh)) | (k << sh);
        cn += k == ACTV_CREATED ? 1u : 0u;
        cg += k == ACTV_NONEXISTENT ? 1u : 0u;
    }
    if (pend) av_store16(kind, i0, n, wb, kw);
    av_tile_count(cn, s_wn, tile_new, tiles);
    av_tile_count(cg, s_wg, tile_gone, tiles);
}

// out_idx[0 .. n_out): the messages of kind v in arrival order (k_turn_starts' walk).  tile_off: the exclusive scan
// of k_actv_resolve's counts; cap: out_idx's entries.
static __global__ void __launch_bounds__(PL_NT) k_actv_list(const uint8_t* __restrict__ kind, uint32_t n, uint32_t wide,
                                                     const uint32_t* __restrict__ tile_off, uint32_t tiles, uint32_t v,
                                                     uint32_t* __restrict__ out_idx, uint32_t cap,
                                                     uint32_t* __restrict__ n_out) {
    __shared__ uint32_t s_wcnt[PL_NW];
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = tile_off[tiles];
    const uint32_t tile_base = tile_off[blockIdx.x];
    if (tile_off[blockIdx.x + 1] == tile_base) return;  // the whole workgroup
    const uint32_t i0 = blockIdx.x * PL_TILE + threadIdx.x * PL_IT;
    uint32_t kw[4];
    pl_load16(kind, i0, n, wide & AV_WIDE_BYTES, (uint32_t)ACTV_NONE, kw);
    uint32_t m = pl_eq_mask(kw, v);
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
        if (j < cap) out_idx[j] = i0 + ((uint32_t)__ffs((int)m) - 1u);   // always true when the scan is right
}

// The election words of the candidates' slots back to zero (they named the creators until now).
static __global__ void __launch_bounds__(BLOCK) k_actv_clear(const ActvWords* __restrict__ w,
                                                      const uint32_t* __restrict__ slot_of, uint32_t* __restrict__ last) {
    if (!w->gate) return;
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j < w->n_cand && slot_of[j] < SLOT_RETRY) last[slot_of[j]] = 0;
}

// Message.IsNewPlacement of the GD_RECV_NULL_CONTEXT frames (the decoder steps over the token): the header walk
// in the serializer's order (Message.cs:1247-1356) up to the bool tokens, through global memory (lim = 0: these
// frames are few).  True iff mask bit 18 is set and the token is SerializationTokenType.True.  A NULL_CONTEXT
// frame decoded completely, so its mask has neither CacheInvalidationHeader nor RequestContext -- or, with WALK
// (GD_OPT_WALK_INVALIDATION), a CacheInvalidationHeader the decoder stepped over, which this walk steps over too.
template <bool WALK = false>
static __global__ void __launch_bounds__(BLOCK) k_actv_newp(const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                     const uint64_t* __restrict__ frame_off,
                                                     const uint8_t* __restrict__ rs, uint32_t n,
                                                     uint8_t* __restrict__ newp) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t v = 0;
    if (rs[i] == RECV_NULL_CONTEXT) {
        const uint64_t start = frame_off[i];
        if (start <= buf_len && buf_len - start >= 12) {
            HeaderWalk hw;
            hw.c.row = nullptr;
            hw.c.g = buf + start;
            hw.c.sh = 0;
            hw.c.lim = 0;
            hw.bad = false;
            const int32_t hl = (int32_t)hw.c.u32(0), bl = (int32_t)hw.c.u32(4);
            const uint32_t m = hw.c.u32(8);
            const bool ok = !(hl < 4 || bl < 0 || (uint64_t)hl + (uint64_t)bl > buf_len - start - 8) &&
                            !(m & ((WALK ? 0u : H_CACHE_INVALIDATION) | H_REQUEST_CONTEXT));
            if (ok && (m & H_IS_NEW_PLACEMENT)) {
                hw.p = 12;
                hw.end = 8u + (uint32_t)hl;
                if (WALK && (m & H_CACHE_INVALIDATION)) hw.skip_invalidation();
                if (m & H_CATEGORY) hw.take(1);
                if (m & H_DEBUG_CONTEXT) hw.skip_string();
                if ((m & H_DIRECTION) && !hw.bad) hw.take(1);
                if ((m & H_TIME_TO_LIVE) && !hw.bad) hw.take(8);
                if ((m & H_FORWARD_COUNT) && !hw.bad) hw.take(4);
                if (m & H_GENERIC_GRAIN_TYPE) hw.skip_string();
                if ((m & H_CORRELATION_ID) && !hw.bad) hw.take(8);
                // bool tokens, serializer order: AlwaysInterleave, IsNewPlacement, ReadOnly, IsUnordered
                const uint32_t before = (m & H_ALWAYS_INTERLEAVE) ? 1u : 0u;
                if (!hw.bad && hw.take(before + 1u)) v = hw.c.u8(hw.p - 1) == TOKEN_TRUE ? 1u : 0u;
            }
        }
    }
    newp[i] = (uint8_t)v;
}

}  // namespace gd
