// gd_forward.h -- gfx950 device code for the forward writer: batched Dispatcher.TryForwardRequest
// (Dispatcher.cs:526-570) -> TryForwardMessage (:591-599) -> ResendMessageImpl (:601-623) -> AddressMessage ->
// Message.Serialize (Message.cs:481-516, HeadersContainer.Serializer :1126-1244) on the frames of a received batch
// that gd_turns* marked GD_TURN_FORWARD / GD_TURN_STUCK, or that stood on the waiting list of a deactivated
// activation.
//
// A forwarded header is the source header with a few fields written over: the CacheInvalidationHeader gains one
// entry (count + 1, the old entries as they stand, then silos[local_silo] + the frame's TargetGrain + the old
// ActivationId), ForwardCount becomes old + 1, TargetActivation / TargetSilo are replaced by the forwarding
// address, or removed and then set again from the route (Message.SetTargetPlacement, as gd_encode.h), and
// IsNewPlacement / NewGrainType follow.  Every other byte is copied in order (rule and statuses:
// include/graindispatch.h, tests/_forward_ref.py).  So an output frame is FWD_SEGS byte runs laid end to end, each
// a copy from one of five places: the source frame, the frame's plan record (the written constants), the
// ActivationId map, the silo table, the type-name table.
//
// The invalidation header is sized, not opaque: int32 count, then per entry SiloAddress (24 B), GrainId UniqueKey
// (24 B + KeyExt string), ActivationId UniqueKey (24 B + KeyExt string), no type token (Message.cs:1132-1140,
// BinaryTokenStreamWriter.cs:27-35): k_fwd_plan walks through it where the other walks stop.
//
//   k_fwd_kinds   GD_TURN_FORWARD / GD_TURN_STUCK -> GD_FWD_FORWARD, one lane a message
//   k_fwd_plan    one lane per frame: the decoder's staging and walk (gd_frames.h) through the invalidation entries
//                 to the copied runs; writes one 128-B FwdPlan a frame -- 8 (source position, length) runs in
//                 output order, the written constants, the table indexes -- its output length, its status and its
//                 TargetGrain.  Two or more old entries (>= 80 B each) push TargetGrain past the 192-B window:
//                 those reads take the cursor's byte-wise global path
//   k_fwd_merge, k_fwd_finish   the chain (gd_forward_send*): the route's results merged with the forwarding
//                 addresses, then the plans of the frames the route hit finished (fwd_place)
//   k_enc_lens, scan_device, k_enc_finish (gd_frameout.h): the offsets and the capacity check, as the encoder
//   k_fwd_write   the hot path: k_run_write<FwdArgs> (gd_frameout.h), the writer the response and the rejection
//                 stage use too.  FwdArgs::frame maps a plan record to the FWD_SEGS runs.  The TargetGrain run is
//                 read twice: into the appended entry and in its own place.
//
// Totals are 32-bit: the host refuses (GD_EINVAL) a call whose bound reaches 2^32, so gd_scan.h's scan serves.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_encode.h"
#include "gd_frameout.h"
#include "gd_frames.h"
#include "gd_hash.h"

namespace gd {

// GD_FWD_* / GD_FWDST_* (include/graindispatch.h)
enum : uint32_t { FWD_NONE = 0, FWD_FORWARD = 1 };
enum : uint32_t { FWDST_OK_ADDRESSED = 0, FWDST_OK_UNADDRESSED = 1, FWDST_SKIPPED = 2, FWDST_MALFORMED = 3,
                  FWDST_FALLBACK = 4, FWDST_REJECT = 5, FWDST_NO_SILO = 6, FWDST_NO_ID = 7 };
constexpr uint32_t FWD_TURN_STUCK = 4, FWD_TURN_FORWARD = 5;     // GD_TURN_*
constexpr uint32_t FWD_RUNS = 8;             // copied runs of the source frame
constexpr uint32_t FWD_SEGS = 19;            // runs of an output frame
constexpr uint32_t ROUTE_KEYEXT_ST = 4;      // GD_ROUTE_KEYEXT

// FwdPlan::flags
enum : uint32_t { FF_COUNT = 1u,        // the invalidation count is written (the output carries the header)
                  FF_APPEND = 2u,       // one entry is appended
                  FF_FC = 4u,           // ForwardCount is written (the new value is not 0)
                  FF_INP = 8u,          // an IsNewPlacement token is written (c[5]: the frame's own, or True)
                  FF_NGT = 16u,         // NewGrainType is written from the type table
                  FF_TA = 32u, FF_TS = 64u,   // TargetActivation / TargetSilo are written
                  FF_TG_EXT = 128u,     // TargetGrain carries a KeyExt string
                  FF_FWD_ADDR = 256u }; // the address is the caller's forwarding address

// One frame's plan, 128 B.  Runs in output order, positions in bytes from the frame start in the SOURCE:
//   0 the old invalidation entries   1 TargetGrain (the appended entry's copy)
//   2 Category .. TimeToLive         3 GenericGrainType .. AlwaysInterleave
//   4 ReadOnly, IsUnordered (+ the frame's NewGrainType when it stays)
//   5 RejectionInfo .. SendingSilo   6 TargetGrain, TargetObserver   7 TransactionInfo / trailing bytes + body
// c: the written dwords -- 0 headerLength, 1 bodyLength, 2 mask, 3 the invalidation count, 4 ForwardCount,
// 5 the IsNewPlacement token (low byte), 6 NewGrainType's length, 7 0xFFFFFFFF (a null KeyExt).
// Only the two OK statuses have a plan that is read.
struct FwdPlan {
    uint32_t pos[FWD_RUNS];
    uint32_t len[FWD_RUNS];
    uint32_t c[8];
    uint32_t ent_act;        // the appended entry's activation index
    uint32_t ta_act;         // TargetActivation's activation index
    uint32_t ts_silo;        // TargetSilo's silo index
    uint32_t type_pos;       // NewGrainType's first byte in the type table
    uint32_t type_len;
    uint32_t flags;
    uint32_t r_ngt;          // bytes of the frame's own NewGrainType (inside run 4 until it is replaced)
    uint32_t pad;
};
static_assert(sizeof(FwdPlan) == 128, "plan record is 128 B");

__device__ __forceinline__ void fwd_plan_store(FwdPlan* dst, const FwdPlan& p) {
    uint4* pp = reinterpret_cast<uint4*>(dst);
    pp[0] = make_uint4(p.pos[0], p.pos[1], p.pos[2], p.pos[3]);
    pp[1] = make_uint4(p.pos[4], p.pos[5], p.pos[6], p.pos[7]);
    pp[2] = make_uint4(p.len[0], p.len[1], p.len[2], p.len[3]);
    pp[3] = make_uint4(p.len[4], p.len[5], p.len[6], p.len[7]);
    pp[4] = make_uint4(p.c[0], p.c[1], p.c[2], p.c[3]);
    pp[5] = make_uint4(p.c[4], p.c[5], p.c[6], p.c[7]);
    pp[6] = make_uint4(p.ent_act, p.ta_act, p.ts_silo, p.type_pos);
    pp[7] = make_uint4(p.type_len, p.flags, p.r_ngt, 0u);
}

// Message.SetTargetPlacement (Message.cs:629-639) on the plan of a frame that left k_fwd_plan unaddressed: exactly
// gd_encode_frames' rule.  Returns the frame's status; the plan changes only with FWDST_OK_ADDRESSED.
__device__ __forceinline__ uint32_t fwd_place(FwdPlan& p, uint32_t silo, uint32_t act, uint32_t placed, uint32_t ty,
                                              const EncTab& t) {
    if (silo >= t.n_silos) return FWDST_NO_SILO;
    if (!enc_has_id(t, act)) return FWDST_NO_ID;
    uint32_t grow = ENC_TA_LEN + ENC_TS_LEN;
    p.flags |= FF_TA | FF_TS;
    p.ta_act = act;
    p.ts_silo = silo;
    p.c[2] |= H_TARGET_ACTIVATION | H_TARGET_SILO;
    if (placed == ENC_PLACED_NEW) {
        if (!(p.flags & FF_INP)) grow += 1;
        p.flags |= FF_INP;
        p.c[5] = TOKEN_TRUE;
        p.c[2] |= H_IS_NEW_PLACEMENT;
    }
    if (ty < t.n_types) {
        const uint32_t o = t.type_off[ty], ln = t.type_off[ty + 1] - o;
        if (ln) {                                            // String.IsNullOrEmpty: unchanged
            p.flags |= FF_NGT;
            p.type_pos = o;
            p.type_len = ln;
            p.c[6] = ln;
            p.len[4] -= p.r_ngt;
            grow += 4 + ln - p.r_ngt;                        // mod 2^32: r_ngt may exceed 4 + ln
            p.c[2] |= H_NEW_GRAIN_TYPE;
        }
    }
    p.c[0] += grow;
    return FWDST_OK_ADDRESSED;
}

// ------------------------------------------------------------------ k_fwd_kinds
static __global__ __launch_bounds__(BLOCK) void k_fwd_kinds(const uint8_t* __restrict__ turn, uint32_t n,
                                                     uint8_t* __restrict__ kind) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = turn[i];
    kind[i] = (uint8_t)((t == FWD_TURN_FORWARD || t == FWD_TURN_STUCK) ? FWD_FORWARD : FWD_NONE);
}

// ------------------------------------------------------------------ k_fwd_plan
struct FwdIn {
    const uint8_t* kind;
    const uint32_t* old_act;         // may be null: no oldAddress
    const uint32_t* fwd_silo;        // with fwd_act, may be null: no forwarding address
    const uint32_t* fwd_act;
    const uint32_t* silo;            // the route's results; null in the chain's first pass
    const uint32_t* act;
    const uint8_t* status;
    const uint8_t* placed;           // may be null
    const uint32_t* new_type;        // may be null
    int32_t max_forward;
    uint32_t local_silo;
    long long* ttl;                  // the chain's send stage: TimeToLive and Category of every frame; may be null
    uint8_t* category;
};

static __global__ __launch_bounds__(BLOCK) void k_fwd_plan(const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                    const uint64_t* __restrict__ frame_off, uint32_t n, FwdIn in,
                                                    EncTab t, FwdPlan* __restrict__ plan,
                                                    uint32_t* __restrict__ out_len, uint8_t* __restrict__ fwd_status,
                                                    uint64_t* __restrict__ target) {
    __shared__ uint32_t s_win[BLOCK / WAVE][WAVE][FRAME_ROW];
    __shared__ unsigned long long s_start[BLOCK / WAVE][WAVE];
    const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const uint32_t i = blockIdx.x * BLOCK + w * WAVE + lane;
    const bool valid = i < n;
    const uint64_t start = frame_off[valid ? i : (n - 1)];

    // ---- stage: as k_decode_frames (gd_frames.h): every lane 12 x 16-B loads over the wave's 64 windows,
    // clamped into [0, dw_end)
    const uint64_t dw_end = buf_len & ~3ull;
    constexpr int CHUNKS = FRAME_WIN / 16;
    s_start[w][lane] = start;
    __syncthreads();
    if (dw_end >= 16) {
        uint4 v[CHUNKS];
#pragma unroll
        for (int it = 0; it < CHUNKS; ++it) {
            const uint32_t q = it * WAVE + lane, f = q / CHUNKS, c = q % CHUNKS;
            const uint64_t a = (s_start[w][f] & ~3ull) + 16ull * c;
            v[it] = *(const uint4*)(buf + (a <= dw_end - 16 ? a : ((dw_end - 16) & ~3ull)));
        }
#pragma unroll
        for (int it = 0; it < CHUNKS; ++it) {
            const uint32_t q = it * WAVE + lane, f = q / CHUNKS, c = q % CHUNKS;
            uint32_t* r = &s_win[w][f][4 * c];
            r[0] = v[it].x;
            r[1] = v[it].y;
            r[2] = v[it].z;
            r[3] = v[it].w;
        }
    }
    __syncthreads();
    if (!valid) return;

    FwdPlan p;
#pragma unroll
    for (uint32_t k = 0; k < FWD_RUNS; ++k) p.pos[k] = p.len[k] = p.c[k] = 0;
    p.ent_act = p.ta_act = p.ts_silo = p.type_pos = p.type_len = p.flags = p.r_ngt = p.pad = 0;
    uint32_t st = FWDST_SKIPPED, cat = 0;
    int64_t ttl = GD_TTL_NONE;
    Key3 tg{0, 0, 0};
    if (in.kind[i] == FWD_FORWARD) {
        const uint64_t a0 = start & ~3ull;
        uint64_t win_end = a0;
        if (dw_end >= 16 && dw_end > a0) {
            const uint64_t full = (dw_end - a0) / 16;
            win_end = a0 + 16 * (full < (uint64_t)CHUNKS ? full : (uint64_t)CHUNKS);
        }
        HeaderWalk hw;
        hw.c.row = s_win[w][lane];
        hw.c.g = buf + start;
        hw.c.sh = (uint32_t)(start & 3);
        hw.c.lim = (start < win_end) ? (uint32_t)(win_end - start) : 0u;
        hw.bad = false;

        bool malformed = start > buf_len || buf_len - start < 8;
        int32_t hl = 0, bl = 0;
        if (!malformed) {
            hl = (int32_t)hw.c.u32(0);
            bl = (int32_t)hw.c.u32(4);
            malformed = hl < 4 || bl < 0 || (uint64_t)hl + (uint64_t)bl > buf_len - start - 8;
        }
        if (malformed) {
            st = FWDST_MALFORMED;
        } else {
            hw.p = 12;
            hw.end = 8u + (uint32_t)hl;
            const uint32_t m = hw.c.u32(8);
            // ---- the invalidation header: int32 count, then count x (SiloAddress, GrainId, ActivationId)
            uint32_t cnt = 0;
            if ((m & H_CACHE_INVALIDATION) && hw.take(4)) {
                const int32_t c = (int32_t)hw.c.u32(12);
                if (c < 0) hw.bad = true;
                cnt = (uint32_t)c;
                for (uint32_t k = 0; k < cnt && !hw.bad; ++k) {      // an entry holds >= 80 B: the header bounds it
                    if (!hw.take(24)) break;
                    hw.key(nullptr);
                    hw.key(nullptr);
                }
            }
            const uint32_t e_cih = hw.p;
            // ---- HeadersContainer.Serializer order (Message.cs:1142-1243)
            if ((m & H_CATEGORY) && !hw.bad && hw.take(1)) cat = hw.c.u8(hw.p - 1);
            if (m & H_DEBUG_CONTEXT) hw.skip_string();
            if ((m & H_DIRECTION) && !hw.bad) hw.take(1);
            if ((m & H_TIME_TO_LIVE) && !hw.bad && hw.take(8)) ttl = (int64_t)hw.c.u64(hw.p - 8);
            const uint32_t p_fc = hw.p;
            int32_t fc = 0;
            uint32_t r_fc = 0;
            if ((m & H_FORWARD_COUNT) && !hw.bad && hw.take(4)) {
                fc = (int32_t)hw.c.u32(hw.p - 4);
                r_fc = 4;
            }
            if (m & H_GENERIC_GRAIN_TYPE) hw.skip_string();
            if ((m & H_CORRELATION_ID) && !hw.bad) hw.take(8);
            if ((m & H_ALWAYS_INTERLEAVE) && !hw.bad) hw.take(1);
            const uint32_t p_inp = hw.p;
            uint32_t r_inp = 0, tok = 0;
            if ((m & H_IS_NEW_PLACEMENT) && !hw.bad && hw.take(1)) {
                tok = hw.c.u8(hw.p - 1);
                r_inp = 1;
            }
            const uint32_t nb = __popc(m & (H_READ_ONLY | H_IS_UNORDERED));
            if (nb && !hw.bad) hw.take(nb);
            const uint32_t p_ngt = hw.p;
            if (m & H_NEW_GRAIN_TYPE) hw.skip_string();
            const uint32_t r_ngt = hw.p - p_ngt;
            if (m & H_REJECTION_INFO) hw.skip_string();
            if ((m & H_REJECTION_TYPE) && !hw.bad) hw.take(1);
            // RequestContext is object-serialized: the walk ends in front of it.  So it does behind TargetGrain
            // when TargetObserver and TransactionInfo both follow (TargetSilo cannot be found between them).
            const bool opaque_tail = (m & H_TARGET_OBSERVER) && (m & H_TRANSACTION_INFO);
            uint32_t p_ta = 0, r_ta = 0, p_tg = 0, e_tg = 0, p_ts = 0, r_ts = 0;
            int32_t ext = -1;
            if (!(m & H_REQUEST_CONTEXT)) {
                if ((m & H_RESEND_COUNT) && !hw.bad) hw.take(4);
                if ((m & H_RESULT) && !hw.bad) hw.take(1);
                if (m & H_SENDING_ACTIVATION) hw.key(nullptr);
                if (m & H_SENDING_GRAIN) hw.key(nullptr);
                if ((m & H_SENDING_SILO) && !hw.bad) hw.take(24);
                p_ta = hw.p;
                if (m & H_TARGET_ACTIVATION) hw.key(nullptr);
                r_ta = hw.p - p_ta;
                p_tg = hw.p;
                if (m & H_TARGET_GRAIN) tg = hw.key(&ext);
                e_tg = hw.p;
                if (!opaque_tail) {
                    r_ts = (m & H_TARGET_SILO) ? ENC_TS_LEN : 0u;
                    p_ts = hw.p;
                    if (m & H_TARGET_OBSERVER) {
                        // object-serialized, no TransactionInfo behind it: TargetSilo is the header's last field
                        if (!hw.bad && hw.end - hw.p < r_ts) hw.bad = true;
                        p_ts = hw.end - r_ts;
                    } else if (r_ts && !hw.bad) {
                        hw.take(ENC_TS_LEN);
                    }
                }
            }
            const uint32_t oa = in.old_act ? in.old_act[i] : NONE32;
            const bool append = oa != NONE32;
            const uint32_t fs = (in.fwd_silo && in.fwd_act) ? in.fwd_silo[i] : NONE32;
            const bool has_fwd = fs != NONE32;
            const uint32_t fa = has_fwd ? in.fwd_act[i] : NONE32;
            if (hw.bad) {
                st = FWDST_MALFORMED;
            } else if ((m & H_REQUEST_CONTEXT) || opaque_tail || !(m & H_TARGET_GRAIN) ||
                       (uint32_t)(tg.tcd >> 56) == CAT_SYSTEM_TARGET) {
                st = FWDST_FALLBACK;                         // SendSystemTargetMessage (Dispatcher.cs:606-609)
            } else if (fc >= in.max_forward) {
                st = FWDST_REJECT;                           // MayForward (:627-630)
            } else if (append && in.local_silo >= t.n_silos) {
                st = FWDST_NO_SILO;
            } else if (append && !enc_has_id(t, oa)) {
                st = FWDST_NO_ID;
            } else if (has_fwd && fs >= t.n_silos) {
                st = FWDST_NO_SILO;
            } else if (has_fwd && !enc_has_id(t, fa)) {
                st = FWDST_NO_ID;
            } else {
                const uint32_t src_len = 8u + (uint32_t)hl + (uint32_t)bl;
                const uint32_t fc_new = (uint32_t)fc + 1u;
                uint32_t fl = (ext >= 0 ? FF_TG_EXT : 0u) | (fc_new ? FF_FC : 0u);
                uint32_t om = m & ~(H_TARGET_ACTIVATION | H_TARGET_SILO | H_FORWARD_COUNT);
                if (fc_new) om |= H_FORWARD_COUNT;
                if ((m & H_CACHE_INVALIDATION) || append) fl |= FF_COUNT;
                if (append) {
                    fl |= FF_APPEND;
                    om |= H_CACHE_INVALIDATION;
                    p.ent_act = oa;
                    p.pos[1] = p_tg;
                    p.len[1] = e_tg - p_tg;
                }
                if (m & H_CACHE_INVALIDATION) {
                    p.pos[0] = 16;
                    p.len[0] = e_cih - 16;
                }
                p.pos[2] = e_cih;
                p.len[2] = p_fc - e_cih;
                p.pos[3] = p_fc + r_fc;
                p.len[3] = p_inp - p.pos[3];
                p.pos[4] = p_inp + r_inp;
                p.len[4] = p_ngt + r_ngt - p.pos[4];
                p.pos[5] = p_ngt + r_ngt;
                p.len[5] = p_ta - p.pos[5];
                p.pos[6] = p_ta + r_ta;
                p.len[6] = p_ts - p.pos[6];
                p.pos[7] = p_ts + r_ts;
                p.len[7] = src_len - p.pos[7];
                p.r_ngt = r_ngt;
                if (has_fwd) {                               // TargetAddress = forwardingAddress, IsNewPlacement = false
                    fl |= FF_TA | FF_TS | FF_FWD_ADDR;
                    om = (om | H_TARGET_ACTIVATION | H_TARGET_SILO) & ~H_IS_NEW_PLACEMENT;
                    p.ta_act = fa;
                    p.ts_silo = fs;
                } else if (r_inp) {
                    fl |= FF_INP;                            // the frame's own token stays
                }
                p.flags = fl;
                uint32_t hb = 4;
#pragma unroll
                for (uint32_t k = 0; k < FWD_RUNS; ++k) hb += p.len[k];
                hb -= (uint32_t)bl;
                hb += ((fl & FF_COUNT) ? 4u : 0u) + (append ? 24u + 28u : 0u) + (fc_new ? 4u : 0u) +
                      ((fl & FF_INP) ? 1u : 0u) + (has_fwd ? ENC_TA_LEN + ENC_TS_LEN : 0u);
                p.c[0] = hb;
                p.c[1] = (uint32_t)bl;
                p.c[2] = om;
                p.c[3] = cnt + (append ? 1u : 0u);
                p.c[4] = fc_new;
                p.c[5] = tok;
                p.c[7] = 0xFFFFFFFFu;
                st = has_fwd ? FWDST_OK_ADDRESSED : FWDST_OK_UNADDRESSED;
                if (!has_fwd && in.status && in.status[i] == 0 /* GD_ROUTE_OK */)
                    st = fwd_place(p, in.silo[i], in.act[i], in.placed ? in.placed[i] : 0u,
                                   in.new_type ? in.new_type[i] : NONE32, t);
            }
        }
    }
    uint32_t olen = 0;
    if (st <= FWDST_OK_UNADDRESSED) {
        fwd_plan_store(plan + i, p);
        olen = 8u + p.c[0] + p.c[1];
    } else {
        plan[i].flags = 0;                                   // k_fwd_merge reads the flags of every frame
    }
    out_len[i] = olen;
    fwd_status[i] = (uint8_t)st;
    if (target) {
        const bool keyed = st != FWDST_SKIPPED && st != FWDST_MALFORMED && st != FWDST_FALLBACK;
        store_key(target, i, keyed ? tg : Key3{0, 0, 0});
    }
    if (in.ttl) in.ttl[i] = ttl;
    if (in.category) in.category[i] = (uint8_t)cat;
}

// ------------------------------------------------------------------ the chain: k_fwd_merge, k_fwd_finish
// The route ran on every frame's `target`.  Per message: a frame that does not leave has no address
// (GD_ROUTE_UNDECODED: the send stage holds it); a forwarding address wins over the route; a TargetGrain with a
// KeyExt string was routed without it and stays unaddressed (GD_ROUTE_KEYEXT); else the route's result stands.
static __global__ __launch_bounds__(BLOCK) void k_fwd_merge(const uint8_t* __restrict__ fwd_status,
                                                     const FwdPlan* __restrict__ plan, uint32_t n,
                                                     uint32_t* __restrict__ silo, uint32_t* __restrict__ act,
                                                     uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t st = fwd_status[i];
    if (st == FWDST_OK_ADDRESSED) {
        silo[i] = plan[i].ts_silo;
        act[i] = plan[i].ta_act;
        status[i] = 0;                                       // GD_ROUTE_OK
    } else if (st != FWDST_OK_UNADDRESSED) {
        silo[i] = NONE32;
        act[i] = NONE32;
        status[i] = ROUTE_UNDECODED;
    } else if (plan[i].flags & FF_TG_EXT) {
        silo[i] = NONE32;
        act[i] = NONE32;
        status[i] = (uint8_t)ROUTE_KEYEXT_ST;
    }
}

// The lengths that depend on the route: the frames the route hit get their address (fwd_place).
static __global__ __launch_bounds__(BLOCK) void k_fwd_finish(const uint32_t* __restrict__ silo,
                                                      const uint32_t* __restrict__ act,
                                                      const uint8_t* __restrict__ status, uint32_t n, EncTab t,
                                                      FwdPlan* __restrict__ plan, uint32_t* __restrict__ out_len,
                                                      uint8_t* __restrict__ fwd_status) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (fwd_status[i] != FWDST_OK_UNADDRESSED || status[i] != 0) return;
    FwdPlan p = plan[i];
    const uint32_t st = fwd_place(p, silo[i], act[i], 0u, NONE32, t);
    if (st == FWDST_OK_ADDRESSED) {
        fwd_plan_store(plan + i, p);
        out_len[i] = 8u + p.c[0] + p.c[1];
    } else {
        out_len[i] = 0;
    }
    fwd_status[i] = (uint8_t)st;
}

// ------------------------------------------------------------------ k_fwd_write: k_run_write<FwdArgs>
struct FwdArgs {
    static constexpr uint32_t SEGS = FWD_SEGS;
    const uint8_t* buf;
    const uint64_t* frame_off;
    const uint32_t* order;
    const FwdPlan* plan;
    const uint32_t* offs;        // n + 1 scanned offsets in output order
    const uint8_t* act_ids;      // 24 B an activation index
    const uint8_t* silo_wire;    // 24 B a silo index
    const uint8_t* type_utf8;
    uint32_t local_silo;
    uint32_t n;
    uint64_t out_cap;

    // Output frame j, whose first output position is fo.
    __device__ __forceinline__ void frame(uint32_t j, uint32_t fo, RunFrame<SEGS>& f) const {
        const uint32_t i = order ? min(order[j], n - 1) : j;
        const uint4* pp = reinterpret_cast<const uint4*>(plan + i);
        const uint4 q0 = pp[0], q1 = pp[1], q2 = pp[2], q3 = pp[3], q6 = pp[6], q7 = pp[7];
        const uint64_t src = reinterpret_cast<uint64_t>(buf + frame_off[i]);
        const uint64_t cb = reinterpret_cast<uint64_t>(plan + i) + 2 * FWD_RUNS * 4;      // FwdPlan::c
        const uint64_t ids = reinterpret_cast<uint64_t>(act_ids), silos = reinterpret_cast<uint64_t>(silo_wire);
        const uint32_t fl = q7.y;
        const uint32_t ap = (fl & FF_APPEND) ? 1u : 0u, ta = (fl & FF_TA) ? 1u : 0u, ts = (fl & FF_TS) ? 1u : 0u;
        uint32_t cur = fo;
        uint64_t prev = 0;
        RUN_SEG(f, cur, prev, 0, cb, 12u + ((fl & FF_COUNT) ? 4u : 0u));
        RUN_SEG(f, cur, prev, 1, src + q0.x, q2.x);
        RUN_SEG(f, cur, prev, 2, silos + 24ull * local_silo, 24u * ap);
        RUN_SEG(f, cur, prev, 3, src + q0.y, q2.y);
        RUN_SEG(f, cur, prev, 4, ids + 24ull * q6.x, 24u * ap);
        RUN_SEG(f, cur, prev, 5, cb + 28, 4u * ap);
        RUN_SEG(f, cur, prev, 6, src + q0.z, q2.z);
        RUN_SEG(f, cur, prev, 7, cb + 16, (fl & FF_FC) ? 4u : 0u);
        RUN_SEG(f, cur, prev, 8, src + q0.w, q2.w);
        RUN_SEG(f, cur, prev, 9, cb + 20, (fl & FF_INP) ? 1u : 0u);
        RUN_SEG(f, cur, prev, 10, src + q1.x, q3.x);
        RUN_SEG(f, cur, prev, 11, cb + 24, (fl & FF_NGT) ? 4u : 0u);
        RUN_SEG(f, cur, prev, 12, reinterpret_cast<uint64_t>(type_utf8) + q6.w, (fl & FF_NGT) ? q7.x : 0u);
        RUN_SEG(f, cur, prev, 13, src + q1.y, q3.y);
        RUN_SEG(f, cur, prev, 14, ids + 24ull * q6.y, 24u * ta);
        RUN_SEG(f, cur, prev, 15, cb + 28, 4u * ta);
        RUN_SEG(f, cur, prev, 16, src + q1.z, q3.z);
        RUN_SEG(f, cur, prev, 17, silos + 24ull * q6.z, 24u * ts);
        RUN_SEG(f, cur, prev, 18, src + q1.w, q3.w);
    }
};

}  // namespace gd

