// gd_reject.h -- gfx950 device code for the forward rejections: the failure arm of
// Dispatcher.TryForwardRequest (Dispatcher.cs:526-570: AddToCacheInvalidationHeader, then TryForwardMessage's
// MayForward test, :591-599, :627-630) -> RejectMessage (:203-222) -> MessageFactory.CreateRejectionResponse
// (MessageFactory.cs:49-111) -> Message.Serialize, on the frames of a received batch that gd_forward_frames*
// marks GD_FWDST_REJECT.
//
// The answer is the response writer's Transient rejection (gd_respond.h) of the request with one entry appended to
// its CacheInvalidationHeader (gd_forward.h): CreateResponseMessage copies the header the forward arm has just
// extended.  Rule and statuses: include/graindispatch.h, tests/_reject_ref.py.
//
// The cut is the one DESIGN 5.24 proposed for the forward writer: whatever the planner knows is written into the
// plan record as bytes, in output order, so a run of the output is either a copy from the request frame or a copy
// from the record.  An output frame is REJ_SEGS = 14 runs (the response writer has 18, the forward writer 19):
//    0 record A  headerLength, bodyLength, mask, [count]
//    1 request   the old entries
//    2 record B  the appended entry's SiloAddress, TargetGrain's three words and its KeyExt length
//    3 request   TargetGrain's KeyExt bytes (the appended entry's copy)
//    4 record C  the ActivationId of old_act, its null KeyExt, [Category]
//    5 request   DebugContext
//    6 record D  Direction, [TimeToLive], [CorrelationId], [AlwaysInterleave], [ReadOnly], [RejectionInfo length]
//    7 table     the RejectionInfo string
//    8 record E  Result
//    9 request   TargetActivation + TargetGrain  (-> SendingActivation, SendingGrain: adjacent in both)
//   10 request   TargetSilo                      (-> SendingSilo; the header's last field behind a TargetObserver)
//   11 request   SendingActivation .. SendingSilo (-> TargetActivation .. TargetSilo: adjacent in both)
//   12 request   TransactionInfo
//   13 caller    the body
// The entries and DebugContext are runs of their own, so the response writer's one remaining FALLBACK frame (entries,
// a default-valued Category byte, a DebugContext) is written here.  TargetGrain's words are not read twice: the
// planner has them in registers.
//
//   k_rej_plan    one lane a frame: reads the kind byte, and only the frames that are GD_FWD_FORWARD are staged
//                 (gd_frames.h's windows, the loads predicated by the wave's ballot) and walked -- through the
//                 entries as k_fwd_plan, on as k_rsp_plan.  Writes the 192-B record of an OK frame, the output
//                 length and the status
//   k_enc_lens, scan_device, k_enc_finish (gd_frameout.h): the offsets and the capacity check, as the encoder
//   k_rej_write   k_run_write<RejArgs> (gd_frameout.h), the writer the response and the forward stage use too.
//                 RejArgs::frame maps a plan record to the REJ_SEGS runs
//
// Totals are 32-bit: the host refuses (GD_EINVAL) a call whose bound reaches 2^32, so gd_scan.h's scan serves.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_forward.h"
#include "gd_respond.h"

namespace gd {

// GD_FWDREJ_* (include/graindispatch.h)
enum : uint32_t { FWDREJ_OK = 0, FWDREJ_SKIPPED = 1, FWDREJ_MALFORMED = 2, FWDREJ_FALLBACK = 3,
                  FWDREJ_MAY_FORWARD = 4, FWDREJ_DISCARDED = 5, FWDREJ_NO_SILO = 6, FWDREJ_NO_ID = 7 };
constexpr uint32_t REJ_SEGS = 14;            // runs of an output frame
constexpr uint32_t REJ_PLAN_DW = 48;         // one frame's plan record: 192 B
// The record, in dwords.  [0, 32) are the written bytes, each run packed from its first byte on:
//   A [0, 4)  B [4, 17)  C [17, 25)  D [25, 31)  E [31]
// [32] the lengths of A, B, C, D, a byte each; [33, 39) the positions of runs 3, 5, 9, 10, 11, 12 in bytes from
// the frame start in the request (run 1 starts at byte 16); [39, 46) the lengths of runs 1, 3, 5, 9, 10, 11, 12;
// [46] the info string's first byte in the table, [47] its length.  Only OK frames have a record that is read.
constexpr uint32_t REJ_A = 0, REJ_B = 16, REJ_C = 68, REJ_D = 100, REJ_E = 124;     // byte offsets

// Up to 24 bytes packed end to end in three registers pairs (no indexed array: nothing leaves the registers).
struct RejPack {
    uint64_t w0, w1, w2;
    uint32_t n;
    // v holds k <= 8 bytes, the rest of it zero
    __device__ __forceinline__ void put(uint64_t v, uint32_t k) {
        const uint32_t b = (n & 7u) * 8u, wi = n >> 3;
        const uint64_t lo = v << b, hi = b ? v >> (64u - b) : 0ull;
        w0 |= wi == 0 ? lo : 0ull;
        w1 |= wi == 0 ? hi : wi == 1 ? lo : 0ull;
        w2 |= wi == 1 ? hi : wi == 2 ? lo : 0ull;
        n += k;
    }
};

// ------------------------------------------------------------------ k_rej_plan
struct RejIn {
    const uint8_t* kind;
    const uint32_t* old_act;         // may be null: no oldAddress
    const uint32_t* info;            // may be null: no info
    const uint64_t* body_off;        // may be null: empty bodies
    const uint32_t* info_off;        // n_info + 1
    uint32_t n_info;
    int32_t max_forward;
    uint32_t local_silo;
};

static __global__ __launch_bounds__(BLOCK) void k_rej_plan(const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                    const uint64_t* __restrict__ frame_off, uint32_t n, RejIn in,
                                                    EncTab t, uint32_t* __restrict__ plan,
                                                    uint32_t* __restrict__ out_len, uint8_t* __restrict__ rej_status) {
    __shared__ uint32_t s_win[BLOCK / WAVE][WAVE][FRAME_ROW];
    __shared__ unsigned long long s_start[BLOCK / WAVE][WAVE];
    const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const uint32_t i = blockIdx.x * BLOCK + w * WAVE + lane;
    const bool valid = i < n;
    // most batches are sparse in rejections: a frame that is not FORWARD costs its kind byte, nothing of buf
    const bool fwd = valid && in.kind[i] == FWD_FORWARD;
    const uint64_t start = fwd ? frame_off[i] : 0ull;
    const unsigned long long live = __ballot(fwd);

    // ---- stage: as k_decode_frames (gd_frames.h): 12 x 16-B loads a lane over the wave's 64 windows, clamped
    // into [0, dw_end); the windows of frames that are not FORWARD are not loaded
    const uint64_t dw_end = buf_len & ~3ull;
    constexpr int CHUNKS = FRAME_WIN / 16;
    s_start[w][lane] = start;
    __syncthreads();
    if (dw_end >= 16 && live) {
        uint4 v[CHUNKS];
#pragma unroll
        for (int it = 0; it < CHUNKS; ++it) {
            const uint32_t q = it * WAVE + lane, f = q / CHUNKS, c = q % CHUNKS;
            v[it] = make_uint4(0, 0, 0, 0);
            if ((live >> f) & 1ull) {
                const uint64_t a = (s_start[w][f] & ~3ull) + 16ull * c;
                v[it] = *(const uint4*)(buf + (a <= dw_end - 16 ? a : ((dw_end - 16) & ~3ull)));
            }
        }
#pragma unroll
        for (int it = 0; it < CHUNKS; ++it) {
            const uint32_t q = it * WAVE + lane, f = q / CHUNKS, c = q % CHUNKS;
            if ((live >> f) & 1ull) {
                uint32_t* r = &s_win[w][f][4 * c];
                r[0] = v[it].x;
                r[1] = v[it].y;
                r[2] = v[it].z;
                r[3] = v[it].w;
            }
        }
    }
    __syncthreads();
    if (!valid) return;
    if (!fwd) {
        out_len[i] = 0;
        rej_status[i] = (uint8_t)FWDREJ_SKIPPED;
        return;
    }

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
    uint32_t st = FWDREJ_MALFORMED, olen = 0;
    if (!malformed) {
        hw.p = 12;
        hw.end = 8u + (uint32_t)hl;
        const uint32_t m = hw.c.u32(8);
        // ---- the walk of k_fwd_plan (gd_forward.h), field for field: the two stages must agree on MALFORMED
        uint32_t cnt = 0;
        if ((m & H_CACHE_INVALIDATION) && hw.take(4)) {
            const int32_t c = (int32_t)hw.c.u32(12);
            if (c < 0) hw.bad = true;
            cnt = (uint32_t)c;
            for (uint32_t k = 0; k < cnt && !hw.bad; ++k) {          // an entry holds >= 80 B: the header bounds it
                if (!hw.take(24)) break;
                hw.key(nullptr);
                hw.key(nullptr);
            }
        }
        const uint32_t e_cih = hw.p;
        uint32_t cat = 0;
        if ((m & H_CATEGORY) && !hw.bad && hw.take(1)) cat = hw.c.u8(hw.p - 1);
        const uint32_t p_dbg = hw.p;
        int32_t dbg = -1;
        if (m & H_DEBUG_CONTEXT) dbg = hw.skip_string();
        const uint32_t e_dbg = hw.p;
        uint32_t dir = 0;
        if ((m & H_DIRECTION) && !hw.bad && hw.take(1)) dir = hw.c.u8(hw.p - 1);
        uint64_t ttl = 0, corr = 0;
        bool has_ttl = false, has_corr = false;
        if ((m & H_TIME_TO_LIVE) && !hw.bad && hw.take(8)) {
            ttl = hw.c.u64(hw.p - 8);
            has_ttl = true;
        }
        int32_t fc = 0;
        if ((m & H_FORWARD_COUNT) && !hw.bad && hw.take(4)) fc = (int32_t)hw.c.u32(hw.p - 4);
        if (m & H_GENERIC_GRAIN_TYPE) hw.skip_string();
        if ((m & H_CORRELATION_ID) && !hw.bad && hw.take(8)) {
            corr = hw.c.u64(hw.p - 8);
            has_corr = true;
        }
        bool ai = false, ro = false;
        if ((m & H_ALWAYS_INTERLEAVE) && !hw.bad && hw.take(1)) ai = hw.c.u8(hw.p - 1) == TOKEN_TRUE;
        if ((m & H_IS_NEW_PLACEMENT) && !hw.bad) hw.take(1);
        if ((m & H_READ_ONLY) && !hw.bad && hw.take(1)) ro = hw.c.u8(hw.p - 1) == TOKEN_TRUE;
        if ((m & H_IS_UNORDERED) && !hw.bad) hw.take(1);
        if (m & H_NEW_GRAIN_TYPE) hw.skip_string();
        if (m & H_REJECTION_INFO) hw.skip_string();
        if ((m & H_REJECTION_TYPE) && !hw.bad) hw.take(1);
        const bool opaque_tail = (m & H_TARGET_OBSERVER) && (m & H_TRANSACTION_INFO_RSP);
        uint32_t p_sa = 0, p_sg = 0, p_ta = 0, p_tg = 0, e_tg = 0, p_ts = 0, r_ts = 0, p_ti = 0;
        int32_t ext = -1;
        Key3 tg{0, 0, 0};
        if (!(m & H_REQUEST_CONTEXT)) {
            if ((m & H_RESEND_COUNT) && !hw.bad) hw.take(4);
            if ((m & H_RESULT) && !hw.bad) hw.take(1);
            p_sa = hw.p;
            if (m & H_SENDING_ACTIVATION) hw.key(nullptr);
            p_sg = hw.p;
            if (m & H_SENDING_GRAIN) hw.key(nullptr);
            if ((m & H_SENDING_SILO) && !hw.bad) hw.take(24);
            p_ta = hw.p;
            if (m & H_TARGET_ACTIVATION) hw.key(nullptr);
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
                    p_ti = hw.end;
                } else {
                    if (r_ts && !hw.bad) hw.take(ENC_TS_LEN);
                    p_ti = hw.p;
                }
            }
        }
        const uint32_t oa = in.old_act ? in.old_act[i] : NONE32;
        const bool append = oa != NONE32;
        if (hw.bad) {
            st = FWDREJ_MALFORMED;
        } else if ((m & H_REQUEST_CONTEXT) || opaque_tail || !(m & H_TARGET_GRAIN) ||
                   (uint32_t)(tg.tcd >> 56) == CAT_SYSTEM_TARGET) {
            st = FWDREJ_FALLBACK;
        } else if (fc < in.max_forward) {
            st = FWDREJ_MAY_FORWARD;                             // MayForward (:627-630): the forward writer's frame
        } else if (dir != 0) {
            st = FWDREJ_DISCARDED;                               // RejectMessage :209-221: only a Request is answered
        } else if (append && in.local_silo >= t.n_silos) {
            st = FWDREJ_NO_SILO;
        } else if (append && !enc_has_id(t, oa)) {
            st = FWDREJ_NO_ID;
        } else {
            st = FWDREJ_OK;
            const uint32_t ap = append ? 1u : 0u;
            const uint32_t cnt_out = cnt + ap;
            const uint32_t len_a = cnt_out ? 16u : 12u;          // a field without entries is dropped, bit included
            const uint32_t len_ent = (m & H_CACHE_INVALIDATION) ? e_cih - 16u : 0u;
            const uint32_t len_ext = (append && ext > 0) ? (uint32_t)ext : 0u;
            const uint32_t len_dbg = dbg > 0 ? e_dbg - p_dbg : 0u;
            const uint32_t len_tatg = e_tg - p_ta;
            const uint32_t p_sx = (m & H_SENDING_GRAIN) ? p_sa : p_sg;    // TargetActivation only with TargetGrain
            const uint32_t len_sx = p_ta - p_sx;
            const uint32_t len_ti = (m & H_TRANSACTION_INFO_RSP) ? hw.end - p_ti : 0u;
            uint32_t info_pos = 0, info_len = 0;
            const uint32_t ix = in.info ? in.info[i] : NONE32;
            if (ix < in.n_info) {
                info_pos = in.info_off[ix];
                info_len = in.info_off[ix + 1] - info_pos;
            }
            uint32_t om = H_DIRECTION | H_RESULT | H_SENDING_GRAIN;
            if (cnt_out) om |= H_CACHE_INVALIDATION;
            if (cat) om |= H_CATEGORY;
            if (dbg > 0) om |= H_DEBUG_CONTEXT;
            if (has_ttl) om |= H_TIME_TO_LIVE;
            if (has_corr) om |= H_CORRELATION_ID;
            if (ai) om |= H_ALWAYS_INTERLEAVE;
            if (ro) om |= H_READ_ONLY;
            if (info_len) om |= H_REJECTION_INFO;
            if (m & H_TARGET_ACTIVATION) om |= H_SENDING_ACTIVATION;
            if (r_ts) om |= H_SENDING_SILO;
            if (m & H_SENDING_GRAIN) om |= H_TARGET_GRAIN | ((m & H_SENDING_ACTIVATION) ? H_TARGET_ACTIVATION : 0u);
            if (m & H_SENDING_SILO) om |= H_TARGET_SILO;
            if (m & H_TRANSACTION_INFO_RSP) om |= H_TRANSACTION_INFO_RSP;
            // record D: Direction 1 (Response) and what follows it up to the info string
            RejPack d{0, 0, 0, 0};
            d.put(1ull, 1);
            if (has_ttl) d.put(ttl, 8);
            if (has_corr) d.put(corr, 8);
            if (ai) d.put(TOKEN_TRUE, 1);
            if (ro) d.put(TOKEN_TRUE, 1);
            if (info_len) d.put(info_len, 4);
            const uint32_t len_b = 52u * ap, len_c = 28u * ap + (cat ? 1u : 0u), len_d = d.n;
            const uint32_t hb = 4u + (len_a - 12u) + len_ent + len_b + len_ext + len_c + len_dbg + len_d + info_len +
                                1u + len_tatg + r_ts + len_sx + len_ti;
            const uint32_t bl_out = in.body_off ? (uint32_t)(in.body_off[i + 1] - in.body_off[i]) : 0u;
            olen = 8u + hb + bl_out;
            // records B and C: the appended entry
            uint32_t sw[6] = {0, 0, 0, 0, 0, 0};
            uint64_t id[3] = {0, 0, 0};
            if (append) {
#pragma unroll
                for (int k = 0; k < 6; ++k) sw[k] = t.silo_wire[6ull * in.local_silo + k];
#pragma unroll
                for (int k = 0; k < 3; ++k) id[k] = t.act_ids[3ull * oa + k];
            }
            const uint32_t c0 = append ? (uint32_t)id[0] : cat;
            uint4* pp = reinterpret_cast<uint4*>(plan + (uint64_t)REJ_PLAN_DW * i);
            pp[0] = make_uint4(hb, bl_out, om, cnt_out);
            pp[1] = make_uint4(sw[0], sw[1], sw[2], sw[3]);
            pp[2] = make_uint4(sw[4], sw[5], (uint32_t)tg.n0, (uint32_t)(tg.n0 >> 32));
            pp[3] = make_uint4((uint32_t)tg.n1, (uint32_t)(tg.n1 >> 32), (uint32_t)tg.tcd, (uint32_t)(tg.tcd >> 32));
            pp[4] = make_uint4((uint32_t)ext, c0, (uint32_t)(id[0] >> 32), (uint32_t)id[1]);
            pp[5] = make_uint4((uint32_t)(id[1] >> 32), (uint32_t)id[2], (uint32_t)(id[2] >> 32), 0xFFFFFFFFu);
            pp[6] = make_uint4(cat, (uint32_t)d.w0, (uint32_t)(d.w0 >> 32), (uint32_t)d.w1);
            pp[7] = make_uint4((uint32_t)(d.w1 >> 32), (uint32_t)d.w2, (uint32_t)(d.w2 >> 32), 2u /* Rejection */);
            pp[8] = make_uint4(len_a | (len_b << 8) | (len_c << 16) | (len_d << 24), p_tg + 28u, p_dbg, p_ta);
            pp[9] = make_uint4(p_ts, p_sx, p_ti, len_ent);
            pp[10] = make_uint4(len_ext, len_dbg, len_tatg, r_ts);
            pp[11] = make_uint4(len_sx, len_ti, info_pos, info_len);
        }
    }
    out_len[i] = olen;
    rej_status[i] = (uint8_t)st;
}

// ------------------------------------------------------------------ k_rej_write: k_run_write<RejArgs>
struct RejArgs {
    static constexpr uint32_t SEGS = REJ_SEGS;
    const uint8_t* buf;
    const uint64_t* frame_off;
    const uint8_t* body;         // may be null (then every body is empty)
    const uint64_t* body_off;
    const uint32_t* order;
    const uint32_t* plan;        // REJ_PLAN_DW dwords a frame
    const uint32_t* offs;        // n + 1 scanned offsets in output order
    const uint8_t* info_utf8;
    uint32_t n;
    uint64_t out_cap;

    // Output frame j, whose first output position is fo.
    __device__ __forceinline__ void frame(uint32_t j, uint32_t fo, RunFrame<SEGS>& f) const {
        const uint32_t i = order ? min(order[j], n - 1) : j;
        const uint4* pp = reinterpret_cast<const uint4*>(plan + (uint64_t)REJ_PLAN_DW * i);
        const uint4 q0 = pp[0], q8 = pp[8], q9 = pp[9], q10 = pp[10], q11 = pp[11];
        const uint64_t src = reinterpret_cast<uint64_t>(buf + frame_off[i]);
        const uint64_t cb = reinterpret_cast<uint64_t>(pp);
        const uint64_t bd = body ? reinterpret_cast<uint64_t>(body + body_off[i]) : 0ull;
        uint32_t cur = fo;
        uint64_t prev = 0;
        RUN_SEG(f, cur, prev, 0, cb + REJ_A, q8.x & 0xFFu);
        RUN_SEG(f, cur, prev, 1, src + 16, q9.w);
        RUN_SEG(f, cur, prev, 2, cb + REJ_B, (q8.x >> 8) & 0xFFu);
        RUN_SEG(f, cur, prev, 3, src + q8.y, q10.x);
        RUN_SEG(f, cur, prev, 4, cb + REJ_C, (q8.x >> 16) & 0xFFu);
        RUN_SEG(f, cur, prev, 5, src + q8.z, q10.y);
        RUN_SEG(f, cur, prev, 6, cb + REJ_D, q8.x >> 24);
        RUN_SEG(f, cur, prev, 7, reinterpret_cast<uint64_t>(info_utf8) + q11.z, q11.w);
        RUN_SEG(f, cur, prev, 8, cb + REJ_E, 1u);
        RUN_SEG(f, cur, prev, 9, src + q8.w, q10.z);
        RUN_SEG(f, cur, prev, 10, src + q9.x, q10.w);
        RUN_SEG(f, cur, prev, 11, src + q9.y, q11.x);
        RUN_SEG(f, cur, prev, 12, src + q9.z, q11.y);
        RUN_SEG(f, cur, prev, 13, bd, q0.y);
    }
};

}  // namespace gd

