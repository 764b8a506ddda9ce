// gd_respond.h -- gfx950 device code for the response writer: batched
// MessageFactory.CreateResponseMessage / CreateRejectionResponse (MessageFactory.cs:49-111) + Message.Serialize
// (Message.cs:481-516, HeadersContainer.Serializer :1126-1244) from the request frames of a received batch.
//
// A response header is a permutation of the request's: Target* and Sending* change places, Category,
// DebugContext, TimeToLive, CorrelationId and the two True tokens are carried over, Direction, RejectionInfo,
// RejectionType and Result are written, everything else is dropped (rule and statuses: include/graindispatch.h,
// tests/_respond_ref.py).  So an output frame is RSP_SEGS byte runs laid end to end, each a copy from one of four
// places: the request frame, the frame's plan record (the written constants), the RejectionInfo table, the
// caller's body bytes.
//
//   k_rsp_kinds   turn / receive statuses -> kind and rejection type, one lane a message
//   k_silo_index  24-B wire SiloAddress -> index in the encoder's silo table (staged in LDS, six dwords compared)
//   k_rsp_plan    one lane per frame: the decoder's staging and walk (gd_frames.h) to the copied runs; writes one
//                 128-B RspPlan a frame -- 12 (source position, length) runs in output order and the constants --
//                 its output length and its status
//   k_enc_lens, scan_device, k_enc_finish (gd_frameout.h): the offsets and the capacity check, as the encoder
//   k_rsp_write   the hot path: k_run_write<RspArgs> (gd_frameout.h), the writer the forward and the rejection
//                 stage use too.  RspArgs::frame turns a frame's plan into the RSP_SEGS run starts (prefix sums,
//                 registers); the writer resolves each 16-B chunk of the output against them.
//
// Totals are 32-bit: the host refuses (GD_EINVAL) a call whose bound reaches 2^32, so gd_scan.h's scan serves.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_frameout.h"
#include "gd_frames.h"
#include "gd_hash.h"

namespace gd {

// GD_RSP_* / GD_RSPST_* (include/graindispatch.h)
enum : uint32_t { RSP_NONE = 0, RSP_RESPONSE = 1, RSP_REJECTION = 2 };
enum : uint32_t { RSPST_OK = 0, RSPST_SKIPPED = 1, RSPST_MALFORMED = 2, RSPST_DISCARDED = 3, RSPST_FALLBACK = 4 };
constexpr uint32_t H_TRANSACTION_INFO_RSP = 1u << 27;
constexpr uint32_t RSP_RUNS = 12;            // copied runs of the request frame
constexpr uint32_t RSP_SEGS = 18;            // runs of an output frame
// GD_TURN_* / GD_RECV_* read by k_rsp_kinds, Message.RejectionTypes written
constexpr uint32_t RSP_TURN_REJECT_OVERLOADED = 3, RSP_TURN_REJECT_TRANSIENT = 6;
constexpr uint32_t RSP_RECV_REJECT_UNKNOWN = 3, RSP_RECV_REJECT_OVERLOADED = 4;
constexpr uint32_t REJ_TRANSIENT = 0, REJ_OVERLOADED = 1, REJ_UNRECOVERABLE = 3;

// One frame's plan, 128 B.  Runs in output order, positions in bytes from the frame start in the SOURCE:
//   0 Category + DebugContext   1 TimeToLive   2 CorrelationId   3 AlwaysInterleave   4 ReadOnly
//   5 TargetActivation (-> SendingActivation)   6 TargetGrain   7 TargetSilo
//   8 SendingActivation (-> TargetActivation)   9 SendingGrain  10 SendingSilo   11 TransactionInfo
// c: the written bytes -- [0,4) headerLength, [4,8) bodyLength, [8,12) mask, [12] Direction, [13,17) the
// RejectionInfo length, [17] RejectionType, [18] Result.  flags: bit 0 RejectionInfo, bit 1 RejectionType, bit 2
// Result are written.  Only OK frames have a plan that is read.
struct RspPlan {
    uint32_t pos[RSP_RUNS];
    uint32_t len[RSP_RUNS];
    uint8_t c[20];
    uint32_t info_pos;       // the string's first byte in the info table
    uint32_t flags;
    uint32_t pad;
};
static_assert(sizeof(RspPlan) == 128, "plan record is 128 B");

// ------------------------------------------------------------------ k_rsp_kinds
static __global__ __launch_bounds__(BLOCK) void k_rsp_kinds(const uint8_t* __restrict__ turn,
                                                     const uint8_t* __restrict__ recv, uint32_t n,
                                                     uint8_t* __restrict__ kind, uint8_t* __restrict__ rej) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = turn[i];
    uint32_t k = RSP_NONE, r = REJ_TRANSIENT;
    if (t == RSP_TURN_REJECT_OVERLOADED) {
        k = RSP_REJECTION;
        r = REJ_OVERLOADED;
    } else if (t == RSP_TURN_REJECT_TRANSIENT) {
        k = RSP_REJECTION;
    } else if (recv) {
        const uint32_t s = recv[i];
        if (s == RSP_RECV_REJECT_UNKNOWN) {
            k = RSP_REJECTION;
            r = REJ_UNRECOVERABLE;
        } else if (s == RSP_RECV_REJECT_OVERLOADED) {
            k = RSP_REJECTION;
            r = REJ_OVERLOADED;
        }
    }
    kind[i] = (uint8_t)k;
    rej[i] = (uint8_t)r;
}

// ------------------------------------------------------------------ k_silo_index
constexpr uint32_t SILO_STAGE = 1024;        // silo addresses staged at a time (24 KiB of LDS)

// wire: 6 dwords a message (4-B aligned); the lowest index whose address equals it, NONE32 when there is none.
static __global__ __launch_bounds__(BLOCK) void k_silo_index(const uint32_t* __restrict__ wire, uint32_t n,
                                                      const uint32_t* __restrict__ tab, uint32_t n_silos,
                                                      uint32_t* __restrict__ silo) {
    __shared__ uint32_t s_tab[SILO_STAGE * 6];
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t w[6] = {0, 0, 0, 0, 0, 0};
    if (i < n) {
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k] = wire[6ull * i + k];
    }
    uint32_t found = NONE32;
    for (uint32_t base = 0; base < n_silos; base += SILO_STAGE) {
        const uint32_t cnt = min(SILO_STAGE, n_silos - base);
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < cnt * 6; k += BLOCK) s_tab[k] = tab[6ull * base + k];
        __syncthreads();
        if (found == NONE32) {
            for (uint32_t s = 0; s < cnt; ++s) {
                const uint32_t* e = &s_tab[6 * s];
                if (((e[0] ^ w[0]) | (e[1] ^ w[1]) | (e[2] ^ w[2]) | (e[3] ^ w[3]) | (e[4] ^ w[4]) | (e[5] ^ w[5])) == 0) {
                    found = base + s;
                    break;
                }
            }
        }
    }
    if (i < n) silo[i] = found;
}

// ------------------------------------------------------------------ k_rsp_plan
struct RspIn {
    const uint8_t* kind;
    const uint8_t* result;           // may be null: Success
    const uint8_t* rejection_type;   // may be null: Transient
    const uint32_t* info;            // may be null: no info
    const uint64_t* body_off;        // may be null: empty bodies
    const uint32_t* info_off;        // n_info + 1
    uint32_t n_info;
};

// WALK (GD_OPT_WALK_INVALIDATION): a CacheInvalidationHeader is stepped over.  CreateResponseMessage copies the
// header (MessageFactory.cs:90) and the field stands directly in front of Category in the request and in the
// answer, so its bytes [12, p0) join run 0 when it has entries; with none the answer drops the bit, as the
// Deserializer builds no list then (Message.cs:1254-1265).  Run 0 has to stay one run: a frame with entries, a
// Category byte of the enum's default (dropped) and a DebugContext behind it (kept) is RSPST_FALLBACK where it
// would have been RSPST_OK.  Without WALK every frame with the field is RSPST_FALLBACK.
template <bool WALK = false>
static __global__ __launch_bounds__(BLOCK) void k_rsp_plan(const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                    const uint64_t* __restrict__ frame_off, uint32_t n, RspIn in,
                                                    RspPlan* __restrict__ plan, uint32_t* __restrict__ out_len,
                                                    uint8_t* __restrict__ rsp_status) {
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

    uint32_t pos[RSP_RUNS], len[RSP_RUNS];
#pragma unroll
    for (uint32_t k = 0; k < RSP_RUNS; ++k) pos[k] = len[k] = 0;
    uint32_t st = RSPST_SKIPPED, olen = 0, om = 0, flags = 0, info_pos = 0, info_len = 0, rt = 0, res = 0, hl_out = 0,
             bl_out = 0;
    bool split0 = false;                             // WALK only: run 0 would be two runs
    const uint32_t kind = in.kind[i];
    if (kind == RSP_RESPONSE || kind == RSP_REJECTION) {
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
            st = RSPST_MALFORMED;
        } else {
            hw.p = 12;
            hw.end = 8u + (uint32_t)hl;
            const uint32_t m = hw.c.u32(8);
            st = RSPST_OK;
            if (!WALK && (m & H_CACHE_INVALIDATION)) {
                st = RSPST_FALLBACK;                 // object-serialized ahead of Direction: nothing can be read
            } else {
                // HeadersContainer.Serializer order (Message.cs:1126-1244)
                const bool cih = WALK && (m & H_CACHE_INVALIDATION) && hw.skip_invalidation() > 0;
                const uint32_t p0 = hw.p;
                uint32_t cat = 0;
                if ((m & H_CATEGORY) && hw.take(1)) cat = hw.c.u8(hw.p - 1);
                const uint32_t p_dbg = hw.p;
                int32_t dbg = -1;
                if (m & H_DEBUG_CONTEXT) dbg = hw.skip_string();
                const uint32_t e_dbg = hw.p;
                uint32_t dir = 0;
                if ((m & H_DIRECTION) && !hw.bad && hw.take(1)) dir = hw.c.u8(hw.p - 1);
                if (hw.bad) {
                    st = RSPST_MALFORMED;
                } else if (dir != 0) {
                    st = RSPST_DISCARDED;            // RejectMessage :209-221: only a Request is answered
                } else if ((m & H_REQUEST_CONTEXT) || ((m & H_TARGET_OBSERVER) && (m & H_TRANSACTION_INFO_RSP))) {
                    st = RSPST_FALLBACK;
                } else {
                    // run 0: Category (when not the enum default) and DebugContext (when not empty) are adjacent
                    const uint32_t b0 = (cat != 0) ? p0 : p_dbg;
                    const uint32_t b1 = (dbg > 0) ? e_dbg : p_dbg;
                    pos[0] = b0;
                    len[0] = b1 > b0 ? b1 - b0 : 0u;
                    if (WALK && cih) {               // ... and the entries stand in front of them
                        split0 = p_dbg != p0 && cat == 0 && dbg > 0;     // a dropped byte between the two
                        pos[0] = 12;
                        len[0] = ((cat != 0 || dbg > 0) ? b1 : p0) - 12;
                        om |= H_CACHE_INVALIDATION;
                    }
                    if (cat != 0) om |= H_CATEGORY;
                    if (dbg > 0) om |= H_DEBUG_CONTEXT;
                    if ((m & H_TIME_TO_LIVE) && hw.take(8)) {
                        pos[1] = hw.p - 8;
                        len[1] = 8;
                        om |= H_TIME_TO_LIVE;
                    }
                    if (m & H_FORWARD_COUNT) hw.take(4);
                    if (m & H_GENERIC_GRAIN_TYPE) hw.skip_string();
                    if ((m & H_CORRELATION_ID) && !hw.bad && hw.take(8)) {
                        pos[2] = hw.p - 8;
                        len[2] = 8;
                        om |= H_CORRELATION_ID;
                    }
                    if ((m & H_ALWAYS_INTERLEAVE) && !hw.bad && hw.take(1) && hw.c.u8(hw.p - 1) == TOKEN_TRUE) {
                        pos[3] = hw.p - 1;
                        len[3] = 1;
                        om |= H_ALWAYS_INTERLEAVE;
                    }
                    if ((m & H_IS_NEW_PLACEMENT) && !hw.bad) hw.take(1);
                    if ((m & H_READ_ONLY) && !hw.bad && hw.take(1) && hw.c.u8(hw.p - 1) == TOKEN_TRUE) {
                        pos[4] = hw.p - 1;
                        len[4] = 1;
                        om |= H_READ_ONLY;
                    }
                    if ((m & H_IS_UNORDERED) && !hw.bad) hw.take(1);
                    if (m & H_NEW_GRAIN_TYPE) hw.skip_string();
                    if (m & H_REJECTION_INFO) hw.skip_string();
                    if ((m & H_REJECTION_TYPE) && !hw.bad) hw.take(1);
                    if ((m & H_RESEND_COUNT) && !hw.bad) hw.take(4);
                    if ((m & H_RESULT) && !hw.bad) hw.take(1);
                    // the request's Sending* become the answer's Target* (runs 8-10) ...
                    const uint32_t p_sa = hw.p;
                    if (m & H_SENDING_ACTIVATION) hw.key(nullptr);
                    const uint32_t p_sg = hw.p;
                    if (m & H_SENDING_GRAIN) hw.key(nullptr);
                    const uint32_t p_ss = hw.p;
                    if ((m & H_SENDING_SILO) && !hw.bad) hw.take(24);
                    // ... and its Target* the answer's Sending* (runs 5-7)
                    const uint32_t p_ta = hw.p;
                    if (m & H_TARGET_ACTIVATION) hw.key(nullptr);
                    const uint32_t p_tg = hw.p;
                    Key3 tg{0, 0, 0};
                    if (m & H_TARGET_GRAIN) tg = hw.key(nullptr);
                    const uint32_t e_tg = hw.p;
                    if (hw.bad) {
                        st = RSPST_MALFORMED;
                    } else if ((m & H_TARGET_GRAIN) && !(m & H_TARGET_ACTIVATION) &&
                               (uint32_t)(tg.tcd >> 56) == CAT_SYSTEM_TARGET) {
                        st = RSPST_FALLBACK;         // ActivationId.GetSystemActivation (MessageFactory.cs:79-82)
                    } else {
                        const uint32_t r_ts = (m & H_TARGET_SILO) ? 24u : 0u;
                        uint32_t p_ts = hw.p;
                        if (m & H_TARGET_OBSERVER) {
                            // object-serialized, no TransactionInfo behind it: TargetSilo is the header's last field
                            if (hw.end - hw.p < r_ts) hw.bad = true;
                            p_ts = hw.end - r_ts;
                            hw.p = hw.end;
                        } else if (r_ts) {
                            hw.take(24);
                        }
                        if (hw.bad) {
                            st = RSPST_MALFORMED;
                        } else {
                            if (m & H_TARGET_GRAIN) {
                                if (m & H_TARGET_ACTIVATION) {
                                    pos[5] = p_ta;
                                    len[5] = p_tg - p_ta;
                                    om |= H_SENDING_ACTIVATION;
                                }
                                pos[6] = p_tg;
                                len[6] = e_tg - p_tg;
                                om |= H_SENDING_GRAIN;
                            }
                            if (r_ts) {
                                pos[7] = p_ts;
                                len[7] = 24;
                                om |= H_SENDING_SILO;
                            }
                            if (m & H_SENDING_GRAIN) {
                                if (m & H_SENDING_ACTIVATION) {
                                    pos[8] = p_sa;
                                    len[8] = p_sg - p_sa;
                                    om |= H_TARGET_ACTIVATION;
                                }
                                pos[9] = p_sg;
                                len[9] = p_ss - p_sg;
                                om |= H_TARGET_GRAIN;
                            }
                            if (m & H_SENDING_SILO) {
                                pos[10] = p_ss;
                                len[10] = 24;
                                om |= H_TARGET_SILO;
                            }
                            if (m & H_TRANSACTION_INFO_RSP) {
                                pos[11] = hw.p;
                                len[11] = hw.end - hw.p;
                                om |= H_TRANSACTION_INFO_RSP;
                            }
                            om |= H_DIRECTION;
                            if (kind == RSP_REJECTION) {
                                res = 2;                                    // ResponseTypes.Rejection
                                rt = in.rejection_type ? in.rejection_type[i] : REJ_TRANSIENT;
                                const uint32_t ix = in.info ? in.info[i] : NONE32;
                                if (ix < in.n_info) {
                                    info_pos = in.info_off[ix];
                                    info_len = in.info_off[ix + 1] - info_pos;
                                }
                            } else if (in.result && in.result[i] == 1) {
                                res = 1;                                    // ResponseTypes.Error
                            }
                            if (info_len) {
                                flags |= 1u;
                                om |= H_REJECTION_INFO;
                            }
                            if (rt) {
                                flags |= 2u;
                                om |= H_REJECTION_TYPE;
                            }
                            if (res) {
                                flags |= 4u;
                                om |= H_RESULT;
                            }
                            uint32_t hb = 4 + 1 + (info_len ? 4 + info_len : 0u) + (rt ? 1u : 0u) + (res ? 1u : 0u);
#pragma unroll
                            for (uint32_t k = 0; k < RSP_RUNS; ++k) hb += len[k];
                            hl_out = hb;
                            if (in.body_off) bl_out = (uint32_t)(in.body_off[i + 1] - in.body_off[i]);
                            olen = 8 + hl_out + bl_out;
                        }
                    }
                }
            }
        }
    }
    if (WALK && split0 && st == RSPST_OK) st = RSPST_FALLBACK;
    if (st == RSPST_OK) {
        uint4* pp = reinterpret_cast<uint4*>(plan + i);
        pp[0] = make_uint4(pos[0], pos[1], pos[2], pos[3]);
        pp[1] = make_uint4(pos[4], pos[5], pos[6], pos[7]);
        pp[2] = make_uint4(pos[8], pos[9], pos[10], pos[11]);
        pp[3] = make_uint4(len[0], len[1], len[2], len[3]);
        pp[4] = make_uint4(len[4], len[5], len[6], len[7]);
        pp[5] = make_uint4(len[8], len[9], len[10], len[11]);
        // c[12] Direction = 1 (Response), c[13..17) the info length, c[17] RejectionType, c[18] Result
        pp[6] = make_uint4(hl_out, bl_out, om, 1u | (info_len << 8));
        pp[7] = make_uint4((info_len >> 24) | ((rt & 0xFFu) << 8) | (res << 16), info_pos, flags, 0u);
    } else {
        olen = 0;
    }
    out_len[i] = olen;
    rsp_status[i] = (uint8_t)st;
}

// ------------------------------------------------------------------ k_rsp_write: k_run_write<RspArgs>
struct RspArgs {
    static constexpr uint32_t SEGS = RSP_SEGS;
    const uint8_t* buf;
    const uint64_t* frame_off;
    const uint8_t* body;         // may be null (then every body is empty)
    const uint64_t* body_off;
    const uint32_t* order;
    const RspPlan* plan;
    const uint32_t* offs;        // n + 1 scanned offsets in output order
    const uint8_t* info_utf8;
    uint32_t n;
    uint64_t out_cap;

    // Output frame j, whose first output position is fo.
    __device__ __forceinline__ void frame(uint32_t j, uint32_t fo, RunFrame<SEGS>& f) const {
        const uint32_t i = order ? min(order[j], n - 1) : j;
        const uint4* pp = reinterpret_cast<const uint4*>(plan + i);
        const uint4 q0 = pp[0], q1 = pp[1], q2 = pp[2], q3 = pp[3], q4 = pp[4], q5 = pp[5], q6 = pp[6], q7 = pp[7];
        const uint64_t src = reinterpret_cast<uint64_t>(buf + frame_off[i]);
        const uint64_t cb = reinterpret_cast<uint64_t>(plan + i) + 2 * RSP_RUNS * 4;     // RspPlan::c
        const uint32_t info_len = (q6.w >> 8) | (q7.x << 24), fl = q7.z;
        const uint64_t bd = body ? reinterpret_cast<uint64_t>(body + body_off[i]) : 0ull;
        uint32_t cur = fo;
        uint64_t prev = 0;
        RUN_SEG(f, cur, prev, 0, cb, 12);
        RUN_SEG(f, cur, prev, 1, src + q0.x, q3.x);
        RUN_SEG(f, cur, prev, 2, cb + 12, 1);
        RUN_SEG(f, cur, prev, 3, src + q0.y, q3.y);
        RUN_SEG(f, cur, prev, 4, src + q0.z, q3.z);
        RUN_SEG(f, cur, prev, 5, src + q0.w, q3.w);
        RUN_SEG(f, cur, prev, 6, src + q1.x, q4.x);
        RUN_SEG(f, cur, prev, 7, cb + 13, (fl & 1u) ? 4u : 0u);
        RUN_SEG(f, cur, prev, 8, reinterpret_cast<uint64_t>(info_utf8) + q7.y, info_len);
        RUN_SEG(f, cur, prev, 9, cb + ((fl & 2u) ? 17 : 18), ((fl >> 1) & 1u) + ((fl >> 2) & 1u));
        RUN_SEG(f, cur, prev, 10, src + q1.y, q4.y);
        RUN_SEG(f, cur, prev, 11, src + q1.z, q4.z);
        RUN_SEG(f, cur, prev, 12, src + q1.w, q4.w);
        RUN_SEG(f, cur, prev, 13, src + q2.x, q5.x);
        RUN_SEG(f, cur, prev, 14, src + q2.y, q5.y);
        RUN_SEG(f, cur, prev, 15, src + q2.z, q5.z);
        RUN_SEG(f, cur, prev, 16, src + q2.w, q5.w);
        RUN_SEG(f, cur, prev, 17, bd, q6.y);
    }
};

}  // namespace gd

