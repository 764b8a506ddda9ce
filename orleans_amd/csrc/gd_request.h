// gd_request.h -- gfx950 device code for the request writer: batched MessageFactory.CreateMessage
// (MessageFactory.cs:21-47) + InsideRuntimeClient.SendRequestMessage (InsideRuntimeClient.cs:120-229) +
// Message.SetTargetPlacement (Message.cs:629-639) + Message.Serialize (Message.cs:481-516, HeadersContainer.
// Serializer :1126-1245).  The third frame writer: gd_encode.h patches a frame, gd_respond.h answers one, this one
// makes one -- there is no source frame, every header byte comes from a few words per message and the handle's
// tables.  Rule and statuses: include/graindispatch.h, tests/_request_ref.py.
//
//   k_req_plan    one lane per message: the status, the mask and the field lengths, as one 32-B ReqPlan; the
//                 frame's output length.  The record holds lengths only: table indexes stay in the caller's arrays,
//                 where the one lane that writes the field reads them.
//   k_enc_lens, scan_device, k_enc_finish (gd_frameout.h)   the offsets in output order and the capacity check
//   k_req_ttl     the send stage's per-message TimeToLive from the batch ttl and the options (the chain only)
//   k_req_write   the hot path.  The output is cut as k_enc_write cuts it: 16-KiB tiles of 16-B chunks at absolute
//                 16-B addresses, one owner per chunk, nothing written outside [0, out_off[n]).  A tile is built in
//                 two phases.  (1) Sixteen lanes take one frame that meets the tile, resolve its layout once from
//                 the plan, and assemble it in the tile's LDS image: twelve lanes write one fixed field each (the
//                 12-B prefix + Category ... TargetSilo, dword loads from the key / ActivationId / silo tables),
//                 then all sixteen copy the strings (DebugContext, GenericGrainType, NewGrainType, the two KeyExt)
//                 and the body's ragged head and tail byte by byte; for every 16-B chunk that lies wholly inside
//                 the body they note the body address in LDS instead.  (2) Every lane takes chunks: a noted chunk
//                 is one 16-B load from `body` (dword aligned + alignbyte), any other is one 16-B LDS read; both
//                 leave as one aligned 16-B store.  No lane searches for its frame or re-derives a layout per
//                 chunk; only the first and last chunk of the whole output use byte stores.
//
// Totals are 32-bit (gd_scan.h's scan): the host refuses what it can bound (eng_request.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_encode.h"
#include "gd_frameout.h"

namespace gd {

// GD_REQ_* statuses and option bits (include/graindispatch.h)
enum : uint32_t { REQ_OK = 0, REQ_UNADDRESSED = 1, REQ_FALLBACK = 2, REQ_NO_ID = 3, REQ_NO_SILO = 4 };
enum : uint32_t { REQ_ONE_WAY = 1, REQ_NO_TTL = 2, REQ_ALWAYS_INTERLEAVE = 4, REQ_READ_ONLY = 8, REQ_UNORDERED = 16,
                  REQ_IFACE_VERSION = 32, REQ_TXN_REQUIRED = 64 };
constexpr uint32_t H_IFACE_VERSION = 1u << 26, H_TXN_REQUIRED = 1u << 28;      // mask-only bits
constexpr uint32_t REQ_MAX_STR = 0xFFF0u;    // longest DebugContext / GenericGrainType string (16 bits in the plan)
constexpr uint32_t REQ_FIXED = 206;          // frame bytes besides the strings, the KeyExt and the body, at most
constexpr long long REQ_TTL_NONE = 0x7FFFFFFFFFFFFFFFll;                       // GD_TTL_NONE
constexpr uint32_t REQ_CAT_SYSTEM_TARGET = 1;                                  // UniqueKey category (TypeCodeData >> 56)
constexpr uint32_t REQ_GROUP = 16;                                             // lanes that share one frame
constexpr uint32_t REQ_TILE = ENC_TILE_CHUNKS * 16;

// The batch as the kernels see it; device pointers.  Keys are 3 x u64 (n0, n1, type_code_data).  Null: text_len /
// sext_len (no KeyExt), options, generic, debug, body + body_off, and the five route arrays (silo + act + status go
// together).
struct ReqIn {
    const uint64_t* target;
    const uint8_t* text;
    const uint64_t* text_off;
    const int32_t* text_len;
    uint64_t text_bytes;
    const uint64_t* sender;
    const uint8_t* sext;
    const uint64_t* sext_off;
    const int32_t* sext_len;
    uint64_t sext_bytes;
    const uint32_t* sender_act;
    const uint8_t* options;
    const uint32_t* generic;
    const uint32_t* debug;
    const uint8_t* body;
    const uint64_t* body_off;
    const uint32_t* silo;
    const uint32_t* act;
    const uint8_t* status;
    const uint8_t* placed;
    const uint32_t* new_type;
    long long id_base, ttl;
};

struct ReqTab {
    EncTab e;                    // ActivationIds, wire silos, grain-class names (gd_encode_configure)
    const uint8_t* str_utf8;     // gd_request_configure's strings
    const uint32_t* str_off;     // n_str + 1
    uint32_t n_str;
    uint32_t my_silo;
};

// One message's plan, 32 B.  Lengths are string bytes without the int32 prefix; 0: the field is absent.
// Messages that contribute no bytes keep tail = status and zeros.
struct ReqPlan {
    uint32_t mask;
    uint32_t tail;               // status | one-way << 8
    uint32_t dbg_gen;            // DebugContext | GenericGrainType << 16
    uint32_t ngt;                // NewGrainType
    int32_t text, sext;          // KeyExt of TargetGrain / SendingGrain; -1: null
    uint32_t body_len;
    uint32_t hdr;                // 8 + headerLength: the body's first byte in the frame
};
static_assert(sizeof(ReqPlan) == 32, "plan record is 32 B");

// Where the fields start in the frame, Serializer order: [0,12) lengths and mask, [12] Category, [13] DebugContext,
// Direction, TimeToLive, GenericGrainType, CorrelationId, the True tokens, NewGrainType, SendingActivation (28),
// SendingGrain (28 + KeyExt), SendingSilo (24), TargetActivation (28), TargetGrain (28 + KeyExt), TargetSilo (24).
struct ReqLay {
    uint32_t o_dir, o_gen, o_cid, ntok, o_ngt, o_sa, o_sx, o_ss, o_ta, o_tg, o_tx, o_ts, hdr;
};

__device__ __forceinline__ ReqLay req_layout(uint32_t mask, uint32_t dbg, uint32_t gen, uint32_t ngt, int32_t text,
                                             int32_t sext) {
    ReqLay l;
    const uint32_t addressed = mask & H_TARGET_ACTIVATION;
    l.o_dir = 13 + (dbg ? 4 + dbg : 0);
    l.o_gen = l.o_dir + 1 + ((mask & H_TIME_TO_LIVE) ? 8 : 0);
    l.o_cid = l.o_gen + (gen ? 4 + gen : 0);
    l.ntok = __popc(mask & (H_ALWAYS_INTERLEAVE | H_IS_NEW_PLACEMENT | H_READ_ONLY | H_IS_UNORDERED));
    l.o_ngt = l.o_cid + 8 + l.ntok;
    l.o_sa = l.o_ngt + (ngt ? 4 + ngt : 0);
    l.o_sx = l.o_sa + 56;
    l.o_ss = l.o_sx + (sext > 0 ? (uint32_t)sext : 0u);
    l.o_ta = l.o_ss + 24;
    l.o_tg = l.o_ta + (addressed ? 28 : 0);
    l.o_tx = l.o_tg + 28;
    l.o_ts = l.o_tx + (text > 0 ? (uint32_t)text : 0u);
    l.hdr = l.o_ts + (addressed ? 24 : 0);
    return l;
}

// ------------------------------------------------------------------ k_req_plan
// A KeyExt length the device writes: -1, or a string inside the batch's bytes.  Anything else is left to C#.
__device__ __forceinline__ int32_t req_ext(const int32_t* len, const uint64_t* off, uint64_t bytes, uint32_t i,
                                           bool& fallback) {
    if (!len) return -1;
    const int32_t l = len[i];
    if (l < -1) fallback = true;
    if (l > 0) {
        const uint64_t o = off[i];
        if (o > bytes || bytes - o < (uint64_t)l) fallback = true;
    }
    return fallback ? -1 : l;
}

// The byte length of string idx of a table (0: no index, past the table, or empty).
__device__ __forceinline__ uint32_t req_str_len(const uint32_t* idx, uint32_t i, const uint32_t* off, uint32_t n_tab) {
    if (!idx) return 0;
    const uint32_t k = idx[i];
    return k < n_tab ? off[k + 1] - off[k] : 0u;
}

static __global__ __launch_bounds__(BLOCK) void k_req_plan(ReqIn in, ReqTab t, uint32_t n, ReqPlan* __restrict__ plan,
                                                    uint32_t* __restrict__ out_len,
                                                    uint8_t* __restrict__ req_status) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t opt = in.options ? in.options[i] : 0u;
    bool fallback = false;
    const int32_t text = req_ext(in.text_len, in.text_off, in.text_bytes, i, fallback);
    const int32_t sext = req_ext(in.sext_len, in.sext_off, in.sext_bytes, i, fallback);
    const bool routed = in.status && in.status[i] == 0 /* GD_ROUTE_OK */;
    uint32_t st;
    if (fallback) st = REQ_FALLBACK;
    else if ((uint32_t)(in.target[3ull * i + 2] >> 56) == REQ_CAT_SYSTEM_TARGET) st = REQ_FALLBACK;
    else if (!enc_has_id(t.e, in.sender_act[i])) st = REQ_NO_ID;
    else if (routed && in.silo[i] >= t.e.n_silos) st = REQ_NO_SILO;
    else if (routed && !enc_has_id(t.e, in.act[i])) st = REQ_NO_ID;
    else st = routed ? REQ_OK : REQ_UNADDRESSED;

    ReqPlan p{0, st, 0, 0, -1, -1, 0, 0};
    uint32_t olen = 0;
    if (st == REQ_OK || st == REQ_UNADDRESSED) {
        const bool addressed = st == REQ_OK;
        const bool one_way = opt & REQ_ONE_WAY;
        const uint32_t dbg = req_str_len(in.debug, i, t.str_off, t.n_str);
        const uint32_t gen = req_str_len(in.generic, i, t.str_off, t.n_str);
        const uint32_t ngt = addressed ? req_str_len(in.new_type, i, t.e.type_off, t.e.n_types) : 0u;
        const bool ttl = in.ttl != REQ_TTL_NONE && !one_way && !(opt & REQ_NO_TTL);
        const bool is_new = addressed && in.placed && in.placed[i] == ENC_PLACED_NEW;
        p.mask = H_CATEGORY | H_DIRECTION | H_CORRELATION_ID | H_SENDING_ACTIVATION | H_SENDING_GRAIN |
                 H_SENDING_SILO | H_TARGET_GRAIN | (dbg ? H_DEBUG_CONTEXT : 0u) | (ttl ? H_TIME_TO_LIVE : 0u) |
                 (gen ? H_GENERIC_GRAIN_TYPE : 0u) | ((opt & REQ_ALWAYS_INTERLEAVE) ? H_ALWAYS_INTERLEAVE : 0u) |
                 ((opt & REQ_READ_ONLY) ? H_READ_ONLY : 0u) | ((opt & REQ_UNORDERED) ? H_IS_UNORDERED : 0u) |
                 (is_new ? H_IS_NEW_PLACEMENT : 0u) | (ngt ? H_NEW_GRAIN_TYPE : 0u) |
                 (addressed ? (H_TARGET_ACTIVATION | H_TARGET_SILO) : 0u) |
                 ((opt & REQ_IFACE_VERSION) ? H_IFACE_VERSION : 0u) | ((opt & REQ_TXN_REQUIRED) ? H_TXN_REQUIRED : 0u);
        p.tail = st | (one_way ? 0x100u : 0u);
        p.dbg_gen = dbg | (gen << 16);
        p.ngt = ngt;
        p.text = text;
        p.sext = sext;
        p.body_len = in.body_off ? (uint32_t)(in.body_off[i + 1] - in.body_off[i]) : 0u;
        p.hdr = req_layout(p.mask, dbg, gen, ngt, text, sext).hdr;
        olen = p.hdr + p.body_len;
    }
    uint4* pp = reinterpret_cast<uint4*>(plan + i);
    pp[0] = make_uint4(p.mask, p.tail, p.dbg_gen, p.ngt);
    pp[1] = make_uint4((uint32_t)p.text, (uint32_t)p.sext, p.body_len, p.hdr);
    out_len[i] = olen;
    req_status[i] = (uint8_t)st;
}

// The TimeToLive each message carries into gd_send_queues: the batch's, unless the frame has none.
static __global__ __launch_bounds__(BLOCK) void k_req_ttl(const uint8_t* __restrict__ options, long long ttl,
                                                   uint32_t n, long long* __restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t opt = options ? options[i] : 0u;
    out[i] = (opt & (REQ_ONE_WAY | REQ_NO_TTL)) ? REQ_TTL_NONE : ttl;
}

// ------------------------------------------------------------------ k_req_write
struct ReqArgs {
    ReqIn in;
    const uint32_t* order;
    const ReqPlan* plan;
    const uint32_t* offs;        // n + 1 scanned offsets in output order
    uint32_t n;
    uint64_t out_cap;
};

// Up to 4 bytes of w at image position p (which may lie outside the tile: those bytes belong to another tile).
__device__ __forceinline__ void req_put(uint8_t* img, long long p, uint32_t w, uint32_t cnt) {
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
        if (b < cnt && (unsigned long long)(p + b) < REQ_TILE) img[p + b] = (uint8_t)(w >> (8 * b));
}

// src[0, len) to image position p on, the group's sixteen lanes together, the part inside the tile only.
__device__ __forceinline__ void req_copy(uint8_t* img, long long p, const uint8_t* src, uint32_t len, uint32_t g) {
    const long long lo = p < 0 ? -p : 0;
    const long long hi = p + (long long)len > (long long)REQ_TILE ? (long long)REQ_TILE - p : (long long)len;
    for (long long k = lo + g; k < hi; k += REQ_GROUP) img[p + k] = src[k];
}

static __global__ __launch_bounds__(BLOCK) void k_req_write(ReqArgs a, ReqTab t, uint8_t* __restrict__ out) {
    __shared__ uint4 s_img[ENC_TILE_CHUNKS];                        // the tile's bytes
    __shared__ unsigned long long s_src[ENC_TILE_CHUNKS];           // a whole-body chunk's source address, else 0
    __shared__ uint32_t s_rng[2];
    const uint32_t n = a.n;
    const uint32_t total = a.offs[n];
    if (total == 0 || (uint64_t)total > a.out_cap) return;          // too long: k_enc_finish raised ERR_ENC_FULL
    // chunk c holds output positions [16 c - lead, 16 c - lead + 16): absolute 16-B addresses (as k_enc_write)
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u);
    const uint64_t t0 = (uint64_t)blockIdx.x * REQ_TILE;            // in lead-shifted coordinates
    if (t0 >= (uint64_t)total + lead) return;
    const uint32_t first = (uint32_t)(t0 > lead ? t0 - lead : 0);   // the tile's first output position
    const uint64_t t1 = t0 + (uint64_t)REQ_TILE - lead;
    const uint32_t last = (uint32_t)(t1 < total ? t1 : total) - 1;  // ... and its last
    if (threadIdx.x < 2) s_rng[threadIdx.x] = enc_find(a.offs, 0, 0, n - 1, threadIdx.x ? last : first);
    for (uint32_t k = threadIdx.x; k < ENC_TILE_CHUNKS; k += BLOCK) s_src[k] = 0ull;
    __syncthreads();
    const uint32_t jlo = s_rng[0], jhi = s_rng[1];
    uint8_t* img = reinterpret_cast<uint8_t*>(s_img);
    const long long base = (long long)t0 - lead;                    // image byte p is output position base + p
    const ReqIn& in = a.in;

    // ---- phase 1: sixteen lanes a frame
    const uint32_t g = threadIdx.x % REQ_GROUP;
    for (uint64_t jj = (uint64_t)jlo + threadIdx.x / REQ_GROUP; jj <= jhi; jj += BLOCK / REQ_GROUP) {
        const uint32_t j = (uint32_t)jj;
        const uint32_t fo = a.offs[j];
        if (a.offs[j + 1] == fo) continue;                          // contributes no bytes
        const uint32_t i = a.order ? min(a.order[j], n - 1) : j;
        const uint4* pp = reinterpret_cast<const uint4*>(a.plan + i);
        const uint4 p0 = pp[0], p1 = pp[1];
        const uint32_t mask = p0.x, dbg = p0.z & 0xFFFFu, gen = p0.z >> 16, ngt = p0.w, body_len = p1.z;
        const int32_t text = (int32_t)p1.x, sext = (int32_t)p1.y;
        const ReqLay l = req_layout(mask, dbg, gen, ngt, text, sext);
        const long long rel = (long long)fo - base;                 // image position of the frame's first byte
        const bool addressed = mask & H_TARGET_ACTIVATION;

        // the fixed fields, one a lane: `len` bytes at frame byte y, from src (six dwords, then w0) or from w0..w3
        uint32_t y = 0, len = 0, w0 = 0, w1 = 0, w2 = 0, w3 = 0, field = g;
        auto inside = [&](uint32_t yy, uint32_t ll) { return rel + yy < (long long)REQ_TILE && rel + yy + ll > 0; };
        switch (g) {
            case 0: y = 0, len = 13, w0 = l.hdr - 8, w1 = body_len, w2 = mask, w3 = 2; break;   // Categories.Application
            case 1: y = 13, len = dbg ? 4 : 0, w0 = dbg; break;
            case 2: {
                const unsigned long long ttl = (unsigned long long)in.ttl;
                y = l.o_dir, len = (mask & H_TIME_TO_LIVE) ? 9 : 1;
                w0 = ((p0.y & 0x100u) ? 2u : 0u) | (uint32_t)(ttl << 8), w1 = (uint32_t)(ttl >> 24), w2 = (uint32_t)(ttl >> 56);
                break;
            }
            case 3: y = l.o_gen, len = gen ? 4 : 0, w0 = gen; break;
            case 4: {
                const unsigned long long id = (unsigned long long)in.id_base + i;
                y = l.o_cid, len = 8 + l.ntok, w0 = (uint32_t)id, w1 = (uint32_t)(id >> 32), w2 = 0x03030303u;   // True tokens
                break;
            }
            case 5: y = l.o_ngt, len = ngt ? 4 : 0, w0 = ngt; break;
            case 6: y = l.o_sa, len = 28, w0 = 0xFFFFFFFFu; break;                  // null KeyExt: int32 -1
            case 7: y = l.o_sa + 28, len = 28, w0 = (uint32_t)sext; break;
            case 8: y = l.o_ss, len = 24; break;
            case 9: y = l.o_ta, len = addressed ? 28 : 0, w0 = 0xFFFFFFFFu; break;
            case 10: y = l.o_tg, len = 28, w0 = (uint32_t)text; break;
            case 11: y = l.o_ts, len = addressed ? 24 : 0; break;
            default: break;
        }
        if (!inside(y, len)) len = 0;
        const uint32_t* src = nullptr;
        if (len && field >= 6) {
            const uint64_t* s8 = field == 6    ? t.e.act_ids + 3ull * in.sender_act[i]
                                 : field == 7  ? in.sender + 3ull * i
                                 : field == 9  ? t.e.act_ids + 3ull * in.act[i]
                                 : field == 10 ? in.target + 3ull * i
                                               : nullptr;
            src = s8 ? reinterpret_cast<const uint32_t*>(s8)
                     : t.e.silo_wire + 6ull * (field == 8 ? t.my_silo : in.silo[i]);
        }
        if (len) {
            uint32_t w[7] = {w0, w1, w2, w3, 0, 0, 0};
            if (src) {
#pragma unroll
                for (uint32_t k = 0; k < 6; ++k) w[k] = src[k];
                w[6] = w0;
            }
#pragma unroll
            for (uint32_t k = 0; k < 7; ++k)
                if (4 * k < len) req_put(img, rel + y + 4 * k, w[k], len - 4 * k);
        }

        // the strings and the body's ragged ends: the sixteen lanes together
        if (dbg && inside(17, dbg)) req_copy(img, rel + 17, t.str_utf8 + t.str_off[in.debug[i]], dbg, g);
        if (gen && inside(l.o_gen + 4, gen))
            req_copy(img, rel + l.o_gen + 4, t.str_utf8 + t.str_off[in.generic[i]], gen, g);
        if (ngt && inside(l.o_ngt + 4, ngt))
            req_copy(img, rel + l.o_ngt + 4, t.e.type_utf8 + t.e.type_off[in.new_type[i]], ngt, g);
        if (sext > 0 && inside(l.o_sx, (uint32_t)sext))
            req_copy(img, rel + l.o_sx, in.sext + in.sext_off[i], (uint32_t)sext, g);
        if (text > 0 && inside(l.o_tx, (uint32_t)text))
            req_copy(img, rel + l.o_tx, in.text + in.text_off[i], (uint32_t)text, g);
        if (body_len && inside(l.hdr, body_len)) {
            const uint8_t* bsrc = in.body + in.body_off[i];
            const long long pb = rel + l.hdr;                       // the body's first image position
            const long long c0 = pb < 0 ? 0 : pb;                   // ... and its part inside the tile, [c0, c1)
            const long long c1 = pb + (long long)body_len > (long long)REQ_TILE ? (long long)REQ_TILE : pb + (long long)body_len;
            const long long m0 = (c0 + 15) & ~15ll, m1 = c1 & ~15ll;   // whole chunks: [m0, m1)
            if (m1 > m0) {
                for (long long c = m0 / 16 + g; c < m1 / 16; c += REQ_GROUP)
                    s_src[c] = reinterpret_cast<unsigned long long>(bsrc + (16 * c - pb));
                req_copy(img, pb, bsrc, (uint32_t)(m0 - pb), g);                                   // head: [c0, m0)
                req_copy(img, m1, bsrc + (m1 - pb), (uint32_t)(c1 - m1), g);                       // tail: [m1, c1)
            } else {
                req_copy(img, pb, bsrc, body_len, g);
            }
        }
    }
    __syncthreads();

    // ---- phase 2: one chunk a lane and step
    for (uint32_t it = 0; it < ENC_TILE_CHUNKS / BLOCK; ++it) {
        const uint32_t c = it * BLOCK + threadIdx.x;
        const uint64_t c0 = t0 + 16ull * c;                                    // lead-shifted start of the chunk
        if (c0 >= (uint64_t)total + lead) break;
        const uint32_t x0 = (uint32_t)(c0 > lead ? c0 - lead : 0);
        const uint64_t c1 = c0 + 16 - lead;
        const uint32_t x1 = (uint32_t)(c1 < total ? c1 : total);              // the chunk's positions [x0, x1)
        uint4 v;
        const unsigned long long sp = s_src[c];
        if (sp) {
            // sixteen body bytes at any alignment
            const uint8_t* s = reinterpret_cast<const uint8_t*>(sp);
            const uint32_t sh = (uint32_t)(sp & 3u);
            const EncU4 q = *reinterpret_cast<const EncU4*>(s - sh);
            if (sh) {
                const uint32_t e = *reinterpret_cast<const uint32_t*>(s - sh + 16);
                v.x = __builtin_amdgcn_alignbyte(q.y, q.x, sh);
                v.y = __builtin_amdgcn_alignbyte(q.z, q.y, sh);
                v.z = __builtin_amdgcn_alignbyte(q.w, q.z, sh);
                v.w = __builtin_amdgcn_alignbyte(e, q.w, sh);
            } else {
                v = make_uint4(q.x, q.y, q.z, q.w);
            }
        } else {
            v = s_img[c];
        }
        if (x1 - x0 == 16) {
            *reinterpret_cast<uint4*>(out + x0) = v;                           // out + x0 is 16-B aligned
        } else {
            const uint32_t k0 = (uint32_t)((long long)x0 - base) - 16 * c;     // the chunk's first byte that is output
            for (uint32_t k = k0; k < k0 + (x1 - x0); ++k) {
                const uint32_t w = k < 4 ? v.x : k < 8 ? v.y : k < 12 ? v.z : v.w;
                out[x0 + k - k0] = (uint8_t)(w >> (8 * (k & 3)));
            }
        }
    }
}

}  // namespace gd
