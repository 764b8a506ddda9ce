// gd_encode.h -- gfx950 device code for the frame encoder: batched Message.SetTargetPlacement
// (Message.cs:629-639, from Dispatcher.cs:753-767) + Message.Serialize (Message.cs:481-516, HeadersContainer.
// Serializer :1126-1245) on the frames of a routed batch, the counterpart of k_decode_frames (gd_frames.h).
//
// Per frame (rule and statuses: include/graindispatch.h, tests/_encode_ref.py): TargetActivation (28 B UniqueKey
// from the handle's act_ids), TargetSilo (24 B wire SiloAddress), IsNewPlacement (True token) and NewGrainType
// (int32 length + UTF-8) are inserted at -- or replace what stands at -- their Serializer positions, the mask and
// headerLength are rewritten, every other byte is copied in order.
//
//   k_enc_plan    one lane per frame: the decoder's staging and walk (192-B LDS window, alignbyte reads, global
//                 fallback past it), extended to the four insertion points; writes one 32-B EncPlan a frame,
//                 its output length and its status
//   k_enc_lens    lens[j] = out_len[order[j]] (+ the scan's closing 0); scan_device turns it into offsets
//   k_enc_finish  out_off[j] as u64; the capacity check against the scanned total (ERR_ENC_FULL)
//                 (both in gd_frameout.h, shared with the response writer)
//   k_enc_write   the hot path.  The OUTPUT is cut into 16-KiB tiles of 16-B chunks at absolute 16-B addresses,
//                 one workgroup a tile, one chunk a lane and step, whatever the frame lengths: a 300-KB body
//                 and a run of 60-B frames load the lanes alike, zero-length frames cost nothing, and a chunk
//                 has one owner, so no byte outside [0, total) is touched and no two lanes share a store.  The
//                 workgroup finds the frames its tile cuts by binary search of the scanned offsets and keeps
//                 their offsets in LDS; a lane finds its chunk's frame there, maps the chunk back through the
//                 frame's plan and, when it lies in one copied run of one frame, moves it with one 16-B load
//                 (dword aligned + alignbyte) and one aligned 16-B store.  Chunks that meet an inserted field,
//                 the 12-B prefix or a frame boundary are resolved byte by byte (source byte, table byte or
//                 constant) and still leave as one 16-B store; only the first and last chunk of the whole
//                 output use byte stores.
//
// Totals are 32-bit: the host refuses (GD_EINVAL) a call whose bound buf_len + n * (57 + longest type string)
// reaches 2^32, so gd_scan.h's scan serves.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_frames.h"
#include "gd_frameout.h"
#include "gd_hash.h"

namespace gd {

// GD_ENC_* (include/graindispatch.h)
enum : uint32_t { ENC_OK = 0, ENC_COPIED = 1, ENC_SKIPPED = 2, ENC_FALLBACK = 3, ENC_MALFORMED = 4, ENC_NO_ID = 5,
                  ENC_NO_SILO = 6 };
constexpr uint32_t H_TRANSACTION_INFO = 1u << 27;
constexpr uint32_t ENC_TA_LEN = 28, ENC_TS_LEN = 24;
constexpr uint32_t ENC_MAX_TYPE = 0xFFF0u;   // longest class-name string (the plan keeps 4 + length in 16 bits)
constexpr uint32_t ENC_PLACED_NEW = 1;       // GD_PLACED_NEW

// One frame's plan, 32 B (two 16-B loads in k_enc_write).  Positions are bytes from the frame start in the
// SOURCE; r* = bytes of the source the new field replaces, n* = bytes written.
//   flags: bit 0 rINP (an IsNewPlacement token stands at p_inp), bit 1 nINP (a True token is written there),
//          bit 2 rTS (a 24-B TargetSilo stands at p_ts)
// NewGrainType's position needs no word: p_inp + the source's IsNewPlacement / ReadOnly / IsUnordered tokens
// (mask bits; enc_map).
// COPIED frames keep src_len and zeros; every other status has src_len 0.
struct EncPlan {
    uint32_t mask;       // the new mask
    uint32_t src_len;    // 8 + headerLength + bodyLength
    uint32_t p_inp, p_ta, p_ts;
    uint32_t r_ngt, r_ta;
    uint32_t tail;       // status | flags << 8 | nNGT << 16
};
static_assert(sizeof(EncPlan) == 32, "plan record is 32 B");

struct EncTab {
    const uint64_t* act_ids;      // 3 x u64 per activation index (gd_activation_ids_set); all zero: none
    uint64_t n_act_ids;
    const uint32_t* silo_wire;    // 6 x u32 per silo index: ip[16], port, generation
    uint32_t n_silos;
    const uint8_t* type_utf8;
    const uint32_t* type_off;     // n_types + 1
    uint32_t n_types;
};

// Activation index a has an ActivationId.
__device__ __forceinline__ bool enc_has_id(const EncTab& t, uint32_t a) {
    if ((uint64_t)a >= t.n_act_ids) return false;
    const uint64_t* id = t.act_ids + 3ull * a;
    return (id[0] | id[1] | id[2]) != 0;
}

// The plan in output coordinates: the starts of the four new fields, their lengths and the source shift behind each.
struct EncMap {
    uint32_t o_inp, o_ngt, o_ta, o_ts;
    uint32_t n_inp, n_ngt, n_ta, n_ts;
    int32_t d1, d2, d3, d4;
    uint32_t out_len;
    bool raw;            // COPIED: output byte x = source byte x
};

__device__ __forceinline__ EncMap enc_map(const EncPlan& p) {
    EncMap m;
    const uint32_t st = p.tail & 0xFFu, fl = (p.tail >> 8) & 0xFFu;
    m.raw = st != ENC_OK;
    const uint32_t r_inp = fl & 1u, r_ts = (fl & 4u) ? ENC_TS_LEN : 0u;
    m.n_inp = (fl >> 1) & 1u;
    m.n_ngt = p.tail >> 16;
    m.n_ta = m.raw ? 0u : ENC_TA_LEN;
    m.n_ts = m.raw ? 0u : ENC_TS_LEN;
    // the source's tokens from p_inp on: its own IsNewPlacement (the bit is set and it was not inserted here),
    // ReadOnly, IsUnordered
    const uint32_t own_inp = (p.mask & H_IS_NEW_PLACEMENT) && !(m.n_inp && !r_inp) ? 1u : 0u;
    const uint32_t p_ngt = p.p_inp + own_inp + __popc(p.mask & (H_READ_ONLY | H_IS_UNORDERED));
    m.d1 = (int32_t)m.n_inp - (int32_t)r_inp;
    m.d2 = m.d1 + (int32_t)m.n_ngt - (int32_t)p.r_ngt;
    m.d3 = m.d2 + (int32_t)m.n_ta - (int32_t)(m.raw ? 0u : p.r_ta);
    m.d4 = m.d3 + (int32_t)m.n_ts - (int32_t)(m.raw ? 0u : r_ts);
    m.o_inp = p.p_inp;
    m.o_ngt = p_ngt + m.d1;
    m.o_ta = p.p_ta + m.d2;
    m.o_ts = p.p_ts + m.d3;
    m.out_len = p.src_len + m.d4;
    return m;
}

// ------------------------------------------------------------------ k_enc_plan
// WALK (GD_OPT_WALK_INVALIDATION): a CacheInvalidationHeader is stepped over, so the four positions lie behind
// it and k_enc_write copies it through in front of Category; without it such a frame is ENC_FALLBACK.
template <bool WALK = false>
static __global__ __launch_bounds__(BLOCK) void k_enc_plan(const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                    const uint64_t* __restrict__ frame_off, uint32_t n,
                                                    const uint32_t* __restrict__ silo,
                                                    const uint32_t* __restrict__ act,
                                                    const uint8_t* __restrict__ route_status,
                                                    const uint8_t* __restrict__ placed,
                                                    const uint32_t* __restrict__ new_type, EncTab t,
                                                    EncPlan* __restrict__ plan, uint32_t* __restrict__ out_len,
                                                    uint8_t* __restrict__ enc_status) {
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

    EncPlan p{0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t st = ENC_SKIPPED, olen = 0;
    const uint32_t rs = route_status[i];
    if (rs == 0 /* GD_ROUTE_OK */ || rs == ROUTE_ADDRESSED) {
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
            st = ENC_MALFORMED;
        } else if (rs == ROUTE_ADDRESSED) {
            st = ENC_COPIED;
            p.src_len = 8u + (uint32_t)hl + (uint32_t)bl;
            olen = p.src_len;
        } else {
            hw.p = 12;
            hw.end = 8u + (uint32_t)hl;
            const uint32_t m = hw.c.u32(8);
            if ((m & ((WALK ? 0u : H_CACHE_INVALIDATION) | H_REQUEST_CONTEXT)) ||
                ((m & H_TARGET_OBSERVER) && (m & H_TRANSACTION_INFO))) {
                st = ENC_FALLBACK;
            } else {
                // HeadersContainer.Serializer order (Message.cs:1126-1245)
                if (WALK && (m & H_CACHE_INVALIDATION)) hw.skip_invalidation();
                if (m & H_CATEGORY) hw.take(1);
                if (m & H_DEBUG_CONTEXT) hw.skip_string();
                if ((m & H_DIRECTION) && !hw.bad) hw.take(1);
                if (m & H_TIME_TO_LIVE) hw.take(8);
                if (m & H_FORWARD_COUNT) hw.take(4);
                if (m & H_GENERIC_GRAIN_TYPE) hw.skip_string();
                if ((m & H_CORRELATION_ID) && !hw.bad) hw.take(8);
                if ((m & H_ALWAYS_INTERLEAVE) && !hw.bad) hw.take(1);
                const uint32_t p_inp = hw.p;
                const uint32_t r_inp = (m & H_IS_NEW_PLACEMENT) ? 1u : 0u;
                const uint32_t nb = r_inp + __popc(m & (H_READ_ONLY | H_IS_UNORDERED));
                if (nb && !hw.bad) hw.take(nb);
                const uint32_t p_ngt = hw.p;
                if (m & H_NEW_GRAIN_TYPE) hw.skip_string();
                const uint32_t r_ngt = hw.p - p_ngt;
                if (m & H_REJECTION_INFO) hw.skip_string();
                if ((m & H_REJECTION_TYPE) && !hw.bad) hw.take(1);
                if ((m & H_RESEND_COUNT) && !hw.bad) hw.take(4);
                if ((m & H_RESULT) && !hw.bad) hw.take(1);
                if (m & H_SENDING_ACTIVATION) hw.key(nullptr);
                if (m & H_SENDING_GRAIN) hw.key(nullptr);
                if ((m & H_SENDING_SILO) && !hw.bad) hw.take(24);
                const uint32_t p_ta = hw.p;
                if (m & H_TARGET_ACTIVATION) hw.key(nullptr);
                const uint32_t r_ta = hw.p - p_ta;
                if (m & H_TARGET_GRAIN) hw.key(nullptr);
                const uint32_t r_ts = (m & H_TARGET_SILO) ? ENC_TS_LEN : 0u;
                uint32_t p_ts = hw.p;
                if (m & H_TARGET_OBSERVER) {
                    // the object-serialized TargetObserver runs to TargetSilo (no TransactionInfo here): the
                    // silo is the header's last field
                    if (!hw.bad && hw.end - hw.p < r_ts) hw.bad = true;
                    p_ts = hw.end - r_ts;
                } else if (r_ts && !hw.bad) {
                    hw.take(ENC_TS_LEN);
                }
                const uint32_t a = act[i], s = silo[i];
                const bool has_id = enc_has_id(t, a);
                if (hw.bad) {
                    st = ENC_MALFORMED;
                } else if (s >= t.n_silos) {
                    st = ENC_NO_SILO;
                } else if (!has_id) {
                    st = ENC_NO_ID;
                } else {
                    st = ENC_OK;
                    const bool is_new = placed && placed[i] == ENC_PLACED_NEW;
                    uint32_t n_ngt = 0;
                    const uint32_t ty = new_type ? new_type[i] : NONE32;
                    if (ty < t.n_types) {
                        const uint32_t ln = t.type_off[ty + 1] - t.type_off[ty];
                        if (ln) n_ngt = 4 + ln;                     // String.IsNullOrEmpty: unchanged
                    }
                    p.mask = m | H_TARGET_ACTIVATION | H_TARGET_SILO | (is_new ? H_IS_NEW_PLACEMENT : 0u) |
                             (n_ngt ? H_NEW_GRAIN_TYPE : 0u);
                    p.src_len = 8u + (uint32_t)hl + (uint32_t)bl;
                    p.p_inp = p_inp;
                    p.p_ta = p_ta;
                    p.p_ts = p_ts;
                    p.r_ngt = n_ngt ? r_ngt : 0u;                   // no type given: the frame's own field stays
                    p.r_ta = r_ta;
                    const uint32_t fl = (is_new ? (r_inp | 2u) : 0u) | (r_ts ? 4u : 0u);
                    p.tail = ENC_OK | (fl << 8) | (n_ngt << 16);
                    olen = enc_map(p).out_len;
                }
            }
        }
    }
    if (st != ENC_OK) p.tail = st;
    uint4* pp = reinterpret_cast<uint4*>(plan + i);
    pp[0] = make_uint4(p.mask, p.src_len, p.p_inp, p.p_ta);
    pp[1] = make_uint4(p.p_ts, p.r_ngt, p.r_ta, p.tail);
    out_len[i] = olen;
    enc_status[i] = (uint8_t)st;
}

// ------------------------------------------------------------------ k_enc_write
struct EncArgs {
    const uint8_t* buf;
    const uint64_t* frame_off;
    const uint32_t* silo;
    const uint32_t* act;
    const uint32_t* new_type;
    const uint32_t* order;
    const EncPlan* plan;
    const uint32_t* offs;        // n + 1 scanned offsets in output order
    uint32_t n;
    uint64_t out_cap;
};

// One output frame as k_enc_write sees it.
struct EncFrame {
    EncMap m;
    const uint8_t* src;
    uint32_t i;                  // input frame index
    uint32_t mask;
};

__device__ __forceinline__ EncFrame enc_frame(const EncArgs& a, uint32_t j) {
    EncFrame f;
    f.i = a.order ? min(a.order[j], a.n - 1) : j;
    const uint4* pp = reinterpret_cast<const uint4*>(a.plan + f.i);
    const uint4 p0 = pp[0], p1 = pp[1];
    const EncPlan p{p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
    f.m = enc_map(p);
    f.mask = p.mask;
    f.src = a.buf + a.frame_off[f.i];
    return f;
}

// Output byte x of frame f (x < out_len).
__device__ __forceinline__ uint32_t enc_byte(const EncArgs& a, const EncTab& t, const EncFrame& f, uint32_t x) {
    const EncMap& m = f.m;
    if (m.raw) return f.src[x];
    if (x < 12) {
        if (x >= 8) return (f.mask >> (8 * (x - 8))) & 0xFFu;
        if (x >= 4) return f.src[x];
        const uint32_t hl = (uint32_t)f.src[0] | ((uint32_t)f.src[1] << 8) | ((uint32_t)f.src[2] << 16) |
                            ((uint32_t)f.src[3] << 24);
        return ((hl + (uint32_t)m.d4) >> (8 * x)) & 0xFFu;
    }
    if (x < m.o_inp) return f.src[x];
    if (x < m.o_inp + m.n_inp) return 3u;                           // SerializationTokenType.True
    if (x < m.o_ngt) return f.src[(int32_t)x - m.d1];
    if (x < m.o_ngt + m.n_ngt) {
        const uint32_t k = x - m.o_ngt, ty = a.new_type[f.i], o = t.type_off[ty];
        if (k < 4) return ((m.n_ngt - 4) >> (8 * k)) & 0xFFu;
        return t.type_utf8[o + k - 4];
    }
    if (x < m.o_ta) return f.src[(int32_t)x - m.d2];
    if (x < m.o_ta + m.n_ta) {
        const uint32_t k = x - m.o_ta;
        if (k >= 24) return 0xFFu;                                  // null KeyExt: int32 -1
        return reinterpret_cast<const uint8_t*>(t.act_ids + 3ull * a.act[f.i])[k];
    }
    if (x < m.o_ts) return f.src[(int32_t)x - m.d3];
    if (x < m.o_ts + m.n_ts)
        return reinterpret_cast<const uint8_t*>(t.silo_wire + 6ull * a.silo[f.i])[x - m.o_ts];
    return f.src[(int32_t)x - m.d4];
}

// Bytes of [x0, x1) that are written fields (the 12-B prefix included), not copies of the source.
__device__ __forceinline__ uint32_t enc_new_bytes(const EncMap& m, uint32_t x0, uint32_t x1) {
    if (m.raw) return 0;
    auto ov = [&](uint32_t s, uint32_t len) {
        const uint32_t lo = max(x0, s), hi = min(x1, s + len);
        return hi > lo ? hi - lo : 0u;
    };
    return ov(0, 12) + ov(m.o_inp, m.n_inp) + ov(m.o_ngt, m.n_ngt) + ov(m.o_ta, m.n_ta) + ov(m.o_ts, m.n_ts);
}

// The source shift of a copied byte at output position x.
__device__ __forceinline__ int32_t enc_shift(const EncMap& m, uint32_t x) {
    if (m.raw) return 0;
    return x >= m.o_ts ? m.d4 : x >= m.o_ta ? m.d3 : x >= m.o_ngt ? m.d2 : x >= m.o_inp ? m.d1 : 0;
}

static __global__ __launch_bounds__(BLOCK) void k_enc_write(EncArgs a, EncTab t, uint8_t* __restrict__ out) {
    __shared__ uint32_t s_off[ENC_TILE_FRAMES + 1];
    __shared__ uint32_t s_rng[2];
    const uint32_t n = a.n;
    const uint32_t total = a.offs[n];
    if (total == 0 || (uint64_t)total > a.out_cap) return;          // too long: k_enc_finish raised ERR_ENC_FULL
    // chunk c holds output positions [16 c - lead, 16 c - lead + 16): absolute 16-B addresses
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u);
    const uint64_t t0 = (uint64_t)blockIdx.x * ENC_TILE_CHUNKS * 16;          // in lead-shifted coordinates
    if (t0 >= (uint64_t)total + lead) return;
    const uint32_t first = (uint32_t)(t0 > lead ? t0 - lead : 0);              // the tile's first output position
    const uint64_t t1 = t0 + (uint64_t)ENC_TILE_CHUNKS * 16 - lead;
    const uint32_t last = (uint32_t)(t1 < total ? t1 : total) - 1;            // ... and its last
    if (threadIdx.x < 2) s_rng[threadIdx.x] = enc_find(a.offs, 0, 0, n - 1, threadIdx.x ? last : first);
    __syncthreads();
    const uint32_t jlo = s_rng[0], jhi = s_rng[1];
    const bool in_lds = jhi - jlo < ENC_TILE_FRAMES;
    if (in_lds)
        for (uint32_t k = threadIdx.x; k <= jhi - jlo + 1; k += BLOCK) s_off[k] = a.offs[jlo + k];
    __syncthreads();
    const uint32_t* so = in_lds ? s_off : a.offs + jlo;

    for (uint32_t it = 0; it < ENC_TILE_CHUNKS / BLOCK; ++it) {
        const uint64_t c0 = t0 + 16ull * (it * BLOCK + threadIdx.x);          // lead-shifted start of the chunk
        if (c0 >= (uint64_t)total + lead) break;
        const uint32_t x0 = (uint32_t)(c0 > lead ? c0 - lead : 0);
        const uint64_t c1 = c0 + 16 - lead;
        const uint32_t x1 = (uint32_t)(c1 < total ? c1 : total);              // the chunk's positions [x0, x1)
        uint32_t j = enc_find(so, jlo, jlo, jhi, x0);
        EncFrame f = enc_frame(a, j);
        uint32_t fo = so[j - jlo];                                             // the frame's first output position
        uint4 v;
        bool done = false;
        if (x1 - x0 == 16 && x1 <= fo + f.m.out_len && enc_new_bytes(f.m, x0 - fo, x1 - fo) == 0) {
            // one copied run of one frame: 16 source bytes at any alignment
            const uint8_t* s = f.src + (int32_t)((int32_t)(x0 - fo) - enc_shift(f.m, x0 - fo));
            const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3u);
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
            done = true;
        }
        if (!done) {
            uint32_t wv[4] = {0, 0, 0, 0};
            for (uint32_t x = x0; x < x1; ++x) {
                while (so[j + 1 - jlo] <= x) {                                 // zero-length frames are stepped over
                    ++j;
                    fo = so[j - jlo];
                    if (so[j + 1 - jlo] > x) f = enc_frame(a, j);
                }
                const uint32_t b = enc_byte(a, t, f, x - fo);
                const uint32_t k = x - x0;
                wv[k >> 2] |= b << (8 * (k & 3));
            }
            v = make_uint4(wv[0], wv[1], wv[2], wv[3]);
        }
        if (x1 - x0 == 16) {
            *reinterpret_cast<uint4*>(out + x0) = v;                           // out + x0 is 16-B aligned
        } else {
            const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
            for (uint32_t k = 0; k < x1 - x0; ++k) out[x0 + k] = (uint8_t)(wv[k >> 2] >> (8 * (k & 3)));
        }
    }
}

}  // namespace gd
