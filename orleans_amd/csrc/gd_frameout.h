// gd_frameout.h -- what the stages that write frames into one contiguous output share (the frame encoder,
// gd_encode.h; the request writer, gd_request.h; the response, forward and rejection writers, gd_respond.h,
// gd_forward.h, gd_reject.h): the output offsets of a batch in a given order, the capacity check, the constants and
// the search of the tiled writers, and k_run_write, the one writer of the stages whose output frame is a fixed
// number of byte runs laid end to end.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gd_common.h"

namespace gd {

constexpr uint32_t ERR_ENC_FULL = 128u;      // DevCounters::err: the encoded total exceeds out_cap

// lens[j] = out_len[order[j]] for j < n, lens[n] = 0 (the exclusive scan leaves the total there).  An order entry
// that is no index of the batch is clamped: `order` is required to be a permutation.
static __global__ __launch_bounds__(BLOCK) void k_enc_lens(const uint32_t* __restrict__ out_len,
                                                    const uint32_t* __restrict__ order, uint32_t n,
                                                    uint32_t* __restrict__ lens) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j > n) return;
    lens[j] = j < n ? out_len[order ? min(order[j], n - 1) : j] : 0u;
}

static __global__ __launch_bounds__(BLOCK) void k_enc_finish(const uint32_t* __restrict__ offs, uint32_t n,
                                                      uint64_t out_cap, unsigned long long* __restrict__ out_off,
                                                      uint32_t* __restrict__ err) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j > n) return;
    out_off[j] = offs[j];
    if (j == n && (uint64_t)offs[n] > out_cap) atomicOr(err, ERR_ENC_FULL);
}

constexpr uint32_t ENC_TILE_CHUNKS = 1024;              // 16-B chunks a workgroup: a 16-KiB tile of the output
constexpr uint32_t ENC_TILE_FRAMES = 1024;              // frame offsets kept in LDS (4 KiB + 4); more: global search

struct __attribute__((packed, aligned(4))) EncU4 {
    uint32_t x, y, z, w;
};

// The last j in [lo, hi] with so[j - base] <= pos (so is non-decreasing and so[lo - base] <= pos).
__device__ __forceinline__ uint32_t enc_find(const uint32_t* so, uint32_t base, uint32_t lo, uint32_t hi, uint32_t pos) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (so[mid - base] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ------------------------------------------------------------------ k_run_write
// One output frame as k_run_write sees it: run k holds the output positions [st[k], st[k + 1]) (st[SEGS] = the
// frame's end) and output position x of it is the byte at address a_k + x, a_k = d[0] + ... + d[k].  (Differences,
// summed under the comparisons: a table of the a_k themselves would be indexed by run and so leave the registers.)
template <uint32_t SEGS>
struct RunFrame {
    uint32_t st[SEGS];
    uint64_t d[SEGS];
};

// Lays a frame's runs end to end: with uint32_t cur = the frame's first output position and uint64_t prev = 0,
// RUN_SEG(f, cur, prev, k, from, len) for k = 0 .. SEGS - 1 in order makes run k of RunFrame f the `len` bytes at
// address `from`.  (A macro: as an inlined function the same statements cost the writers ten or more VGPRs.)
#define RUN_SEG(f, cur, prev, k, from, len) \
    f.st[k] = cur;                          \
    f.d[k] = ((from) - cur) - prev;         \
    prev = (from) - cur;                    \
    cur += (len)

// The address of the byte at output position x, and *same = [x, x + span] lies in one run.
template <uint32_t SEGS>
__device__ __forceinline__ uint64_t run_addr(const RunFrame<SEGS>& f, uint32_t x, uint32_t span, bool* same) {
    uint64_t a = f.d[0];
    uint32_t c0 = 0, c1 = 0;
#pragma unroll
    for (uint32_t k = 1; k < SEGS; ++k) {
        const bool in = x >= f.st[k];
        a += in ? f.d[k] : 0ull;
        c0 += in ? 1u : 0u;
        c1 += (x + span >= f.st[k]) ? 1u : 0u;
    }
    *same = c0 == c1;
    return a + x;
}

__device__ __forceinline__ void run_put(uint4& v, uint32_t w, uint32_t val) {
    v.x = w == 0 ? val : v.x;
    v.y = w == 1 ? val : v.y;
    v.z = w == 2 ? val : v.z;
    v.w = w == 3 ? val : v.w;
}

// The writer of every stage whose output frame is A::SEGS byte runs laid end to end.  The argument struct A holds
// n, offs (n + 1 scanned offsets in output order), out_cap and the member frame(j, fo, f): the runs of output frame
// j, whose first output position is fo, from the stage's plan record.  The output is cut as k_enc_write cuts it:
// 16-KiB tiles of 16-B chunks at absolute 16-B addresses, one chunk a lane and step, one owner a chunk.  A lane
// resolves its chunk against its frame's run starts (registers): a chunk inside one run (a body, a long string) is
// one 16-B load (dword aligned + alignbyte); else dword by dword, a dword inside one run being two aligned loads
// and an alignbyte, and only a dword that straddles a run edge or a frame boundary is put together from bytes.  The
// chunk leaves as one aligned 16-B store; only the first and last chunk of the whole output use byte stores.
template <class A>
static __global__ __launch_bounds__(BLOCK) void k_run_write(A a, uint8_t* __restrict__ out) {
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
        const bool whole = x1 - x0 == 16;                                      // then out + x0 is 16-B aligned
        uint32_t j = jlo, fend = 0;                                            // the frame at hand ends at fend
        RunFrame<A::SEGS> f;
        uint4 v = make_uint4(0, 0, 0, 0);
        uint32_t x = x0;
        while (x < x1) {
            if (x >= fend) {                                                   // zero-length frames are stepped over
                j = enc_find(so, jlo, j, jhi, x);
                fend = so[j + 1 - jlo];
                a.frame(j, so[j - jlo], f);
            }
            const uint32_t k = x - x0, room = min(x1, fend) - x;
            bool same = false;
            if (whole && k == 0 && room == 16) {
                const uint64_t s = run_addr(f, x, 15, &same);
                if (same) {                                                    // one run: 16 source bytes at any alignment
                    const uint32_t sh = (uint32_t)(s & 3u);
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
                    x += 16;
                    continue;
                }
            }
            if (whole && (k & 3u) == 0 && room >= 4) {
                const uint64_t s = run_addr(f, x, 3, &same);
                if (same) {                                                    // a dword inside one run
                    const uint32_t sh = (uint32_t)(s & 3u);
                    const uint32_t* p = reinterpret_cast<const uint32_t*>(s - sh);
                    uint32_t d = p[0];
                    if (sh) d = __builtin_amdgcn_alignbyte(p[1], d, sh);
                    run_put(v, k >> 2, d);
                    x += 4;
                    continue;
                }
            }
            const uint32_t b = *reinterpret_cast<const uint8_t*>(run_addr(f, x, 0, &same));
            if (whole) {
                const uint32_t wd = k >> 2, old = wd == 0 ? v.x : wd == 1 ? v.y : wd == 2 ? v.z : v.w;
                run_put(v, wd, old | (b << (8 * (k & 3u))));
            } else {
                out[x] = (uint8_t)b;                                           // the first or last chunk of the output
            }
            x += 1;
        }
        if (whole) *reinterpret_cast<uint4*>(out + x0) = v;
    }
}

}  // namespace gd
