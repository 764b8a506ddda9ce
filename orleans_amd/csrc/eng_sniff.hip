// eng_sniff.hip -- libgraindispatch: the sniff stage: InsideRuntimeClient.SniffIncomingMessage for a
// received batch -- the entries of the frames' CacheInvalidationHeaders (gd_sniff_frames*), InvalidateCacheEntry for
// a batch of (grain, ActivationId) on the non-owner cache (gd_cache_invalidate*), and the chain of the two
// (gd_sniff_invalidate*).  Kernels: gd_sniff.h.  Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_sniff.h"

namespace {

int check_sniff_args(gd_handle* h, const void* buf, uint64_t buf_len, const void* frame_off, uint32_t n,
                     const gd_sniff_out* o) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (!o || !o->count || !o->ent_off || !o->status) return set_err(h, GD_EINVAL, "null argument");
    if (n && (!buf || !frame_off)) return set_err(h, GD_EINVAL, "null argument");
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "sniff frames: n > 2^31");
    // an entry holds at least 80 B and the frames are disjoint ranges of buf: m <= buf_len / 80
    if (buf_len / 80 >= (1ull << 32)) return set_err(h, GD_EINVAL, "sniff frames: buf_len / 80 reaches 2^32");
    return GD_OK;
}

SniffOut sniff_out(const gd_sniff_out* o) {
    return SniffOut{o->count,     o->ent_off,           o->status,      o->flags,      o->ent_frame,
                    o->ent_silo,  (uint64_t*)o->ent_grain, o->ent_ext_off, o->ent_ext_len, (uint64_t*)o->ent_act_id};
}

// The stage on device arrays; enqueue only.
int sniff_device(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                 const SniffOut& o, uint32_t ent_cap) {
    if (n == 0) {
        HIP_TRY(h, hipMemsetAsync(o.ent_off, 0, sizeof(uint32_t), h->stream));
        return GD_OK;
    }
    StageTime stage(h, "stage:sniff");
    const dim3 grid(blocks_for(n, SNIFF_BLOCK));
    GD_TRY(launch(h, "k_sniff_count", grid, dim3(SNIFF_BLOCK), 0, k_sniff_count, buf, buf_len, frame_off, n, o));
    GD_TRY(scan_device<OpAdd>(h, o.ent_off, n + 1, false, false, "sniff"));
    return launch(h, "k_sniff_extract", grid, dim3(SNIFF_BLOCK), 0, k_sniff_extract, buf, buf_len, frame_off, n, o,
                  ent_cap, &h->ctr->err);
}

// InvalidateCacheEntry(keys[k], act_ids[k]) for k = 0 .. live - 1 in order, on device arrays; enqueue only.
int invalidate_device(gd_handle* h, const gd_key* keys, const ExtArgs& x, const gd_key* act_ids, uint32_t m,
                      const uint32_t* d_m, uint8_t* out) {
    if (m == 0) return GD_OK;
    StageTime stage(h, "stage:cache_invalidate");
    if (h->ccap > (1ull << 32)) return set_err(h, GD_EINVAL, "cache table too large to invalidate in");
    DevBuf* S = h->inv_scr;
    if (h->inv_cap != h->ccap || !S[0].p) {                  // a new table, or a call that ended early: all none
        GD_TRY(ensure(h, S[0], (size_t)h->ccap * 4));
        HIP_TRY(h, hipMemsetAsync(S[0].p, 0xFF, (size_t)h->ccap * 4, h->stream));
    }
    h->inv_cap = 0;
    GD_TRY(ensure(h, S[1], (size_t)m * 4));
    GD_TRY(ensure(h, S[2], (size_t)m));
    GD_TRY(ensure(h, h->cbuf[0], (size_t)m * 4));
    GD_TRY(ensure(h, h->cbuf[1], (size_t)m * 4));
    uint32_t* first = (uint32_t*)S[0].p;
    uint32_t* slot_of = (uint32_t*)S[1].p;
    uint8_t* cls = (uint8_t*)S[2].p;
    uint32_t* hit = (uint32_t*)h->cbuf[0].p;
    uint32_t* cslot = (uint32_t*)h->cbuf[1].p;
    const InvArgs a{keys, x, act_ids, m, d_m, (const uint64_t*)h->act_ids.p, h->n_act_ids};
    const dim3 grid(blocks_for(m, BLOCK));
    GD_TRY(launch(h, "k_inv_find", grid, dim3(BLOCK), 0, k_inv_find, a, cache_args(h), first, slot_of, cls, h->cctr));
    GD_TRY(launch(h, "k_inv_resolve", grid, dim3(BLOCK), 0, k_inv_resolve, m, d_m, (const uint32_t*)slot_of,
                  (const uint8_t*)cls, (const uint32_t*)first, hit, cslot, out));
    GD_TRY(cache_touch(h, hit, cslot, m));
    GD_TRY(launch(h, "k_inv_apply", grid, dim3(BLOCK), 0, k_inv_apply, m, d_m, (const uint32_t*)slot_of,
                  (const uint8_t*)cls, first, h->cslots, h->cctr));
    h->inv_cap = h->ccap;
    return GD_OK;
}

int check_chain_args(gd_handle* h, const gd_sniff_out* o, uint32_t ent_cap, const void* inv) {
    if (ent_cap && (!o->ent_grain || !o->ent_ext_off || !o->ent_ext_len || !o->ent_act_id || !inv))
        return set_err(h, GD_EINVAL, "sniff + invalidate: ent_grain, ent_ext_off, ent_ext_len, ent_act_id and inv are required");
    return GD_OK;
}

// The entry arrays of a host-pointer call: held on the device, the first m entries brought down once m is known.
struct SniffHold {
    gd_sniff_out dev{};
    void stage(HostStage& io, const gd_sniff_out* want, uint32_t n, uint32_t cap) {
        dev.count = io.out(want->count, n, 4);
        dev.ent_off = io.out(want->ent_off, (size_t)n + 1, 16);
        dev.status = io.out(want->status, n, 4);
        dev.flags = io.out_if(want->flags, n, 4);
        dev.ent_frame = io.hold<uint32_t>(cap, 0, want->ent_frame != nullptr);
        dev.ent_silo = io.hold<uint32_t>((size_t)cap * 6, 0, want->ent_silo != nullptr);
        dev.ent_grain = io.hold<gd_key>(cap, 0, want->ent_grain != nullptr);
        dev.ent_ext_off = io.hold<uint64_t>(cap, 0, want->ent_ext_off != nullptr);
        dev.ent_ext_len = io.hold<int32_t>(cap, 0, want->ent_ext_len != nullptr);
        dev.ent_act_id = io.hold<gd_key>(cap, 0, want->ent_act_id != nullptr);
    }
    int fetch(HostStage& io, const gd_sniff_out* want, uint32_t m) {
        GD_TRY(io.fetch(want->ent_frame, dev.ent_frame, m));
        GD_TRY(io.fetch(want->ent_silo, dev.ent_silo, (size_t)m * 6));
        GD_TRY(io.fetch(want->ent_grain, dev.ent_grain, m));
        GD_TRY(io.fetch(want->ent_ext_off, dev.ent_ext_off, m));
        GD_TRY(io.fetch(want->ent_ext_len, dev.ent_ext_len, m));
        return io.fetch(want->ent_act_id, dev.ent_act_id, m);
    }
};

}  // namespace

extern "C" {

int gd_sniff_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                           uint32_t n, const gd_sniff_out* d_out, uint32_t ent_cap) {
    GD_TRY(check_sniff_args(h, d_buf, buf_len, d_frame_off, n, d_out));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_sniff_frames_device"));
    return sniff_device(h, d_buf, buf_len, d_frame_off, n, sniff_out(d_out), ent_cap);
}

int gd_sniff_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                    const gd_sniff_out* out, uint32_t ent_cap, uint32_t* out_m) {
    GD_TRY(check_sniff_args(h, buf, buf_len, frame_off, n, out));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_sniff_frames"));
    if (out_m) *out_m = 0;
    if (n == 0) {
        out->ent_off[0] = 0;
        return GD_OK;
    }
    HostStage io(h);
    const uint8_t* dbuf = io.in(buf, (size_t)buf_len);
    const uint64_t* dfoff = io.in(frame_off, n);
    SniffHold s;
    s.stage(io, out, n, ent_cap);
    GD_TRY(io.status());
    GD_TRY(sniff_device(h, dbuf, buf_len, dfoff, n, sniff_out(&s.dev), ent_cap));
    GD_TRY(io.fetch());
    GD_TRY(sync(h));
    const uint32_t m = out->ent_off[n];
    if (out_m) *out_m = m;
    if (m <= ent_cap) GD_TRY(s.fetch(io, out, m));
    return sync_checked(h);                                  // m past ent_cap: ERR_SNIFF_FULL -> GD_EFULL
}

int gd_cache_invalidate_device(gd_handle* h, const gd_key* d_keys, const gd_key_ext* d_ext, const gd_key* d_act_ids,
                               uint32_t m, const uint32_t* d_m, uint8_t* d_out) {
    GD_TRY(cache_check(h));
    if (m && (!d_keys || !d_act_ids || !d_out || !ext_ok(d_ext, m))) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_cache_invalidate_device"));
    ExtArgs x{};
    if (d_ext) x = ExtArgs{d_ext->bytes, d_ext->offset, d_ext->length, d_ext->bytes_len};
    return invalidate_device(h, d_keys, x, d_act_ids, m, d_m, d_out);
}

int gd_cache_invalidate(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, const gd_key* act_ids, uint32_t m,
                        uint8_t* out) {
    GD_TRY(cache_check(h));
    if (m && (!keys || !act_ids || !out || !ext_ok(ext, m))) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_cache_invalidate"));
    if (m == 0) return GD_OK;
    if (ext) {                                               // as gd_cache_remove_ext: every KeyExt item is matchable
        for (uint32_t i = 0; i < m; ++i) {
            if (!is_keyext_cat(keys[i].type_code_data)) continue;
            const uint8_t* s;
            int32_t len;
            GD_TRY(host_ext(h, ext, i, s, len));
        }
    }
    HostStage io(h);
    const gd_key* dk = io.in(keys, m);
    const gd_key* dids = io.in(act_ids, m);
    const uint8_t* dxb = io.in(ext && ext->bytes_len ? ext->bytes : nullptr, ext ? (size_t)ext->bytes_len : 0);
    const uint64_t* dxo = io.in(ext ? ext->offset : nullptr, m);
    const int32_t* dxl = io.in(ext ? ext->length : nullptr, m);
    uint8_t* dout = io.out(out, m, 4);
    GD_TRY(io.status());
    ExtArgs x{};
    if (ext) x = ExtArgs{dxb, dxo, dxl, ext->bytes_len};
    GD_TRY(invalidate_device(h, dk, x, dids, m, nullptr, dout));
    GD_TRY(io.fetch());
    return sync(h);
}

int gd_sniff_invalidate_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                               uint32_t n, const gd_sniff_out* d_out, uint32_t ent_cap, uint8_t* d_inv) {
    GD_TRY(cache_check(h));
    GD_TRY(check_sniff_args(h, d_buf, buf_len, d_frame_off, n, d_out));
    GD_TRY(check_chain_args(h, d_out, ent_cap, d_inv));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_sniff_invalidate_device"));
    const SniffOut o = sniff_out(d_out);
    GD_TRY(sniff_device(h, d_buf, buf_len, d_frame_off, n, o, ent_cap));
    const ExtArgs x{d_buf, o.ent_ext_off, o.ent_ext_len, buf_len};
    return invalidate_device(h, d_out->ent_grain, x, d_out->ent_act_id, ent_cap, o.ent_off + n, d_inv);
}

int gd_sniff_invalidate(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                        const gd_sniff_out* out, uint32_t ent_cap, uint8_t* inv, uint32_t* out_m) {
    GD_TRY(cache_check(h));
    GD_TRY(check_sniff_args(h, buf, buf_len, frame_off, n, out));
    GD_TRY(check_chain_args(h, out, ent_cap, inv));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_sniff_invalidate"));
    if (out_m) *out_m = 0;
    if (n == 0) {
        out->ent_off[0] = 0;
        return GD_OK;
    }
    HostStage io(h);
    const uint8_t* dbuf = io.in(buf, (size_t)buf_len);
    const uint64_t* dfoff = io.in(frame_off, n);
    SniffHold s;
    s.stage(io, out, n, ent_cap);
    uint8_t* dinv = io.hold<uint8_t>(ent_cap, 4, inv != nullptr);
    GD_TRY(io.status());
    const SniffOut o = sniff_out(&s.dev);
    GD_TRY(sniff_device(h, dbuf, buf_len, dfoff, n, o, ent_cap));
    const ExtArgs x{dbuf, o.ent_ext_off, o.ent_ext_len, buf_len};
    GD_TRY(invalidate_device(h, s.dev.ent_grain, x, s.dev.ent_act_id, ent_cap, o.ent_off + n, dinv));
    GD_TRY(io.fetch());
    GD_TRY(sync(h));
    const uint32_t m = out->ent_off[n];
    if (out_m) *out_m = m;
    if (m <= ent_cap) {
        GD_TRY(s.fetch(io, out, m));
        GD_TRY(io.fetch(inv, dinv, m));
    }
    return sync_checked(h);
}

}  // extern "C"
