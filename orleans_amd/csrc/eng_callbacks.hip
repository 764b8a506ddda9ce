// eng_callbacks.hip -- libgraindispatch: the callback table (gd_callbacks.h): SendRequestMessage's
// callbacks.TryAdd, ReceiveResponse -> DoCallback, the response timers and BreakOutstandingMessagesToDeadSilo
// for a batch.  Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_callbacks.h"

namespace {

constexpr unsigned long long CB_MIN_CAP = 64, CB_MAX_CAP = 1ull << 31;

CbTab cb_tab(gd_handle* h) {
    return CbTab{(CbSlot*)h->cb_tab.p, (int64_t*)h->cb_dl.p, h->cb_cap - 1ull, (CbCounters*)h->cb_ctr.p};
}
uint32_t* cb_word(gd_handle* h, uint32_t k) { return (uint32_t*)h->cb_last.p + (size_t)k * h->cb_cap; }

int check_handle(gd_handle* h, const char* call, uint64_t n = 0) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (!h->cb_cap) return set_err(h, GD_ESTATE, "%s before gd_callbacks_configure", call);
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "%s: n > 2^31", call);
    return GD_OK;
}

struct CbCounts {
    uint32_t live, tomb, err;
};

// The counters after a synchronisation (live / tomb summed over their stripes); device error bits are cleared
// and reported once.
int cb_pull(gd_handle* h, CbCounts* c, const char* call) {
    CbCounters full;
    GD_TRY(read_back(h, h->cb_ctr.p, (uint32_t*)&full, sizeof(CbCounters) / 4));
    *c = CbCounts{0, 0, full.err};
    for (uint32_t k = 0; k < CB_STRIPES; ++k) {
        c->live += full.stripe[k][0];
        c->tomb += full.stripe[k][1];
    }
    if (!c->err) return GD_OK;
    GD_TRY(table_err_clear(h, &((CbCounters*)h->cb_ctr.p)->err, c->err, h->cb_last, h->cb_cap));
    if (c->err & CB_ERR_FULL) return set_err(h, GD_EFULL, "%s: the callback table is full (0x%x)", call, c->err);
    if (c->err & CB_ERR_SILO) return set_err(h, GD_EINVAL, "%s: a target silo index above 0xFFFE (0x%x)", call, c->err);
    return set_err(h, GD_ETIMEOUT, "%s: an earlier device batch did not settle (0x%x)", call, c->err);
}

// A zeroed table of `cap` slots with its deadlines and election words.
int cb_alloc(gd_handle* h, unsigned long long cap, DevBuf& tab, DevBuf& dl, DevBuf& last) {
    return table_alloc(h, "callback", cap, sizeof(CbSlot), 8, tab, dl, last);
}

// Rebuild on the stream at `cap` slots: the `live` entries move, the tombstones go.
int cb_rebuild(gd_handle* h, unsigned long long cap, uint32_t live) {
    if (cap > CB_MAX_CAP) return set_err(h, GD_EFULL, "callback table: more than 2^31 slots");
    DevBuf fresh[3];
    GD_TRY(cb_alloc(h, cap, fresh[0], fresh[1], fresh[2]));
    const CbTab old = cb_tab(h);
    const unsigned long long old_cap = h->cb_cap;
    const CbTab nt{(CbSlot*)fresh[0].p, (int64_t*)fresh[1].p, cap - 1ull, old.ctr};
    GD_TRY(launch(h, "k_cb_rebuild", dim3(blocks_for(old_cap, BLOCK)), dim3(BLOCK), 0, k_cb_rebuild,
                  (const CbSlot*)old.slots, (const int64_t*)old.deadline, old_cap, nt));
    // the counts afterwards: `live` entries (the caller's read-back), no tombstone
    HIP_TRY(h, hipMemsetAsync(old.ctr->stripe, 0, sizeof(old.ctr->stripe), h->stream));
    HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)&old.ctr->stripe[0][0], (int)live, 1, h->stream));
    return table_swap(h, {&h->cb_tab, &h->cb_dl, &h->cb_last}, fresh, h->cb_cap, cap);
}

// Room for `incoming` adds (table_reserve).
int cb_reserve(gd_handle* h, uint64_t incoming, const char* call) {
    return table_reserve(
        h, h->cb_used_ub, h->cb_cap, incoming, call,
        [&](uint64_t& live, uint64_t& tomb) {
            CbCounts c;
            GD_TRY(cb_pull(h, &c, call));
            live = c.live;
            tomb = c.tomb;
            return (int)GD_OK;
        },
        [&](unsigned long long cap, uint64_t live) { return cb_rebuild(h, cap, (uint32_t)live); });
}

// ---- the batches on device arrays.  sync_passes: read-back driven passes (the host forms); else gated ones.
int add_device(gd_handle* h, const int64_t* ids, const uint32_t* handles, const int64_t* deadlines, uint32_t n,
               uint8_t* out_added, bool sync_passes, const char* call) {
    if (n == 0) return GD_OK;
    GD_TRY(cb_reserve(h, n, call));
    StageTime stage(h, "stage:cb_add");
    GD_TRY(ensure(h, h->cb_scr[0], (size_t)n * 4));
    GD_TRY(ensure(h, h->cb_scr[1], (size_t)n + 16));
    uint32_t* slot_of = (uint32_t*)h->cb_scr[0].p;
    uint8_t* is_new = (uint8_t*)h->cb_scr[1].p;
    const CbTab t = cb_tab(h);
    uint32_t* last = cb_word(h, 0);
    const dim3 grid(blocks_for(n, BLOCK)), block(BLOCK);
    const uint32_t* unsettled = nullptr;
    GD_TRY(claim_pass_driver(h, t.ctr->retry, CB_PASSES, sync_passes, call, &unsettled,
                             [&](uint32_t p, const uint32_t* gate, uint32_t*) {   // k_cb_claim finds its own word
                                 return launch(h, "k_cb_claim", grid, block, 0, k_cb_claim, ids, n, t, slot_of, is_new, p,
                                               gate, last);
                             }));
    return launch(h, "k_cb_commit", grid, block, 0, k_cb_commit, handles, deadlines, n, t, (const uint32_t*)slot_of,
                  (const uint8_t*)is_new, last, unsettled, out_added);
}

int lookup_device(gd_handle* h, const int64_t* ids, uint32_t n, uint32_t* out_handle, uint32_t* out_resend,
                  uint32_t* out_silo, uint8_t* out_found) {
    return launch(h, "k_cb_find", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_cb_find, ids, n, cb_tab(h),
                  (uint32_t*)nullptr, (uint32_t*)nullptr, out_handle, out_resend, out_silo, out_found);
}

int set_target_device(gd_handle* h, const int64_t* ids, const uint32_t* silo, uint32_t n, uint8_t* out_found) {
    if (n == 0) return GD_OK;
    GD_TRY(ensure(h, h->cb_scr[0], (size_t)n * 4));
    uint32_t* slot_of = (uint32_t*)h->cb_scr[0].p;
    const dim3 grid(blocks_for(n, BLOCK)), block(BLOCK);
    GD_TRY(launch(h, "k_cb_find", grid, block, 0, k_cb_find, ids, n, cb_tab(h), slot_of, cb_word(h, 0),
                  (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, out_found));
    return launch(h, "k_cb_set_target", grid, block, 0, k_cb_set_target, silo, n, cb_tab(h), (const uint32_t*)slot_of,
                  cb_word(h, 0));
}

int respond_device(gd_handle* h, const CbResp& a, uint32_t n, uint32_t* fire_idx, uint32_t* n_fire, bool sync_rounds,
                   const char* call) {
    if (n == 0) {
        if (n_fire) HIP_TRY(h, hipMemsetAsync(n_fire, 0, 4, h->stream));
        return GD_OK;
    }
    StageTime stage(h, "stage:cb_respond");
    GD_TRY(ensure(h, h->cb_scr[0], (size_t)n * 4));
    GD_TRY(ensure(h, h->cb_scr[1], (size_t)n + 16));
    uint32_t* slot_of = (uint32_t*)h->cb_scr[0].p;
    uint8_t* cls = (uint8_t*)h->cb_scr[1].p;
    const CbTab t = cb_tab(h);
    const uint32_t max_resend = h->cb_max_resend;
    const dim3 grid(blocks_for(n, BLOCK)), block(BLOCK);
    HIP_TRY(h, hipMemsetAsync(t.ctr->unres, 0, sizeof(t.ctr->unres), h->stream));
    GD_TRY(launch(h, "k_cb_find_resp", grid, block, 0, k_cb_find_resp, a, n, t, slot_of, cls, cb_word(h, 0)));
    GD_TRY(launch(h, "k_cb_resolve", grid, block, 0, k_cb_resolve, a, n, t, (const uint32_t*)slot_of, cls,
                  cb_word(h, 0), cb_word(h, 1), max_resend, (const uint32_t*)nullptr, &t.ctr->unres[0]));
    if (max_resend && sync_rounds) {
        for (uint32_t r = 1;; ++r) {
            uint32_t unresolved = 0;
            GD_TRY(read_back(h, &t.ctr->unres[(r - 1) % CB_ROUNDS], &unresolved, 1));
            if (!unresolved) break;
            if (r > max_resend + 2u) return set_err(h, GD_ETIMEOUT, "%s: the rounds did not settle", call);
            HIP_TRY(h, hipMemsetAsync(&t.ctr->unres[r % CB_ROUNDS], 0, 4, h->stream));
            GD_TRY(launch(h, "k_cb_resolve", grid, block, 0, k_cb_resolve, a, n, t, (const uint32_t*)slot_of, cls,
                          cb_word(h, r & 1u), cb_word(h, (r + 1u) & 1u), max_resend, (const uint32_t*)nullptr,
                          &t.ctr->unres[r % CB_ROUNDS]));
        }
    } else if (max_resend) {
        // an id's responses need at most max_resend + 2 rounds; past CB_ROUNDS the batch is flagged unsettled
        const uint32_t rounds = std::min<uint32_t>(max_resend + 2u, CB_ROUNDS);
        for (uint32_t r = 1; r < rounds; ++r)
            GD_TRY(launch(h, "k_cb_resolve", grid, block, 0, k_cb_resolve, a, n, t, (const uint32_t*)slot_of, cls,
                          cb_word(h, r & 1u), cb_word(h, (r + 1u) & 1u), max_resend,
                          (const uint32_t*)&t.ctr->unres[r - 1], &t.ctr->unres[r]));
        if (rounds < max_resend + 2u)
            GD_TRY(launch(h, "k_cb_settled", dim3(1), dim3(WAVE), 0, k_cb_settled, t.ctr, rounds - 1u));
    }
    if (fire_idx) {
        const uint32_t tiles = blocks_for(n, PL_TILE);
        GD_TRY(ensure(h, h->cb_scr[2], ((size_t)tiles + 1) * 4));
        uint32_t* tile_cnt = (uint32_t*)h->cb_scr[2].p;
        const uint32_t wide = ((uintptr_t)a.outcome & 15u) == 0 ? 1u : 0u;
        GD_TRY(launch(h, "k_cb_fire_count", dim3(tiles), dim3(PL_NT), 0, k_cb_fire_count, (const uint8_t*)a.outcome, n,
                      wide, tile_cnt, tiles));
        GD_TRY(scan_device<OpAdd>(h, tile_cnt, tiles + 1, false, false, "cb_fire"));
        GD_TRY(launch(h, "k_cb_fire_list", dim3(tiles), dim3(PL_NT), 0, k_cb_fire_list, (const uint8_t*)a.outcome, n,
                      wide, (const uint32_t*)tile_cnt, tiles, fire_idx, n_fire));
    }
    return GD_OK;
}

// expire (by_silo 0) and break_silo (1) on device outputs of `cap` entries.
int scan_apply_device(gd_handle* h, uint32_t by_silo, int64_t now, uint32_t silo, uint32_t cap, int64_t* out_id,
                      uint32_t* out_handle, uint8_t* out_kind, uint32_t* n_out) {
    StageTime stage(h, "stage:cb_scan");
    const CbTab t = cb_tab(h);
    const CbScan a{by_silo, now, cb_silo_in(silo), h->cb_max_resend, h->cb_resend_on_timeout ? 1u : 0u, h->cb_period};
    GD_TRY(ensure(h, h->cb_scr[3], ((size_t)h->cb_cap + 1) * 4));
    uint32_t* pos = (uint32_t*)h->cb_scr[3].p;
    const dim3 grid(blocks_for(h->cb_cap + 1, BLOCK)), block(BLOCK);
    GD_TRY(launch(h, "k_cb_scan_mark", grid, block, 0, k_cb_scan_mark, t, a, pos));
    GD_TRY(scan_device<OpAdd>(h, pos, (uint32_t)(h->cb_cap + 1), false, false, "cb_scan"));
    return launch(h, "k_cb_scan_emit", grid, block, 0, k_cb_scan_emit, t, a, (const uint32_t*)pos, cap, out_id,
                  out_handle, out_kind, n_out);
}

int scan_apply_host(gd_handle* h, uint32_t by_silo, int64_t now, uint32_t silo, uint32_t cap, int64_t* out_id,
                    uint32_t* out_handle, uint8_t* out_kind, uint32_t* n_out, const char* call) {
    GD_TRY(check_handle(h, call));
    if (!n_out || (cap && (!out_id || !out_handle || !out_kind))) return set_err(h, GD_EINVAL, "%s: null argument", call);
    if (by_silo && silo >= CB_SILO_NONE) return set_err(h, GD_EINVAL, "%s: silo index above 0xFFFE", call);
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, call));
    // a list never holds more than the table: outputs of that size stand in for a larger cap
    const uint32_t dcap = (uint32_t)std::min<uint64_t>(cap, h->cb_cap);
    HostStage io(h);
    int64_t* did = io.hold<int64_t>(dcap, 8);          // the first *n_out of the three come down, once it is known
    uint32_t* dhandle = io.hold<uint32_t>(dcap, 4);
    uint8_t* dkind = io.hold<uint8_t>(dcap, 16);
    uint32_t* dn = io.hold<uint32_t>(1);
    GD_TRY(io.status());
    GD_TRY(scan_apply_device(h, by_silo, now, silo, dcap, did, dhandle, dkind, dn));
    GD_TRY(read_back(h, dn, n_out, 1));
    if (*n_out > cap) return set_err(h, GD_EINVAL, "%s: %u entries are due, cap is %u (nothing changed)", call, *n_out, cap);
    GD_TRY(io.fetch(out_id, did, *n_out));
    GD_TRY(io.fetch(out_handle, dhandle, *n_out));
    GD_TRY(io.fetch(out_kind, dkind, *n_out));
    CbCounts c;
    return cb_pull(h, &c, call);
}

}  // namespace

extern "C" {

int gd_callbacks_configure(gd_handle* h, uint64_t capacity_hint, uint32_t max_resend_count, int resend_on_timeout,
                           int64_t period_ticks) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (max_resend_count > 255u) return set_err(h, GD_EINVAL, "gd_callbacks_configure: max_resend_count > 255");
    if (period_ticks < 0) return set_err(h, GD_EINVAL, "gd_callbacks_configure: negative period_ticks");
    if (capacity_hint > CB_MAX_CAP) return set_err(h, GD_EINVAL, "gd_callbacks_configure: capacity_hint > 2^31");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_callbacks_configure"));
    unsigned long long cap = CB_MIN_CAP;
    while (cap < capacity_hint) cap <<= 1;
    if (!h->cb_cap) {
        GD_TRY(ensure(h, h->cb_ctr, sizeof(CbCounters)));
        HIP_TRY(h, hipMemsetAsync(h->cb_ctr.p, 0, sizeof(CbCounters), h->stream));
        GD_TRY(cb_alloc(h, cap, h->cb_tab, h->cb_dl, h->cb_last));
        h->cb_cap = cap;
        h->cb_used_ub = 0;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else if (cap > h->cb_cap) {
        CbCounts c;
        GD_TRY(cb_pull(h, &c, "gd_callbacks_configure"));
        GD_TRY(cb_rebuild(h, cap, c.live));
        h->cb_used_ub = c.live;
    }
    h->cb_max_resend = max_resend_count;
    h->cb_resend_on_timeout = resend_on_timeout != 0;
    h->cb_period = period_ticks;
    return GD_OK;
}

int gd_callbacks_clear(gd_handle* h) {
    GD_TRY(check_handle(h, "gd_callbacks_clear"));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_callbacks_clear"));
    HIP_TRY(h, hipMemsetAsync(h->cb_tab.p, 0, (size_t)h->cb_cap * sizeof(CbSlot), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->cb_last.p, 0, (size_t)h->cb_cap * 8, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->cb_ctr.p, 0, sizeof(CbCounters), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->cb_used_ub = 0;
    return GD_OK;
}

int gd_callbacks_count(gd_handle* h, uint64_t* out_live, uint64_t* out_capacity) {
    GD_TRY(check_handle(h, "gd_callbacks_count"));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_callbacks_count"));
    CbCounts c;
    GD_TRY(cb_pull(h, &c, "gd_callbacks_count"));
    h->cb_used_ub = (uint64_t)c.live + c.tomb;
    if (out_live) *out_live = c.live;
    if (out_capacity) *out_capacity = h->cb_cap;
    return GD_OK;
}

int gd_callbacks_add_device(gd_handle* h, const int64_t* d_ids, const uint32_t* d_handles, const int64_t* d_deadlines,
                            uint32_t n, uint8_t* d_out_added) {
    GD_TRY(check_handle(h, "gd_callbacks_add_device", n));
    if (n && (!d_ids || !d_handles || !d_deadlines)) return set_err(h, GD_EINVAL, "gd_callbacks_add_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return add_device(h, d_ids, d_handles, d_deadlines, n, d_out_added, false, "gd_callbacks_add_device");
}

int gd_callbacks_add(gd_handle* h, const int64_t* ids, const uint32_t* handles, const int64_t* deadlines, uint32_t n,
                     uint8_t* out_added) {
    GD_TRY(check_handle(h, "gd_callbacks_add", n));
    if (n && (!ids || !handles || !deadlines)) return set_err(h, GD_EINVAL, "gd_callbacks_add: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_callbacks_add"));
    HostStage io(h);
    const int64_t* di = io.in(ids, n);
    const uint32_t* dh = io.in(handles, n);
    const int64_t* dd = io.in(deadlines, n);
    uint8_t* dadded = io.out(out_added, n, 16);
    GD_TRY(io.status());
    GD_TRY(add_device(h, di, dh, dd, n, dadded, true, "gd_callbacks_add"));
    GD_TRY(io.fetch());
    CbCounts c;
    return cb_pull(h, &c, "gd_callbacks_add");
}

int gd_callbacks_set_target_device(gd_handle* h, const int64_t* d_ids, const uint32_t* d_silo, uint32_t n,
                                   uint8_t* d_out_found) {
    GD_TRY(check_handle(h, "gd_callbacks_set_target_device", n));
    if (n && (!d_ids || !d_silo)) return set_err(h, GD_EINVAL, "gd_callbacks_set_target_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return set_target_device(h, d_ids, d_silo, n, d_out_found);
}

int gd_callbacks_set_target(gd_handle* h, const int64_t* ids, const uint32_t* silo, uint32_t n, uint8_t* out_found) {
    GD_TRY(check_handle(h, "gd_callbacks_set_target", n));
    if (n && (!ids || !silo)) return set_err(h, GD_EINVAL, "gd_callbacks_set_target: null argument");
    for (uint32_t i = 0; i < n; ++i)
        if (silo[i] != GD_CB_NO_SILO && silo[i] >= CB_SILO_NONE)
            return set_err(h, GD_EINVAL, "gd_callbacks_set_target: silo index above 0xFFFE at %u", i);
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_callbacks_set_target"));
    HostStage io(h);
    const int64_t* di = io.in(ids, n);
    const uint32_t* ds = io.in(silo, n);
    uint8_t* dfound = io.out(out_found, n, 16);
    GD_TRY(io.status());
    GD_TRY(set_target_device(h, di, ds, n, dfound));
    GD_TRY(io.fetch());
    CbCounts c;
    return cb_pull(h, &c, "gd_callbacks_set_target");
}

int gd_callbacks_lookup_device(gd_handle* h, const int64_t* d_ids, uint32_t n, uint32_t* d_out_handle,
                               uint32_t* d_out_resend, uint32_t* d_out_silo, uint8_t* d_out_found) {
    GD_TRY(check_handle(h, "gd_callbacks_lookup_device", n));
    if (n && !d_ids) return set_err(h, GD_EINVAL, "gd_callbacks_lookup_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return lookup_device(h, d_ids, n, d_out_handle, d_out_resend, d_out_silo, d_out_found);
}

int gd_callbacks_lookup(gd_handle* h, const int64_t* ids, uint32_t n, uint32_t* out_handle, uint32_t* out_resend,
                        uint32_t* out_silo, uint8_t* out_found) {
    GD_TRY(check_handle(h, "gd_callbacks_lookup", n));
    if (n && !ids) return set_err(h, GD_EINVAL, "gd_callbacks_lookup: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_callbacks_lookup"));
    HostStage io(h);
    const int64_t* di = io.in(ids, n);
    uint32_t* dhandle = io.out(out_handle, n, 4);
    uint32_t* dresend = io.out(out_resend, n, 4);
    uint32_t* dsilo = io.out(out_silo, n, 4);
    uint8_t* dfound = io.out(out_found, n, 16);
    GD_TRY(io.status());
    GD_TRY(lookup_device(h, di, n, dhandle, dresend, dsilo, dfound));
    GD_TRY(io.fetch());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_callbacks_respond_device(gd_handle* h, const int64_t* d_ids, const uint8_t* d_result,
                                const uint8_t* d_rejection_type, const uint8_t* d_flags, const uint8_t* d_turn,
                                uint32_t n, uint8_t* d_out_outcome, uint8_t* d_out_flags, uint32_t* d_out_handle,
                                uint32_t* d_fire_idx, uint32_t* d_n_fire) {
    GD_TRY(check_handle(h, "gd_callbacks_respond_device", n));
    if ((d_fire_idx != nullptr) != (d_n_fire != nullptr))
        return set_err(h, GD_EINVAL, "gd_callbacks_respond_device: fire_idx and n_fire go together");
    if (n && (!d_ids || !d_out_outcome || !d_out_flags || !d_out_handle))
        return set_err(h, GD_EINVAL, "gd_callbacks_respond_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    const CbResp a{d_ids, d_result, d_rejection_type, d_flags, d_turn, d_out_outcome, d_out_flags, d_out_handle};
    return respond_device(h, a, n, d_fire_idx, d_n_fire, false, "gd_callbacks_respond_device");
}

int gd_callbacks_respond(gd_handle* h, const int64_t* ids, const uint8_t* result, const uint8_t* rejection_type,
                         const uint8_t* flags, const uint8_t* turn, uint32_t n, uint8_t* out_outcome,
                         uint8_t* out_flags, uint32_t* out_handle, uint32_t* fire_idx, uint32_t* n_fire) {
    GD_TRY(check_handle(h, "gd_callbacks_respond", n));
    if ((fire_idx != nullptr) != (n_fire != nullptr))
        return set_err(h, GD_EINVAL, "gd_callbacks_respond: fire_idx and n_fire go together");
    if (n && (!ids || !out_outcome || !out_flags || !out_handle))
        return set_err(h, GD_EINVAL, "gd_callbacks_respond: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_callbacks_respond"));
    HostStage io(h);
    CbResp a{};
    a.ids = io.in(ids, n);
    a.result = io.in(result, n);
    a.rejection = io.in(rejection_type, n);
    a.flags = io.in(flags, n);
    a.turn = io.in(turn, n);
    a.outcome = io.out(out_outcome, n, 16);
    a.oflags = io.out(out_flags, n, 16);
    a.handle = io.out(out_handle, n, 4);
    // the whole fire list comes down (n entries at most); the host reads the first *n_fire
    uint32_t* dfire = io.out_if(fire_idx, n, 4);
    uint32_t* dnf = io.out_if(n_fire, 1);
    GD_TRY(io.status());
    GD_TRY(respond_device(h, a, n, dfire, dnf, true, "gd_callbacks_respond"));
    GD_TRY(io.fetch());
    CbCounts c;
    return cb_pull(h, &c, "gd_callbacks_respond");
}

int gd_callbacks_expire_device(gd_handle* h, int64_t now, uint32_t cap, int64_t* d_out_id, uint32_t* d_out_handle,
                               uint8_t* d_out_kind, uint32_t* d_n_out) {
    GD_TRY(check_handle(h, "gd_callbacks_expire_device"));
    if (!d_n_out || (cap && (!d_out_id || !d_out_handle || !d_out_kind)))
        return set_err(h, GD_EINVAL, "gd_callbacks_expire_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return scan_apply_device(h, 0u, now, 0u, cap, d_out_id, d_out_handle, d_out_kind, d_n_out);
}

int gd_callbacks_expire(gd_handle* h, int64_t now, uint32_t cap, int64_t* out_id, uint32_t* out_handle,
                        uint8_t* out_kind, uint32_t* n_out) {
    return scan_apply_host(h, 0u, now, 0u, cap, out_id, out_handle, out_kind, n_out, "gd_callbacks_expire");
}

int gd_callbacks_break_silo_device(gd_handle* h, uint32_t silo, uint32_t cap, int64_t* d_out_id, uint32_t* d_out_handle,
                                   uint8_t* d_out_kind, uint32_t* d_n_out) {
    GD_TRY(check_handle(h, "gd_callbacks_break_silo_device"));
    if (!d_n_out || (cap && (!d_out_id || !d_out_handle || !d_out_kind)))
        return set_err(h, GD_EINVAL, "gd_callbacks_break_silo_device: null argument");
    if (silo >= CB_SILO_NONE) return set_err(h, GD_EINVAL, "gd_callbacks_break_silo_device: silo index above 0xFFFE");
    HIP_TRY(h, hipSetDevice(h->device));
    return scan_apply_device(h, 1u, 0, silo, cap, d_out_id, d_out_handle, d_out_kind, d_n_out);
}

int gd_callbacks_break_silo(gd_handle* h, uint32_t silo, uint32_t cap, int64_t* out_id, uint32_t* out_handle,
                            uint8_t* out_kind, uint32_t* n_out) {
    return scan_apply_host(h, 1u, 0, silo, cap, out_id, out_handle, out_kind, n_out, "gd_callbacks_break_silo");
}

}  // extern "C"
