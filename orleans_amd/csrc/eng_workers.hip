// eng_workers.hip -- libgraindispatch: the stateless-worker stage (gd_workers.h): the worker sets of
// ActivationDirectory (RecordNewTarget, RemoveTarget, FindTargets) and StatelessWorkerDirector.SelectActivationCore
// for a batch.  Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_scan.h"
#include "gd_workers.h"

namespace {

constexpr unsigned long long WK_MIN_CAP = 64, WK_MAX_CAP = 1ull << 31;

size_t wk_side_bytes(uint32_t sc) { return (size_t)(WK_HDR + sc) * 4; }

WkTab wk_tab(gd_handle* h) {
    return WkTab{(Slot*)h->wk_slots.p, h->wk_cap - 1ull, (DevCounters*)h->wk_ctr.p, (uint32_t*)h->wk_last.p,
                 (uint32_t*)h->wk_side.p, h->wk_sc};
}
uint32_t* wk_retry(gd_handle* h) { return (uint32_t*)h->wk_state.p; }
uint32_t* wk_miss(gd_handle* h) { return wk_retry(h) + WK_PASSES; }

int check_handle(gd_handle* h, const char* call, uint64_t n = 0) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (!h->wk_sc) return set_err(h, GD_ESTATE, "%s before gd_workers_configure", call);
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "%s: n > 2^31", call);
    return GD_OK;
}

// The table's counters after a synchronisation; device error bits are cleared and reported once.
int wk_pull(gd_handle* h, DevCounters* c, const char* call) {
    DevCounters* d = (DevCounters*)h->wk_ctr.p;
    GD_TRY(fold_counters(h, d));
    GD_TRY(read_back(h, d, (uint32_t*)c, sizeof(DevCounters) / 4));
    if (!c->err) return GD_OK;
    GD_TRY(table_err_clear(h, &d->err, c->err, h->wk_last, h->wk_cap));
    if (c->err & WK_ERR_FULL) return set_err(h, GD_EFULL, "%s: the worker-set table is full (0x%x)", call, c->err);
    return set_err(h, GD_ETIMEOUT, "%s: an earlier device batch did not settle in the worker-set table (0x%x)", call, c->err);
}

// Rebuild on the stream at `cap` slots: the live sets move with their lists, the tombstones go.
int wk_rebuild(gd_handle* h, unsigned long long cap) {
    if (cap > WK_MAX_CAP) return set_err(h, GD_EFULL, "worker-set table: more than 2^31 slots");
    DevBuf fresh[3];
    GD_TRY(table_alloc(h, "worker-set", cap, sizeof(Slot), wk_side_bytes(h->wk_sc), fresh[0], fresh[1], fresh[2]));
    const WkTab old = wk_tab(h);
    const unsigned long long old_cap = h->wk_cap;
    HIP_TRY(h, hipMemsetAsync(old.ctr, 0, CTR_BYTES, h->stream));      // k_wk_rehash counts live and max_probe anew
    const WkTab to{(Slot*)fresh[0].p, cap - 1ull, old.ctr, (uint32_t*)fresh[2].p, (uint32_t*)fresh[1].p, h->wk_sc};
    GD_TRY(launch(h, "k_wk_rehash", dim3(blocks_for(old_cap, BLOCK)), dim3(BLOCK), 0, k_wk_rehash,
                  (const Slot*)old.slots, (const uint32_t*)old.side, old_cap, to));
    return table_swap(h, {&h->wk_slots, &h->wk_side, &h->wk_last}, fresh, h->wk_cap, cap);
}

// What a batch of n keys shares: slot_of / is_new, then (after the claims) perm, offsets over the table's slots
// and the inverse permutation.
struct WkBatch {
    uint32_t *slot_of, *perm, *offsets, *rank;
    uint8_t* is_new;
};
int wk_scratch(gd_handle* h, uint32_t n, WkBatch& b) {
    GD_TRY(ensure(h, h->wk_scr[0], (size_t)n * 4));
    GD_TRY(ensure(h, h->wk_scr[1], (size_t)n + 16));
    GD_TRY(ensure(h, h->wk_scr[2], (size_t)n * 4));
    GD_TRY(ensure(h, h->wk_scr[4], (size_t)n * 4));
    b.slot_of = (uint32_t*)h->wk_scr[0].p;
    b.is_new = (uint8_t*)h->wk_scr[1].p;
    b.perm = (uint32_t*)h->wk_scr[2].p;
    b.rank = (uint32_t*)h->wk_scr[4].p;
    b.offsets = nullptr;
    return GD_OK;
}
// offsets (and the idle counts) are sized by the table: taken after any growth.
int wk_slot_scratch(gd_handle* h, WkBatch& b) {
    GD_TRY(ensure(h, h->wk_scr[3], ((size_t)h->wk_cap + 2) * 4));
    GD_TRY(ensure(h, h->wk_scr[5], (size_t)h->wk_cap * 4));
    b.offsets = (uint32_t*)h->wk_scr[3].p;
    return GD_OK;
}

// k_wk_find over the batch, room for the sets it may create, the claim passes, the bucketing over slots.
// pre8 / pre_ctx: k_wk_find's preset outputs.  Growth moves the sets, so the find is repeated after it.
int wk_find_claim_bucket(gd_handle* h, const gd_key* keys, const int32_t* max_local, uint32_t n, bool claim,
                         WkBatch& b, uint8_t* pre8, uint32_t pre_other, uint32_t pre_held, uint32_t* pre_ctx,
                         bool sync_passes, const char* call) {
    GD_TRY(wk_scratch(h, n, b));
    const dim3 grid(blocks_for(n, BLOCK)), block(BLOCK);
    auto find = [&]() {
        HIP_TRY(h, hipMemsetAsync(wk_miss(h), 0, 4, h->stream));
        return launch(h, "k_wk_find", grid, block, 0, k_wk_find, keys, n, wk_tab(h), max_local, claim ? 1u : 0u,
                      b.slot_of, b.is_new, wk_miss(h), pre8, pre_other, pre_held, pre_ctx);
    };
    GD_TRY(find());
    if (claim) {
        if ((h->wk_used_ub + n) * 4 <= h->wk_cap * 3) {
            h->wk_used_ub += n;
        } else {
            // the bound cannot tell: the batch's own count of set-less messages decides
            uint32_t misses = 0;
            GD_TRY(read_back(h, wk_miss(h), &misses, 1));
            if (misses) {
                bool moved = false;
                GD_TRY(table_reserve(
                    h, h->wk_used_ub, h->wk_cap, misses, call,
                    [&](uint64_t& live, uint64_t& tomb) {
                        DevCounters c;
                        GD_TRY(wk_pull(h, &c, call));
                        live = c.live;
                        tomb = c.tomb;
                        return (int)GD_OK;
                    },
                    [&](unsigned long long cap, uint64_t) {
                        moved = true;
                        return wk_rebuild(h, cap);
                    }));
                if (moved) GD_TRY(find());
            }
        }
        const WkTab t = wk_tab(h);
        const uint32_t* unsettled = nullptr;
        GD_TRY(claim_pass_driver(h, wk_retry(h), WK_PASSES, sync_passes, call, &unsettled,
                                 [&](uint32_t p, const uint32_t* gate, uint32_t* word) {
                                     return launch(h, "k_wk_claim", grid, block, 0, k_wk_claim, keys, n, t, b.slot_of,
                                                   b.is_new, p, p == 0 ? (const uint32_t*)wk_miss(h) : gate, word);
                                 }));
        if (unsettled) GD_TRY(launch(h, "k_wk_settled", dim3(1), dim3(WAVE), 0, k_wk_settled, t.ctr, unsettled));
    }
    GD_TRY(wk_slot_scratch(h, b));
    return bucket_device(h, b.slot_of, n, (uint32_t)h->wk_cap, b.perm, b.offsets, b.rank);
}

struct WkSelectArgs {
    const int32_t* max_local;
    const uint32_t* draw;
    uint32_t ctx_base;
    WkTurns turns;
    uint32_t* ctx;
    uint8_t* pick;
    uint32_t *new_idx, *n_new;
};

int select_device(gd_handle* h, const gd_key* keys, uint32_t n, const WkSelectArgs& a, bool sync_passes,
                  const char* call) {
    if (n == 0) {
        if (a.n_new) HIP_TRY(h, hipMemsetAsync(a.n_new, 0, 4, h->stream));
        return GD_OK;
    }
    StageTime stage(h, "stage:wk_select");
    WkBatch b;
    GD_TRY(wk_find_claim_bucket(h, keys, a.max_local, n, true, b, a.pick, GD_WK_NONE, GD_WK_HELD, a.ctx, sync_passes,
                                call));
    GD_TRY(ensure(h, h->wk_scr[6], ((size_t)n + 1) * 4));
    uint32_t* acnt = (uint32_t*)h->wk_scr[5].p;
    uint32_t* pos = (uint32_t*)h->wk_scr[6].p;
    const WkTab t = wk_tab(h);
    const dim3 grid(blocks_for(n, BLOCK)), grid1(blocks_for((uint64_t)n + 1, BLOCK)), block(BLOCK);
    GD_TRY(launch(h, "k_wk_sets", dim3(blocks_for(h->wk_cap, BLOCK / WAVE)), dim3(BLOCK), 0, k_wk_sets, t,
                  (const uint32_t*)b.offsets, (const uint32_t*)b.perm, n, a.max_local, h->wk_default_ml, 1u, a.turns,
                  acnt, a.ctx));
    GD_TRY(launch(h, "k_wk_classify", grid1, block, 0, k_wk_classify, n, t, (const uint32_t*)b.slot_of,
                  (const uint32_t*)b.rank, (const uint32_t*)b.offsets, (const uint32_t*)acnt, a.draw, a.pick, pos));
    GD_TRY(scan_device<OpAdd>(h, pos, n + 1, false, false, "wk_select"));
    GD_TRY(launch(h, "k_wk_finish", grid, block, 0, k_wk_finish, n, t, (const uint32_t*)b.slot_of,
                  (const uint32_t*)b.rank, (const uint32_t*)b.offsets, (const uint32_t*)b.perm, (const uint32_t*)acnt,
                  a.draw, (const uint32_t*)pos, a.ctx_base, (const uint8_t*)a.pick, a.ctx, a.new_idx, a.n_new));
    return launch(h, "k_wk_commit", dim3(blocks_for(h->wk_cap, BLOCK)), block, 0, k_wk_commit, t,
                  (const uint32_t*)b.offsets, (const uint32_t*)acnt);
}

int add_device(gd_handle* h, const gd_key* keys, const uint32_t* ctx, const int32_t* max_local, uint32_t n,
               uint8_t* out_status, bool sync_passes, const char* call) {
    if (n == 0) return GD_OK;
    StageTime stage(h, "stage:wk_add");
    WkBatch b;
    GD_TRY(wk_find_claim_bucket(h, keys, max_local, n, true, b, out_status, GD_WK_NOT_GRAIN, GD_WK_FULL, nullptr,
                                sync_passes, call));
    const WkTab t = wk_tab(h);
    const dim3 slots(blocks_for(h->wk_cap, BLOCK)), block(BLOCK);
    GD_TRY(launch(h, "k_wk_sets", dim3(blocks_for(h->wk_cap, BLOCK / WAVE)), dim3(BLOCK), 0, k_wk_sets, t,
                  (const uint32_t*)b.offsets, (const uint32_t*)b.perm, n, max_local, h->wk_default_ml, 0u, WkTurns{},
                  (uint32_t*)nullptr, (uint32_t*)nullptr));
    GD_TRY(launch(h, "k_wk_add_apply", dim3(blocks_for(n, BLOCK)), block, 0, k_wk_add_apply, ctx, n, t,
                  (const uint32_t*)b.slot_of, (const uint32_t*)b.rank, (const uint32_t*)b.offsets, out_status));
    return launch(h, "k_wk_add_commit", slots, block, 0, k_wk_add_commit, t, (const uint32_t*)b.offsets);
}

int remove_device(gd_handle* h, const gd_key* keys, const uint32_t* ctx, uint32_t n, uint8_t* out_removed,
                  const char* call) {
    if (n == 0) return GD_OK;
    StageTime stage(h, "stage:wk_remove");
    WkBatch b;
    // a pair whose grain has no set is reported here; k_wk_remove_sets reports the others
    GD_TRY(wk_find_claim_bucket(h, keys, nullptr, n, false, b, out_removed, 0u, 0u, nullptr, false, call));
    return launch(h, "k_wk_remove_sets", dim3((uint32_t)h->wk_cap), dim3(WK_SET_NT), 0, k_wk_remove_sets, wk_tab(h),
                  (const uint32_t*)b.offsets, (const uint32_t*)b.perm, ctx, out_removed);
}

int lookup_device(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t* out_count, uint32_t* out_max_local,
                  uint32_t* out_list) {
    return launch(h, "k_wk_lookup", dim3(n), dim3(WK_SET_NT), 0, k_wk_lookup, keys, wk_tab(h), out_count, out_max_local,
                  out_list);
}

int check_select(gd_handle* h, const char* call, const void* keys, uint32_t n, uint32_t ctx_base, uint32_t n_ctx,
                 const void* ctx_flags, const void* num_running, const void* ctx, const void* pick, const void* new_idx,
                 const void* n_new) {
    GD_TRY(check_handle(h, call, n));
    if ((new_idx != nullptr) != (n_new != nullptr)) return set_err(h, GD_EINVAL, "%s: new_idx and n_new go together", call);
    if (n && (!keys || !ctx || !pick)) return set_err(h, GD_EINVAL, "%s: null argument", call);
    if (n && n_ctx && (!ctx_flags || !num_running)) return set_err(h, GD_EINVAL, "%s: null context array", call);
    if ((uint64_t)ctx_base + n > GD_ACT_MULTI)
        return set_err(h, GD_EINVAL, "%s: ctx_base + n passes GD_ACT_MULTI", call);
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_workers_configure(gd_handle* h, uint64_t capacity, uint32_t slot_capacity, uint32_t default_max_local) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (slot_capacity < 1 || slot_capacity > GD_WK_MAX_SLOT_CAPACITY)
        return set_err(h, GD_EINVAL, "gd_workers_configure: slot_capacity %u not in 1..%u", slot_capacity,
                       GD_WK_MAX_SLOT_CAPACITY);
    if (default_max_local < 1 || default_max_local > slot_capacity)
        return set_err(h, GD_EINVAL, "gd_workers_configure: default_max_local %u not in 1..slot_capacity", default_max_local);
    if (capacity > WK_MAX_CAP / 2) return set_err(h, GD_EINVAL, "gd_workers_configure: capacity > 2^30");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_workers_configure"));
    unsigned long long cap = WK_MIN_CAP;
    while (cap * 3 < capacity * 4) cap <<= 1;             // `capacity` sets at load <= 0.75
    if (h->wk_sc && h->wk_sc != slot_capacity) {
        DevCounters c;
        GD_TRY(wk_pull(h, &c, "gd_workers_configure"));
        if (c.live)
            return set_err(h, GD_EINVAL, "gd_workers_configure: slot_capacity changes while %llu sets are present", c.live);
        h->wk_sc = 0;
    }
    if (!h->wk_sc) {
        GD_TRY(ensure(h, h->wk_state, (WK_PASSES + 1) * 4));
        HIP_TRY(h, hipMemsetAsync(h->wk_state.p, 0, (WK_PASSES + 1) * 4, h->stream));
        GD_TRY(ensure(h, h->wk_ctr, CTR_BYTES));
        HIP_TRY(h, hipMemsetAsync(h->wk_ctr.p, 0, CTR_BYTES, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (DevBuf* b : {&h->wk_slots, &h->wk_side, &h->wk_last}) free_buf(*b);
        cap = std::max(cap, h->wk_cap);
        GD_TRY(table_alloc(h, "worker-set", cap, sizeof(Slot), wk_side_bytes(slot_capacity), h->wk_slots, h->wk_side,
                           h->wk_last));
        h->wk_cap = cap;
        h->wk_used_ub = 0;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->wk_sc = slot_capacity;
    } else if (cap > h->wk_cap) {
        DevCounters c;
        GD_TRY(wk_pull(h, &c, "gd_workers_configure"));
        GD_TRY(wk_rebuild(h, cap));
        h->wk_used_ub = c.live;
    }
    h->wk_default_ml = default_max_local;
    return GD_OK;
}

int gd_workers_clear(gd_handle* h) {
    GD_TRY(check_handle(h, "gd_workers_clear"));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_workers_clear"));
    HIP_TRY(h, hipMemsetAsync(h->wk_slots.p, 0, (size_t)h->wk_cap * sizeof(Slot), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->wk_last.p, 0, (size_t)h->wk_cap * 8, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->wk_ctr.p, 0, CTR_BYTES, h->stream));
    h->wk_used_ub = 0;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_workers_count(gd_handle* h, uint64_t* out_sets, uint64_t* out_capacity) {
    GD_TRY(check_handle(h, "gd_workers_count"));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_workers_count"));
    DevCounters c;
    GD_TRY(wk_pull(h, &c, "gd_workers_count"));
    h->wk_used_ub = c.live + c.tomb;
    if (out_sets) *out_sets = c.live;
    if (out_capacity) *out_capacity = h->wk_cap;
    return GD_OK;
}

int gd_workers_add_device(gd_handle* h, const gd_key* d_grains, const uint32_t* d_ctx, const int32_t* d_max_local,
                          uint32_t n, uint8_t* d_out_status) {
    GD_TRY(check_handle(h, "gd_workers_add_device", n));
    if (n && (!d_grains || !d_ctx || !d_out_status)) return set_err(h, GD_EINVAL, "gd_workers_add_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_workers_add_device"));
    return add_device(h, d_grains, d_ctx, d_max_local, n, d_out_status, false, "gd_workers_add_device");
}

int gd_workers_add(gd_handle* h, const gd_key* grains, const uint32_t* ctx, const int32_t* max_local, uint32_t n,
                   uint8_t* out_status) {
    GD_TRY(check_handle(h, "gd_workers_add", n));
    if (n && (!grains || !ctx || !out_status)) return set_err(h, GD_EINVAL, "gd_workers_add: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_workers_add"));
    HostStage io(h);
    const gd_key* dk = io.in(grains, n);
    const uint32_t* dc = io.in(ctx, n);
    const int32_t* dm = io.in(max_local, n);
    uint8_t* dst = io.out(out_status, n, 16);
    GD_TRY(io.status());
    GD_TRY(add_device(h, dk, dc, dm, n, dst, true, "gd_workers_add"));
    GD_TRY(io.fetch());
    DevCounters c;
    return wk_pull(h, &c, "gd_workers_add");
}

int gd_workers_remove_device(gd_handle* h, const gd_key* d_grains, const uint32_t* d_ctx, uint32_t n,
                             uint8_t* d_out_removed) {
    GD_TRY(check_handle(h, "gd_workers_remove_device", n));
    if (n && (!d_grains || !d_ctx)) return set_err(h, GD_EINVAL, "gd_workers_remove_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_workers_remove_device"));
    return remove_device(h, d_grains, d_ctx, n, d_out_removed, "gd_workers_remove_device");
}

int gd_workers_remove(gd_handle* h, const gd_key* grains, const uint32_t* ctx, uint32_t n, uint8_t* out_removed) {
    GD_TRY(check_handle(h, "gd_workers_remove", n));
    if (n && (!grains || !ctx)) return set_err(h, GD_EINVAL, "gd_workers_remove: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_workers_remove"));
    HostStage io(h);
    const gd_key* dk = io.in(grains, n);
    const uint32_t* dc = io.in(ctx, n);
    uint8_t* drm = io.out_if(out_removed, n, 16);
    GD_TRY(io.status());
    GD_TRY(remove_device(h, dk, dc, n, drm, "gd_workers_remove"));
    GD_TRY(io.fetch());
    DevCounters c;
    return wk_pull(h, &c, "gd_workers_remove");
}

int gd_workers_lookup_device(gd_handle* h, const gd_key* d_grains, uint32_t n, uint32_t* d_out_count,
                             uint32_t* d_out_max_local, uint32_t* d_out_list) {
    GD_TRY(check_handle(h, "gd_workers_lookup_device", n));
    if (n && !d_grains) return set_err(h, GD_EINVAL, "gd_workers_lookup_device: null argument");
    if (n > 0x7FFFFFFFu) return set_err(h, GD_EINVAL, "gd_workers_lookup_device: n > 2^31 - 1");
    HIP_TRY(h, hipSetDevice(h->device));
    return lookup_device(h, d_grains, n, d_out_count, d_out_max_local, d_out_list);
}

int gd_workers_lookup(gd_handle* h, const gd_key* grains, uint32_t n, uint32_t* out_count, uint32_t* out_max_local,
                      uint32_t* out_list) {
    GD_TRY(check_handle(h, "gd_workers_lookup", n));
    if (n && !grains) return set_err(h, GD_EINVAL, "gd_workers_lookup: null argument");
    if (n > 0x7FFFFFFFu) return set_err(h, GD_EINVAL, "gd_workers_lookup: n > 2^31 - 1");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_workers_lookup"));
    HostStage io(h);
    const gd_key* dk = io.in(grains, n);
    uint32_t* dcount = io.out_if(out_count, n, 4);
    uint32_t* dml = io.out_if(out_max_local, n, 4);
    uint32_t* dlist = io.out_if(out_list, (size_t)n * h->wk_sc, 4);
    GD_TRY(io.status());
    GD_TRY(lookup_device(h, dk, n, dcount, dml, dlist));
    GD_TRY(io.fetch());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_workers_select_device(gd_handle* h, const gd_key* d_grains, uint32_t n, const int32_t* d_max_local,
                             const uint32_t* d_draw, uint32_t ctx_base, uint32_t n_ctx, const uint8_t* d_ctx_flags,
                             const uint32_t* d_num_running, const uint32_t* d_wait_offsets, uint32_t* d_ctx,
                             uint8_t* d_pick, uint32_t* d_new_idx, uint32_t* d_n_new) {
    GD_TRY(check_select(h, "gd_workers_select_device", d_grains, n, ctx_base, n_ctx, d_ctx_flags, d_num_running, d_ctx,
                        d_pick, d_new_idx, d_n_new));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_workers_select_device"));
    const WkSelectArgs a{d_max_local, d_draw, ctx_base, WkTurns{n_ctx, d_ctx_flags, d_num_running, d_wait_offsets},
                         d_ctx,       d_pick, d_new_idx, d_n_new};
    return select_device(h, d_grains, n, a, false, "gd_workers_select_device");
}

int gd_workers_select(gd_handle* h, const gd_key* grains, uint32_t n, const int32_t* max_local, const uint32_t* draw,
                      uint32_t ctx_base, uint32_t n_ctx, const uint8_t* ctx_flags, const uint32_t* num_running,
                      const uint32_t* wait_offsets, uint32_t* out_ctx, uint8_t* out_pick, uint32_t* out_new_idx,
                      uint32_t* n_new) {
    GD_TRY(check_select(h, "gd_workers_select", grains, n, ctx_base, n_ctx, ctx_flags, num_running, out_ctx, out_pick,
                        out_new_idx, n_new));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_workers_select"));
    HostStage io(h);
    WkSelectArgs a{};
    const gd_key* dk = io.in(grains, n);
    a.max_local = io.in(max_local, n);
    a.draw = io.in(draw, n);
    a.ctx_base = ctx_base;
    a.turns.n_ctx = n_ctx;
    a.turns.ctx_flags = io.in(ctx_flags, n_ctx);
    a.turns.num_running = io.in(num_running, n_ctx);
    a.turns.wait_offsets = io.in(wait_offsets, (size_t)n_ctx + 1);
    a.ctx = io.out(out_ctx, n, 4);
    a.pick = io.out(out_pick, n, 16);
    // the whole list comes down (n entries at most); the host reads the first *n_new
    a.new_idx = io.out_if(out_new_idx, n, 4);
    a.n_new = io.out_if(n_new, 1);
    GD_TRY(io.status());
    GD_TRY(select_device(h, dk, n, a, true, "gd_workers_select"));
    GD_TRY(io.fetch());
    DevCounters c;
    return wk_pull(h, &c, "gd_workers_select");
}

}  // extern "C"
