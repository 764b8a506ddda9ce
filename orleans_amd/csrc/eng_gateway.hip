// eng_gateway.hip -- libgraindispatch: the gateway stage (gd_gateway.h): the client table and the
// reply routes of Messaging/Gateway.cs, RecordOpenedSocket / RecordClosedSocket, the cleanup agent's two scans,
// TryDeliverToProxy with GatewaySender.Process's decision, the send stage with the proxy check in its place, and
// GatewayAcceptor.HandleMessage, for a batch.  Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_gateway.h"

namespace {

constexpr unsigned long long GW_MIN_CAP = 64, GW_MAX_CAP = 1ull << 31;
constexpr int GW_CLIENTS = 0, GW_ROUTES = 1;
constexpr size_t GW_LDS_MAX = 65536;          // a workgroup's LDS without an opt-in

size_t side_bytes(int t) { return t == GW_CLIENTS ? sizeof(GwClient) : sizeof(int64_t); }

GwTab gw_tab(gd_handle* h, int t) {
    return GwTab{(Slot*)h->gw_slots[t].p, h->gw_cap[t] - 1ull, (DevCounters*)h->gw_ctr[t].p, (uint32_t*)h->gw_last[t].p};
}
GwClient* gw_clients(gd_handle* h) { return (GwClient*)h->gw_side[GW_CLIENTS].p; }
int64_t* gw_times(gd_handle* h) { return (int64_t*)h->gw_side[GW_ROUTES].p; }
GwState* gw_state(gd_handle* h) { return (GwState*)h->gw_state.p; }

int check_handle(gd_handle* h, const char* call, uint64_t n = 0) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (!h->gw_nsenders) return set_err(h, GD_ESTATE, "%s before gd_gateway_configure", call);
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "%s: n > 2^31", call);
    return GD_OK;
}

// A table's counters after a synchronisation; device error bits are cleared and reported once.
int gw_pull(gd_handle* h, int t, DevCounters* c, const char* call) {
    DevCounters* d = (DevCounters*)h->gw_ctr[t].p;
    GD_TRY(fold_counters(h, d));
    GD_TRY(read_back(h, d, (uint32_t*)c, sizeof(DevCounters) / 4));
    if (!c->err) return GD_OK;
    GD_TRY(table_err_clear(h, &d->err, c->err, h->gw_last[t], h->gw_cap[t]));
    const char* what = t == GW_CLIENTS ? "client" : "route";
    if (c->err & GW_ERR_FULL) return set_err(h, GD_EFULL, "%s: the gateway's %s table is full (0x%x)", call, what, c->err);
    return set_err(h, GD_ETIMEOUT, "%s: an earlier device batch did not settle in the %s table (0x%x)", call, what, c->err);
}
int gw_pull_both(gd_handle* h, const char* call) {
    DevCounters c;
    GD_TRY(gw_pull(h, GW_CLIENTS, &c, call));
    return gw_pull(h, GW_ROUTES, &c, call);
}

// A zeroed table of `cap` slots with its values and election words.
int gw_alloc(gd_handle* h, int t, unsigned long long cap, DevBuf& slots, DevBuf& side, DevBuf& last) {
    return table_alloc(h, "gateway", cap, sizeof(Slot), side_bytes(t), slots, side, last);
}

// Rebuild on the stream at `cap` slots: the live entries move with their values, the tombstones go.
int gw_rebuild(gd_handle* h, int t, unsigned long long cap) {
    if (cap > GW_MAX_CAP) return set_err(h, GD_EFULL, "gateway table: more than 2^31 slots");
    DevBuf fresh[3];
    GD_TRY(gw_alloc(h, t, cap, fresh[0], fresh[1], fresh[2]));
    const GwTab old = gw_tab(h, t);
    const unsigned long long old_cap = h->gw_cap[t];
    HIP_TRY(h, hipMemsetAsync(old.ctr, 0, CTR_BYTES, h->stream));      // k_gw_rehash counts live and max_probe anew
    const dim3 grid(blocks_for(old_cap, BLOCK)), block(BLOCK);
    if (t == GW_CLIENTS)
        GD_TRY(launch(h, "k_gw_rehash", grid, block, 0, k_gw_rehash<GwClient>, (const Slot*)old.slots,
                      (const GwClient*)h->gw_side[t].p, old_cap, (Slot*)fresh[0].p, (GwClient*)fresh[1].p, cap - 1ull,
                      old.ctr));
    else
        GD_TRY(launch(h, "k_gw_rehash", grid, block, 0, k_gw_rehash<int64_t>, (const Slot*)old.slots,
                      (const int64_t*)h->gw_side[t].p, old_cap, (Slot*)fresh[0].p, (int64_t*)fresh[1].p, cap - 1ull,
                      old.ctr));
    return table_swap(h, {&h->gw_slots[t], &h->gw_side[t], &h->gw_last[t]}, fresh, h->gw_cap[t], cap);
}

// Room for `incoming` new entries in table t (table_reserve).
int gw_reserve(gd_handle* h, int t, uint64_t incoming, const char* call) {
    return table_reserve(
        h, h->gw_used_ub[t], h->gw_cap[t], incoming, call,
        [&](uint64_t& live, uint64_t& tomb) {
            DevCounters c;
            GD_TRY(gw_pull(h, t, &c, call));
            live = c.live;
            tomb = c.tomb;
            return (int)GD_OK;
        },
        [&](unsigned long long cap, uint64_t) { return gw_rebuild(h, t, cap); });
}

// The claim passes of a batch over table t: pass 0 (init: open's), then read-back driven ones (the host forms) or
// GW_PASSES - 1 gated ones and the unsettled flag (the device forms).
int gw_claims(gd_handle* h, int t, const gd_key* keys, uint32_t n, uint32_t* slot_of, uint8_t* is_new, bool init,
              uint32_t* win, bool elect_all, bool sync_passes, const char* call) {
    const GwTab tab = gw_tab(h, t);
    uint32_t* retry = gw_state(h)->retry[t];
    const dim3 grid(blocks_for(n, BLOCK)), block(BLOCK);
    const uint32_t ea = elect_all ? 1u : 0u;
    const uint32_t* unsettled = nullptr;
    GD_TRY(claim_pass_driver(h, retry, GW_PASSES, sync_passes, call, &unsettled,
                             [&](uint32_t p, const uint32_t* gate, uint32_t* word) {
                                 return launch(h, "k_gw_claim", grid, block, 0, k_gw_claim, keys, n, tab, slot_of, is_new,
                                               p, p == 0 && init ? 1u : 0u, gate, word, win, ea);
                             }));
    if (!unsettled) return GD_OK;
    return launch(h, "k_gw_settled", dim3(1), dim3(WAVE), 0, k_gw_settled, tab.ctr, unsettled);
}

// ---- the batches on device arrays
int open_device(gd_handle* h, const gd_key* ids, const uint32_t* handles, uint32_t n, const GwOpenOut& o,
                bool sync_passes, const char* call) {
    if (n == 0) return GD_OK;
    GD_TRY(gw_reserve(h, GW_CLIENTS, n, call));
    StageTime stage(h, "stage:gw_open");
    GD_TRY(ensure(h, h->gw_scr[0], (size_t)n * 4));
    GD_TRY(ensure(h, h->gw_scr[1], (size_t)n + 16));
    GD_TRY(ensure(h, h->gw_scr[2], ((size_t)n + 1) * 4));
    uint32_t* slot_of = (uint32_t*)h->gw_scr[0].p;
    uint8_t* is_new = (uint8_t*)h->gw_scr[1].p;
    uint32_t* pos = (uint32_t*)h->gw_scr[2].p;
    const GwTab t = gw_tab(h, GW_CLIENTS);
    GD_TRY(gw_claims(h, GW_CLIENTS, ids, n, slot_of, is_new, true, nullptr, true, sync_passes, call));
    const dim3 grid(blocks_for(n, BLOCK)), block(BLOCK);
    GD_TRY(launch(h, "k_gw_open_mark", dim3(blocks_for((uint64_t)n + 1, BLOCK)), block, 0, k_gw_open_mark, n,
                  (const uint32_t*)slot_of, (const uint8_t*)is_new, (const uint32_t*)t.last, pos));
    GD_TRY(scan_device<OpAdd>(h, pos, n + 1, false, false, "gw_open"));
    GD_TRY(launch(h, "k_gw_open_commit", grid, block, 0, k_gw_open_commit, handles, n, t, gw_clients(h),
                  (const GwState*)gw_state(h), h->gw_nsenders, (const uint32_t*)slot_of, (const uint8_t*)is_new,
                  (const uint32_t*)pos, o));
    return launch(h, "k_gw_open_report", grid, block, 0, k_gw_open_report, n, t, gw_state(h), h->gw_nsenders,
                  (const uint32_t*)slot_of, (const uint32_t*)pos, o);
}

int close_device(gd_handle* h, const gd_key* ids, const uint32_t* pending_left, uint32_t n, int64_t now,
                 uint8_t* out_found) {
    if (n == 0) return GD_OK;
    GD_TRY(ensure(h, h->gw_scr[0], (size_t)n * 4));
    uint32_t* slot_of = (uint32_t*)h->gw_scr[0].p;
    const GwTab t = gw_tab(h, GW_CLIENTS);
    const dim3 grid(blocks_for(n, BLOCK)), block(BLOCK);
    GD_TRY(launch(h, "k_gw_find", grid, block, 0, k_gw_find, ids, n, t, slot_of, t.last));
    return launch(h, "k_gw_close_apply", grid, block, 0, k_gw_close_apply, pending_left, n, t, gw_clients(h), now,
                  (const uint32_t*)slot_of, out_found);
}

int drop_device(gd_handle* h, int64_t now, uint32_t cap, gd_key* out_id, uint32_t* out_handle, uint32_t* out_pending,
                uint32_t* n_out) {
    StageTime stage(h, "stage:gw_drop");
    const GwTab t = gw_tab(h, GW_CLIENTS);
    const unsigned long long slots = h->gw_cap[GW_CLIENTS];
    GD_TRY(ensure(h, h->gw_scr[2], ((size_t)slots + 1) * 4));
    uint32_t* pos = (uint32_t*)h->gw_scr[2].p;
    const dim3 grid(blocks_for(slots + 1, BLOCK)), block(BLOCK);
    GD_TRY(launch(h, "k_gw_drop_mark", grid, block, 0, k_gw_drop_mark, t, (const GwClient*)gw_clients(h), now,
                  h->gw_drop_timeout, pos));
    GD_TRY(scan_device<OpAdd>(h, pos, (uint32_t)(slots + 1), false, false, "gw_drop"));
    return launch(h, "k_gw_drop_emit", grid, block, 0, k_gw_drop_emit, t, (const GwClient*)gw_clients(h),
                  (const uint32_t*)pos, cap, out_id, out_handle, out_pending, n_out);
}

int routes_expire_device(gd_handle* h, int64_t now, uint32_t* n_removed) {
    const GwTab t = gw_tab(h, GW_ROUTES);
    HIP_TRY(h, hipMemsetAsync(n_removed, 0, 4, h->stream));
    return launch(h, "k_gw_routes_expire", dim3(blocks_for(h->gw_cap[GW_ROUTES], BLOCK)), dim3(BLOCK), 0,
                  k_gw_routes_expire, t, (const int64_t*)gw_times(h), now, h->gw_route_expiry, n_removed);
}

int lookup_device(gd_handle* h, const gd_key* ids, uint32_t n, const GwLookupOut& o) {
    return launch(h, "k_gw_lookup", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_gw_lookup, ids, n,
                  gw_tab(h, GW_CLIENTS), (const GwClient*)gw_clients(h), gw_tab(h, GW_ROUTES),
                  (const int64_t*)gw_times(h), h->gw_nsenders, o);
}

// perm / offsets of the bucket ids q over B buckets (ids past B - 1 in the last): the send stage's small-fan-out
// partition while its scatter's LDS fits a workgroup, else the general bucketing; both are stable.
int partition_device(gd_handle* h, const uint32_t* q, uint32_t n, uint32_t B, uint32_t* perm, uint32_t* offsets) {
    if (n == 0) return launch(h, "k_fill", dim3(blocks_for(B + 1, BLOCK)), dim3(BLOCK), 0, k_fill_u32, offsets, B + 1, 0u);
    if (sq_scatter_lds(B) > GW_LDS_MAX) return bucket_device(h, q, n, B - 1, perm, offsets);
    const uint32_t tiles = blocks_for(n, SQ_TILE);
    GD_TRY(ensure(h, h->gw_scr[3], ((size_t)B * tiles + B) * 4));
    uint32_t* hist = (uint32_t*)h->gw_scr[3].p;
    uint32_t* totals = hist + (size_t)B * tiles;
    uint32_t bits = 1;
    while ((1u << bits) < B) ++bits;
    GD_TRY(launch(h, "k_gw_hist", dim3(tiles), dim3(SQ_NT), (size_t)sq_pad4(B) * 4, k_gw_hist, q, n, B, tiles, hist));
    GD_TRY(launch(h, "k_radix_rowscan", dim3(B), dim3(BLOCK), 0, k_radix_rowscan, hist, tiles, totals));
    GD_TRY(launch(h, "k_sendq_offsets", dim3(1), dim3(SQ_NT), 0, k_sendq_offsets, (const uint32_t*)totals, B, n, offsets));
    return launch(h, "k_sendq_scatter", dim3(tiles), dim3(SQ_NT), sq_scatter_lds(B), k_sendq_scatter, q, n, B, bits,
                  tiles, (const uint32_t*)hist, (const uint32_t*)offsets, perm, h->lane_order ? h->radix_rank_atomic : 0u);
}

// TryDeliverToProxy for the batch and the routes it records; rs: gd_gateway_send_queues' route statuses.
int proxy_device(gd_handle* h, const gd_key* target, const gd_key* sending, const uint32_t* sending_silo,
                 const uint8_t* rs, const int64_t* ttl, uint32_t n, int64_t now, uint8_t* st, uint32_t* handle,
                 uint32_t* sender, bool sync_passes, const char* call) {
    if (sending) GD_TRY(gw_reserve(h, GW_ROUTES, n, call));
    uint32_t* slot_of = nullptr;
    uint8_t* is_new = nullptr;
    if (sending) {
        GD_TRY(ensure(h, h->gw_scr[0], (size_t)n * 4));
        GD_TRY(ensure(h, h->gw_scr[1], (size_t)n + 16));
        slot_of = (uint32_t*)h->gw_scr[0].p;
        is_new = (uint8_t*)h->gw_scr[1].p;
    }
    const dim3 grid(blocks_for(n, BLOCK)), block(BLOCK);
    GD_TRY(launch(h, "k_gw_deliver", grid, block, 0, k_gw_deliver, target, sending, rs, ttl, n, gw_tab(h, GW_CLIENTS),
                  gw_clients(h), h->gw_nsenders, st, handle, sender, slot_of));
    if (!sending) return GD_OK;
    const GwTab rt = gw_tab(h, GW_ROUTES);
    GD_TRY(gw_claims(h, GW_ROUTES, sending, n, slot_of, is_new, false, rt.last + h->gw_cap[GW_ROUTES], false, sync_passes,
                     call));
    return launch(h, "k_gw_route_apply", grid, block, 0, k_gw_route_apply, sending_silo, n, now, rt, gw_times(h),
                  (const uint32_t*)slot_of, (const uint8_t*)is_new);
}

int deliver_device(gd_handle* h, const gd_key* target, const gd_key* sending, const uint32_t* sending_silo,
                   const int64_t* ttl, uint32_t n, int64_t now, uint8_t* st, uint32_t* handle, uint32_t* sender,
                   uint32_t* perm, uint32_t* offsets, bool sync_passes, const char* call) {
    const uint32_t B = h->gw_nsenders + 1;
    if (n == 0) return offsets ? partition_device(h, nullptr, 0, B, perm, offsets) : GD_OK;
    StageTime stage(h, "stage:gw_deliver");
    if (!sender) {
        GD_TRY(ensure(h, h->gw_scr[4], (size_t)n * 4));
        sender = (uint32_t*)h->gw_scr[4].p;
    }
    GD_TRY(proxy_device(h, target, sending, sending_silo, nullptr, ttl, n, now, st, handle, sender, sync_passes, call));
    return perm ? partition_device(h, sender, n, B, perm, offsets) : GD_OK;
}

int gw_send_device(gd_handle* h, const gd_key* target, const gd_key* sending, const uint32_t* sending_silo,
                   const uint32_t* silo, const uint8_t* rs, const uint8_t* cat, const int64_t* ttl, uint32_t n,
                   int64_t now, uint8_t* st, uint32_t* q, uint32_t* handle, uint32_t* perm, uint32_t* offsets,
                   bool sync_passes, const char* call) {
    const uint32_t B = h->send_nq + 4 + h->gw_nsenders;
    if (n == 0) return offsets ? partition_device(h, nullptr, 0, B, perm, offsets) : GD_OK;
    StageTime stage(h, "stage:gw_send_queues");
    GD_TRY(ensure(h, h->gw_scr[4], (size_t)n * 4));
    GD_TRY(ensure(h, h->gw_scr[5], (size_t)n * 5 + 16));
    uint32_t* gw_sender = (uint32_t*)h->gw_scr[4].p;
    uint32_t* qs = (uint32_t*)h->gw_scr[5].p;             // the bucket ids when the caller wants none
    uint8_t* gw_st = (uint8_t*)(qs + n);
    if (!q) q = qs;
    GD_TRY(proxy_device(h, target, sending, sending_silo, rs, ttl, n, now, gw_st, handle, gw_sender, sync_passes, call));
    const bool tab_lds = (size_t)h->send_nsilos * 4 <= SQ_TAB_LDS_BYTES;
    const SendArgs a{(const uint32_t*)h->send_tab.p, h->send_nsilos, h->send_nq, h->cfg.my_silo, tab_lds ? 1u : 0u};
    const uint32_t tiles = blocks_for(n, SQ_TILE);
    GD_TRY(launch(h, "k_sendq_classify", dim3(tiles), dim3(SQ_NT), sq_classify_lds(h->send_nq + 4, h->send_nsilos, tab_lds),
                  k_sendq_classify, silo, rs, cat, ttl, n, a, tiles, st, q, (uint32_t*)nullptr));
    GD_TRY(launch(h, "k_gw_send_merge", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_gw_send_merge,
                  (const uint8_t*)gw_st, (const uint32_t*)gw_sender, n, h->send_nq, st, q));
    return perm ? partition_device(h, q, n, B, perm, offsets) : GD_OK;
}

int ingress_device(gd_handle* h, const gd_key* target, const gd_key* sending, const uint8_t* direction,
                   const int64_t* ttl, uint32_t n, int overloaded, uint8_t* st, uint32_t* silo, uint32_t* route_idx,
                   uint32_t* n_route, gd_key* route_keys) {
    if (n == 0) {
        if (n_route) HIP_TRY(h, hipMemsetAsync(n_route, 0, 4, h->stream));
        return GD_OK;
    }
    StageTime stage(h, "stage:gw_ingress");
    uint32_t* pos = nullptr;
    if (route_idx) {
        GD_TRY(ensure(h, h->gw_scr[2], ((size_t)n + 1) * 4));
        pos = (uint32_t*)h->gw_scr[2].p;
    }
    GD_TRY(launch(h, "k_gw_ingress", dim3(blocks_for((uint64_t)n + 1, BLOCK)), dim3(BLOCK), 0, k_gw_ingress, target,
                  sending, direction, ttl, n, overloaded ? 1u : 0u, gw_tab(h, GW_ROUTES), h->cfg.my_silo, st, silo, pos));
    if (!route_idx) return GD_OK;
    GD_TRY(scan_device<OpAdd>(h, pos, n + 1, false, false, "gw_ingress"));
    return launch(h, "k_gw_ingress_emit", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_gw_ingress_emit, target, n,
                  (const uint32_t*)pos, route_idx, n_route, route_keys);
}

int check_pairs(gd_handle* h, const char* call, const void* perm, const void* offsets) {
    if ((perm != nullptr) != (offsets != nullptr)) return set_err(h, GD_EINVAL, "%s: perm and offsets go together", call);
    return GD_OK;
}
int check_ingress(gd_handle* h, const char* call, const void* route_idx, const void* n_route, const void* route_keys) {
    if ((route_idx != nullptr) != (n_route != nullptr))
        return set_err(h, GD_EINVAL, "%s: route_idx and n_route go together", call);
    if (route_keys && !route_idx) return set_err(h, GD_EINVAL, "%s: route_keys needs route_idx and n_route", call);
    return GD_OK;
}
int check_send(gd_handle* h, const char* call) {
    if (!h->send_nq) return set_err(h, GD_ESTATE, "%s before gd_send_configure", call);
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_gateway_configure(gd_handle* h, uint32_t n_senders, int64_t client_drop_timeout, int64_t route_expiry,
                         uint64_t capacity_hint) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (n_senders < 1 || n_senders > GD_GW_MAX_SENDERS)
        return set_err(h, GD_EINVAL, "gd_gateway_configure: n_senders %u not in 1..%u", n_senders, GD_GW_MAX_SENDERS);
    if (client_drop_timeout < 0 || route_expiry < 0) return set_err(h, GD_EINVAL, "gd_gateway_configure: negative timeout");
    if (capacity_hint > GW_MAX_CAP) return set_err(h, GD_EINVAL, "gd_gateway_configure: capacity_hint > 2^31");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_gateway_configure"));
    unsigned long long cap = GW_MIN_CAP;
    while (cap < capacity_hint) cap <<= 1;
    if (!h->gw_nsenders) {
        GD_TRY(ensure(h, h->gw_state, sizeof(GwState)));
        HIP_TRY(h, hipMemsetAsync(h->gw_state.p, 0, sizeof(GwState), h->stream));
        for (int t = 0; t < 2; ++t) {
            GD_TRY(ensure(h, h->gw_ctr[t], CTR_BYTES));
            HIP_TRY(h, hipMemsetAsync(h->gw_ctr[t].p, 0, CTR_BYTES, h->stream));
            GD_TRY(gw_alloc(h, t, cap, h->gw_slots[t], h->gw_side[t], h->gw_last[t]));
            h->gw_cap[t] = cap;
            h->gw_used_ub[t] = 0;
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    } else {
        DevCounters c[2];
        for (int t = 0; t < 2; ++t) GD_TRY(gw_pull(h, t, &c[t], "gd_gateway_configure"));
        if (n_senders != h->gw_nsenders && c[GW_CLIENTS].live)
            return set_err(h, GD_EINVAL, "gd_gateway_configure: n_senders changes while %llu clients are present",
                           c[GW_CLIENTS].live);
        if (n_senders != h->gw_nsenders) HIP_TRY(h, hipMemsetAsync(&gw_state(h)->rr, 0, 4, h->stream));
        for (int t = 0; t < 2; ++t)
            if (cap > h->gw_cap[t]) {
                GD_TRY(gw_rebuild(h, t, cap));
                h->gw_used_ub[t] = c[t].live;
            }
    }
    h->gw_nsenders = n_senders;
    h->gw_drop_timeout = client_drop_timeout;
    h->gw_route_expiry = route_expiry;
    return GD_OK;
}

int gd_gateway_clear(gd_handle* h) {
    GD_TRY(check_handle(h, "gd_gateway_clear"));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_gateway_clear"));
    for (int t = 0; t < 2; ++t) {
        HIP_TRY(h, hipMemsetAsync(h->gw_slots[t].p, 0, (size_t)h->gw_cap[t] * sizeof(Slot), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->gw_last[t].p, 0, (size_t)h->gw_cap[t] * 8, h->stream));
        HIP_TRY(h, hipMemsetAsync(h->gw_ctr[t].p, 0, CTR_BYTES, h->stream));
        h->gw_used_ub[t] = 0;
    }
    HIP_TRY(h, hipMemsetAsync(h->gw_state.p, 0, sizeof(GwState), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_gateway_count(gd_handle* h, uint64_t* out_clients, uint64_t* out_routes, uint64_t* out_client_capacity,
                     uint64_t* out_route_capacity) {
    GD_TRY(check_handle(h, "gd_gateway_count"));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_gateway_count"));
    DevCounters c[2];
    for (int t = 0; t < 2; ++t) {
        GD_TRY(gw_pull(h, t, &c[t], "gd_gateway_count"));
        h->gw_used_ub[t] = c[t].live + c[t].tomb;
    }
    if (out_clients) *out_clients = c[GW_CLIENTS].live;
    if (out_routes) *out_routes = c[GW_ROUTES].live;
    if (out_client_capacity) *out_client_capacity = h->gw_cap[GW_CLIENTS];
    if (out_route_capacity) *out_route_capacity = h->gw_cap[GW_ROUTES];
    return GD_OK;
}

int gd_gateway_open_device(gd_handle* h, const gd_key* d_ids, const uint32_t* d_handles, uint32_t n,
                           uint32_t* d_out_handle, uint32_t* d_out_sender, uint8_t* d_out_new, uint32_t* d_out_pending) {
    GD_TRY(check_handle(h, "gd_gateway_open_device", n));
    if (n && (!d_ids || !d_handles)) return set_err(h, GD_EINVAL, "gd_gateway_open_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return open_device(h, d_ids, d_handles, n, GwOpenOut{d_out_handle, d_out_sender, d_out_pending, d_out_new}, false,
                       "gd_gateway_open_device");
}

int gd_gateway_open(gd_handle* h, const gd_key* ids, const uint32_t* handles, uint32_t n, uint32_t* out_handle,
                    uint32_t* out_sender, uint8_t* out_new, uint32_t* out_pending) {
    GD_TRY(check_handle(h, "gd_gateway_open", n));
    if (n && (!ids || !handles)) return set_err(h, GD_EINVAL, "gd_gateway_open: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_gateway_open"));
    HostStage io(h);
    const gd_key* di = io.in(ids, n);
    const uint32_t* dh = io.in(handles, n);
    GwOpenOut o{};
    o.handle = io.out_if(out_handle, n, 4);
    o.sender = io.out_if(out_sender, n, 4);
    o.is_new = io.out_if(out_new, n, 16);
    o.pending = io.out_if(out_pending, n, 4);
    GD_TRY(io.status());
    GD_TRY(open_device(h, di, dh, n, o, true, "gd_gateway_open"));
    GD_TRY(io.fetch());
    DevCounters c;
    return gw_pull(h, GW_CLIENTS, &c, "gd_gateway_open");
}

int gd_gateway_close_device(gd_handle* h, const gd_key* d_ids, const uint32_t* d_pending_left, uint32_t n, int64_t now,
                            uint8_t* d_out_found) {
    GD_TRY(check_handle(h, "gd_gateway_close_device", n));
    if (n && !d_ids) return set_err(h, GD_EINVAL, "gd_gateway_close_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return close_device(h, d_ids, d_pending_left, n, now, d_out_found);
}

int gd_gateway_close(gd_handle* h, const gd_key* ids, const uint32_t* pending_left, uint32_t n, int64_t now,
                     uint8_t* out_found) {
    GD_TRY(check_handle(h, "gd_gateway_close", n));
    if (n && !ids) return set_err(h, GD_EINVAL, "gd_gateway_close: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_gateway_close"));
    HostStage io(h);
    const gd_key* di = io.in(ids, n);
    const uint32_t* dp = io.in(pending_left, n);
    uint8_t* dfound = io.out_if(out_found, n, 16);
    GD_TRY(io.status());
    GD_TRY(close_device(h, di, dp, n, now, dfound));
    GD_TRY(io.fetch());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_gateway_drop_device(gd_handle* h, int64_t now, uint32_t cap, gd_key* d_out_id, uint32_t* d_out_handle,
                           uint32_t* d_out_pending, uint32_t* d_n_out) {
    GD_TRY(check_handle(h, "gd_gateway_drop_device"));
    if (!d_n_out || (cap && (!d_out_id || !d_out_handle || !d_out_pending)))
        return set_err(h, GD_EINVAL, "gd_gateway_drop_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return drop_device(h, now, cap, d_out_id, d_out_handle, d_out_pending, d_n_out);
}

int gd_gateway_drop(gd_handle* h, int64_t now, uint32_t cap, gd_key* out_id, uint32_t* out_handle,
                    uint32_t* out_pending, uint32_t* n_out) {
    GD_TRY(check_handle(h, "gd_gateway_drop"));
    if (!n_out || (cap && (!out_id || !out_handle || !out_pending)))
        return set_err(h, GD_EINVAL, "gd_gateway_drop: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_gateway_drop"));
    // a list never holds more than the table: outputs of that size stand in for a larger cap
    const uint32_t dcap = (uint32_t)std::min<uint64_t>(cap, h->gw_cap[GW_CLIENTS]);
    HostStage io(h);
    gd_key* did = io.hold<gd_key>(dcap, 8);
    uint32_t* dhandle = io.hold<uint32_t>(dcap, 4);
    uint32_t* dpending = io.hold<uint32_t>(dcap, 4);
    uint32_t* dn = io.hold<uint32_t>(1);
    GD_TRY(io.status());
    GD_TRY(drop_device(h, now, dcap, did, dhandle, dpending, dn));
    GD_TRY(read_back(h, dn, n_out, 1));
    if (*n_out > cap) return set_err(h, GD_EINVAL, "gd_gateway_drop: %u clients are due, cap is %u (nothing changed)", *n_out, cap);
    GD_TRY(io.fetch(out_id, did, *n_out));
    GD_TRY(io.fetch(out_handle, dhandle, *n_out));
    GD_TRY(io.fetch(out_pending, dpending, *n_out));
    DevCounters c;
    return gw_pull(h, GW_CLIENTS, &c, "gd_gateway_drop");
}

int gd_gateway_routes_expire_device(gd_handle* h, int64_t now, uint32_t* d_n_removed) {
    GD_TRY(check_handle(h, "gd_gateway_routes_expire_device"));
    if (!d_n_removed) return set_err(h, GD_EINVAL, "gd_gateway_routes_expire_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return routes_expire_device(h, now, d_n_removed);
}

int gd_gateway_routes_expire(gd_handle* h, int64_t now, uint32_t* n_removed) {
    GD_TRY(check_handle(h, "gd_gateway_routes_expire"));
    if (!n_removed) return set_err(h, GD_EINVAL, "gd_gateway_routes_expire: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_gateway_routes_expire"));
    HostStage io(h);
    uint32_t* dn = io.hold<uint32_t>(1);
    GD_TRY(io.status());
    GD_TRY(routes_expire_device(h, now, dn));
    return read_back(h, dn, n_removed, 1);
}

int gd_gateway_lookup_device(gd_handle* h, const gd_key* d_ids, uint32_t n, uint32_t* d_out_handle,
                             uint32_t* d_out_sender, uint8_t* d_out_connected, int64_t* d_out_since,
                             uint32_t* d_out_pending, uint8_t* d_out_found, uint32_t* d_out_route_silo,
                             int64_t* d_out_route_time, uint8_t* d_out_route_found) {
    GD_TRY(check_handle(h, "gd_gateway_lookup_device", n));
    if (n && !d_ids) return set_err(h, GD_EINVAL, "gd_gateway_lookup_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return lookup_device(h, d_ids, n,
                         GwLookupOut{d_out_handle, d_out_sender, d_out_connected, d_out_since, d_out_pending, d_out_found,
                                     d_out_route_silo, d_out_route_time, d_out_route_found});
}

int gd_gateway_lookup(gd_handle* h, const gd_key* ids, uint32_t n, uint32_t* out_handle, uint32_t* out_sender,
                      uint8_t* out_connected, int64_t* out_since, uint32_t* out_pending, uint8_t* out_found,
                      uint32_t* out_route_silo, int64_t* out_route_time, uint8_t* out_route_found) {
    GD_TRY(check_handle(h, "gd_gateway_lookup", n));
    if (n && !ids) return set_err(h, GD_EINVAL, "gd_gateway_lookup: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_gateway_lookup"));
    HostStage io(h);
    const gd_key* di = io.in(ids, n);
    GwLookupOut o{};
    o.handle = io.out_if(out_handle, n, 4);
    o.sender = io.out_if(out_sender, n, 4);
    o.connected = io.out_if(out_connected, n, 16);
    o.since = io.out_if(out_since, n, 8);
    o.pending = io.out_if(out_pending, n, 4);
    o.found = io.out_if(out_found, n, 16);
    o.route_silo = io.out_if(out_route_silo, n, 4);
    o.route_time = io.out_if(out_route_time, n, 8);
    o.route_found = io.out_if(out_route_found, n, 16);
    GD_TRY(io.status());
    GD_TRY(lookup_device(h, di, n, o));
    GD_TRY(io.fetch());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GD_OK;
}

int gd_gateway_deliver_device(gd_handle* h, const gd_key* d_target_grain, const gd_key* d_sending_grain,
                              const uint32_t* d_sending_silo, const int64_t* d_ttl, uint32_t n, int64_t now,
                              uint8_t* d_out_status, uint32_t* d_out_handle, uint32_t* d_out_sender, uint32_t* d_perm,
                              uint32_t* d_offsets) {
    GD_TRY(check_handle(h, "gd_gateway_deliver_device", n));
    GD_TRY(check_pairs(h, "gd_gateway_deliver_device", d_perm, d_offsets));
    if (n && (!d_target_grain || !d_out_status)) return set_err(h, GD_EINVAL, "gd_gateway_deliver_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return deliver_device(h, d_target_grain, d_sending_grain, d_sending_silo, d_ttl, n, now, d_out_status, d_out_handle,
                          d_out_sender, d_perm, d_offsets, false, "gd_gateway_deliver_device");
}

int gd_gateway_deliver(gd_handle* h, const gd_key* target_grain, const gd_key* sending_grain,
                       const uint32_t* sending_silo, const int64_t* ttl, uint32_t n, int64_t now, uint8_t* out_status,
                       uint32_t* out_handle, uint32_t* out_sender, uint32_t* out_perm, uint32_t* out_offsets) {
    GD_TRY(check_handle(h, "gd_gateway_deliver", n));
    GD_TRY(check_pairs(h, "gd_gateway_deliver", out_perm, out_offsets));
    if (n && (!target_grain || !out_status)) return set_err(h, GD_EINVAL, "gd_gateway_deliver: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_gateway_deliver"));
    HostStage io(h);
    const gd_key* dt = io.in(target_grain, n);
    const gd_key* ds = io.in(sending_grain, n);
    const uint32_t* dss = io.in(sending_silo, n);
    const int64_t* dttl = io.in(ttl, n);
    uint8_t* dst = io.out(out_status, n, 16);
    uint32_t* dhandle = io.out_if(out_handle, n, 4);
    uint32_t* dsender = io.out_if(out_sender, n, 4);
    uint32_t* dperm = io.out_if(out_perm, n, 4);
    uint32_t* doff = io.out_if(out_offsets, (size_t)h->gw_nsenders + 2);
    GD_TRY(io.status());
    GD_TRY(deliver_device(h, dt, ds, dss, dttl, n, now, dst, dhandle, dsender, dperm, doff, true, "gd_gateway_deliver"));
    GD_TRY(io.fetch());
    return gw_pull_both(h, "gd_gateway_deliver");
}

int gd_gateway_send_queues_device(gd_handle* h, const gd_key* d_target_grain, const gd_key* d_sending_grain,
                                  const uint32_t* d_sending_silo, const uint32_t* d_silo,
                                  const uint8_t* d_route_status, const uint8_t* d_category, const int64_t* d_ttl,
                                  uint32_t n, int64_t now, uint8_t* d_send_status, uint32_t* d_queue,
                                  uint32_t* d_out_handle, uint32_t* d_perm, uint32_t* d_offsets) {
    GD_TRY(check_handle(h, "gd_gateway_send_queues_device", n));
    GD_TRY(check_send(h, "gd_gateway_send_queues_device"));
    GD_TRY(check_pairs(h, "gd_gateway_send_queues_device", d_perm, d_offsets));
    if (n && (!d_target_grain || !d_silo || !d_send_status))
        return set_err(h, GD_EINVAL, "gd_gateway_send_queues_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return gw_send_device(h, d_target_grain, d_sending_grain, d_sending_silo, d_silo, d_route_status, d_category, d_ttl, n,
                          now, d_send_status, d_queue, d_out_handle, d_perm, d_offsets, false,
                          "gd_gateway_send_queues_device");
}

int gd_gateway_send_queues(gd_handle* h, const gd_key* target_grain, const gd_key* sending_grain,
                           const uint32_t* sending_silo, const uint32_t* silo, const uint8_t* route_status,
                           const uint8_t* category, const int64_t* ttl, uint32_t n, int64_t now,
                           uint8_t* out_send_status, uint32_t* out_queue, uint32_t* out_handle, uint32_t* out_perm,
                           uint32_t* out_offsets) {
    GD_TRY(check_handle(h, "gd_gateway_send_queues", n));
    GD_TRY(check_send(h, "gd_gateway_send_queues"));
    GD_TRY(check_pairs(h, "gd_gateway_send_queues", out_perm, out_offsets));
    if (n && (!target_grain || !silo || !out_send_status))
        return set_err(h, GD_EINVAL, "gd_gateway_send_queues: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_gateway_send_queues"));
    HostStage io(h);
    const gd_key* dt = io.in(target_grain, n);
    const gd_key* ds = io.in(sending_grain, n);
    const uint32_t* dss = io.in(sending_silo, n);
    const uint32_t* dsilo = io.in(silo, n);
    const uint8_t* drs = io.in(route_status, n);
    const uint8_t* dcat = io.in(category, n);
    const int64_t* dttl = io.in(ttl, n);
    uint8_t* dst = io.out(out_send_status, n, 16);
    uint32_t* dq = io.out_if(out_queue, n, 4);
    uint32_t* dhandle = io.out_if(out_handle, n, 4);
    uint32_t* dperm = io.out_if(out_perm, n, 4);
    uint32_t* doff = io.out_if(out_offsets, (size_t)h->send_nq + h->gw_nsenders + 5);
    GD_TRY(io.status());
    GD_TRY(gw_send_device(h, dt, ds, dss, dsilo, drs, dcat, dttl, n, now, dst, dq, dhandle, dperm, doff, true,
                          "gd_gateway_send_queues"));
    GD_TRY(io.fetch());
    return gw_pull_both(h, "gd_gateway_send_queues");
}

int gd_gateway_ingress_device(gd_handle* h, const gd_key* d_target_grain, const gd_key* d_sending_grain,
                              const uint8_t* d_direction, const int64_t* d_ttl, uint32_t n, int overloaded,
                              uint8_t* d_out_status, uint32_t* d_out_silo, uint32_t* d_route_idx, uint32_t* d_n_route,
                              gd_key* d_route_keys) {
    GD_TRY(check_handle(h, "gd_gateway_ingress_device", n));
    GD_TRY(check_ingress(h, "gd_gateway_ingress_device", d_route_idx, d_n_route, d_route_keys));
    if (n && (!d_target_grain || !d_out_status)) return set_err(h, GD_EINVAL, "gd_gateway_ingress_device: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return ingress_device(h, d_target_grain, d_sending_grain, d_direction, d_ttl, n, overloaded, d_out_status, d_out_silo,
                          d_route_idx, d_n_route, d_route_keys);
}

int gd_gateway_ingress(gd_handle* h, const gd_key* target_grain, const gd_key* sending_grain, const uint8_t* direction,
                       const int64_t* ttl, uint32_t n, int overloaded, uint8_t* out_status, uint32_t* out_silo,
                       uint32_t* route_idx, uint32_t* n_route, gd_key* route_keys) {
    GD_TRY(check_handle(h, "gd_gateway_ingress", n));
    GD_TRY(check_ingress(h, "gd_gateway_ingress", route_idx, n_route, route_keys));
    if (n && (!target_grain || !out_status)) return set_err(h, GD_EINVAL, "gd_gateway_ingress: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_gateway_ingress"));
    HostStage io(h);
    const gd_key* dt = io.in(target_grain, n);
    const gd_key* ds = io.in(sending_grain, n);
    const uint8_t* dd = io.in(direction, n);
    const int64_t* dttl = io.in(ttl, n);
    uint8_t* dst = io.out(out_status, n, 16);
    uint32_t* dsilo = io.out_if(out_silo, n, 4);
    // the whole lists come down (n entries at most); the host reads the first *n_route
    uint32_t* didx = io.out_if(route_idx, n, 4);
    uint32_t* dn = io.out_if(n_route, 1);
    gd_key* dkeys = io.out_if(route_keys, n, 8);
    GD_TRY(io.status());
    GD_TRY(ingress_device(h, dt, ds, dd, dttl, n, overloaded, dst, dsilo, didx, dn, dkeys));
    GD_TRY(io.fetch());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GD_OK;
}

}  // extern "C"
