// gd_gateway.h -- gfx950 device code of the gateway stage: Gateway.clients and
// ClientsReplyRoutingCache.clientRoutes (Messaging/Gateway.cs:265-306, 340-383) as two open-addressing tables in
// HBM; RecordOpenedSocket / RecordClosedSocket (:117-169), DropDisconnectedClients (:182-222), DropExpiredEntries
// (:369-382), TryDeliverToProxy (:229-250) with GatewaySender.Process's decision (:401-475), and
// GatewayAcceptor.HandleMessage (GatewayAcceptor.cs:88-141) for a batch.
//
// The tables.  Both are keyed by a 24-B GrainId of category Client, so both are the directory's 32-B Slot
// (gd_common.h) with its home (home_slot of the Jenkins hash), its states, its claim and its election words:
// gd_dirbatch.h's claim_walk and rehash_place over DirSlots, the directory's own policy (reg_claim_item with no
// IsValidSilo values).  What does not fit the slot lies beside it, slot for slot:
//   clients   act = the ClientState handle, meta's low 16 bits = GatewaySenderNumber (< 1,024);
//             GwClient {DisconnectedSince i64, PendingToSend.Count u32, connected u32}: one 16-B load
//   routes    act = the gateway silo index (GD_NO_SILO allowed); the recorded tick, i64
// A lookup (find_slot, gd_probe.h) walks from the home with whole-slot loads (two 16-B loads a slot) for at most
// DevCounters::max_probe + 1 slots; EMPTY ends a chain, TOMB keeps it going.  Two election words a slot, zero
// between calls: word 0 in ~i (first wins; it also names a fresh claim's claimer to the launch's other items),
// word 1 in 1 + i (last wins).
//
// Launches:
//   open           k_gw_claim pass 0 (Client keys only; every item that ends on a slot votes ~i), passes 1..
//                  (read-back driven, or GW_PASSES - 1 gated ones), k_gw_open_mark, scan_device (the new ids'
//                  round-robin ranks), k_gw_open_commit (the first item of each slot: insert or reconnect),
//                  k_gw_open_report (the others' outputs, next_round_robin, the words cleared)
//   close          k_gw_find (votes ~i), k_gw_close_apply
//   drop           k_gw_drop_mark, scan_device, k_gw_drop_emit (applies only if the count fits `cap`)
//   routes_expire  k_gw_routes_expire
//   lookup         k_gw_lookup
//   deliver        k_gw_deliver (statuses, pending += 1 by atomicAdd, which messages record a route),
//                  k_gw_claim passes over the sending grains (each settled item votes 1 + i on word 1),
//                  k_gw_route_apply (the last item of each slot writes silo, tick, LIVE), [k_gw_hist,
//                  k_radix_rowscan, k_sendq_offsets, k_sendq_scatter: the send stage's partition over the sender
//                  numbers as bucket ids]
//   send_queues    k_gw_deliver (held messages skipped), the route passes, k_sendq_classify (no counts),
//                  k_gw_send_merge, the partition over n_queues + 4 + n_senders buckets
//   ingress        k_gw_ingress, [scan_device, k_gw_ingress_emit]
//   rebuild        k_gw_rehash into a zeroed table
// No kernel waits on another lane's progress: an item that meets a claim not yet recorded defers to the next pass
// (SLOT_RETRY), and a device form whose GW_PASSES passes did not settle flags ERR_UNSETTLED.  Every store is a plain
// vector store or a device-scope atomic.  One item a thread, 256 threads (the neighbouring kernels' shape;
// alternatives were not measured).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "gd_common.h"
#include "gd_dirbatch.h"
#include "gd_hash.h"
#include "gd_scan.h"
#include "gd_sendq.h"
#include "graindispatch.h"

namespace gd {

constexpr uint32_t CAT_CLIENT = 4;               // UniqueKey.Category.Client (UniqueKey.cs:23)
constexpr uint32_t GW_PASSES = REG_PASSES;       // claim passes of the device forms
constexpr uint32_t GW_ERR_FULL = 2u;             // DevCounters::err (claim_walk's bit)

struct alignas(16) GwClient {
    int64_t since;          // DisconnectedSince in ticks; INT64_MAX while connected
    uint32_t pending;       // PendingToSend.Count
    uint32_t connected;     // Socket != null
};
static_assert(sizeof(GwClient) == 16, "client value must be 16 bytes");

struct GwState {
    uint32_t rr;                      // nextGatewaySenderToUseForRoundRobin, kept modulo n_senders
    uint32_t pad[3];
    uint32_t retry[2][GW_PASSES];     // items pass p deferred: [0] open's claims, [1] the route upserts'
};

struct GwTab {
    Slot* slots;
    unsigned long long mask;
    DevCounters* ctr;
    uint32_t* last;                   // [2][mask + 1] election words
};
__device__ __forceinline__ uint32_t* gw_win(const GwTab& t) { return t.last + (t.mask + 1ull); }

GD_HD uint32_t gw_cat(uint64_t tcd) { return (uint32_t)(tcd >> 56); }
// GrainId.IsClient (GrainId.cs:23): Client or GeoClient
GD_HD bool gw_is_client(uint32_t cat) { return cat == CAT_CLIENT || cat == CAT_GEO_CLIENT; }

// ------------------------------------------------------------------ claims (open, the route upsert)
// A claim pass.  init (open's pass 0): every key of category Client runs, the others get NONE32; else the items
// whose slot_of is SLOT_RETRY run (deliver marked them, or the previous pass deferred them).  gate (nullable): the
// previous pass's deferred count; retry: this pass's.  A settled item votes ~i on word 0 when its entry is the
// batch's (elect_all: always) and 1 + i on word 1 when `win` is given.
static __global__ void __launch_bounds__(BLOCK) k_gw_claim(const gd_key* __restrict__ keys, uint32_t n, GwTab t,
                                                    uint32_t* __restrict__ slot_of, uint8_t* __restrict__ is_new,
                                                    uint32_t pass, uint32_t init, const uint32_t* __restrict__ gate,
                                                    uint32_t* retry, uint32_t* __restrict__ win, uint32_t elect_all) {
    if (gate && *gate == 0) return;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pd = 0;
    bool reused = false;
    if (i < n) {
        bool run;
        if (init) {
            run = gw_cat(keys[i].type_code_data) == CAT_CLIENT;
            if (!run) {
                slot_of[i] = NONE32;
                is_new[i] = 0;
            }
        } else {
            run = slot_of[i] == SLOT_RETRY;
        }
        if (run) {
            reg_claim_item(i, keys, t.slots, t.mask, t.ctr, slot_of, is_new, nullptr, TableArgs{}, retry, pd, reused,
                           claim_tag(pass), t.last);
            const uint32_t s = slot_of[i];
            if (s < SLOT_RETRY) {
                if (is_new[i] || elect_all) atomicMax(&t.last[s], ~i);
                if (win) atomicMax(&win[s], i + 1u);
            }
        }
    }
    claim_counters(t.ctr, pd, reused);
}

// The device forms' last gated pass left items deferred: the batch is flagged.
static __global__ void __launch_bounds__(WAVE) k_gw_settled(DevCounters* ctr, const uint32_t* __restrict__ unsettled) {
    if (threadIdx.x == 0 && *unsettled) atomicOr(&ctr->err, ERR_UNSETTLED);
}

// ------------------------------------------------------------------ open
// flag[i] = item i inserts a new client (the first item of a slot this batch claimed); flag[n] = 0 (the scan's
// total lands there).
static __global__ void __launch_bounds__(BLOCK) k_gw_open_mark(uint32_t n, const uint32_t* __restrict__ slot_of,
                                                        const uint8_t* __restrict__ is_new,
                                                        const uint32_t* __restrict__ last,
                                                        uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > n) return;
    uint32_t f = 0;
    if (i < n) {
        const uint32_t s = slot_of[i];
        f = s < SLOT_RETRY && is_new[i] && last[s] == ~i ? 1u : 0u;
    }
    flag[i] = f;
}

struct GwOpenOut {
    uint32_t *handle, *sender, *pending;     // each nullable
    uint8_t* is_new;
};

// The first item of each slot: RecordOpenedSocket's insert (Gateway.cs:136-139) or reconnect (:123-133), then
// RecordConnection (:142).  pos = the exclusive scan of k_gw_open_mark's flags: the new ids' ranks.
static __global__ void __launch_bounds__(BLOCK) k_gw_open_commit(const uint32_t* __restrict__ handles, uint32_t n,
                                                          GwTab t, GwClient* __restrict__ side,
                                                          const GwState* __restrict__ state, uint32_t n_senders,
                                                          const uint32_t* __restrict__ slot_of,
                                                          const uint8_t* __restrict__ is_new,
                                                          const uint32_t* __restrict__ pos, GwOpenOut o) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool fresh = false;
    if (i < n) {
        const uint32_t s = slot_of[i];
        if (s < SLOT_RETRY && t.last[s] == ~i) {
            Slot& sl = t.slots[s];
            uint32_t handle, sender, pending = 0;
            if (is_new[i]) {
                handle = handles[i];
                sender = (uint32_t)(((uint64_t)state->rr + pos[i]) % n_senders);
                sl.act = handle;
                sl.meta = make_meta(SLOT_LIVE, sender);
                fresh = true;
            } else {
                handle = sl.act;
                sender = slot_silo(sl.meta);
                pending = side[s].pending;             // the drain QueueRequest(clientState, null) triggers
            }
            side[s] = GwClient{INT64_MAX, 0u, 1u};
            if (o.handle) o.handle[i] = handle;
            if (o.sender) o.sender[i] = sender;
            if (o.pending) o.pending[i] = pending;
            if (o.is_new) o.is_new[i] = fresh ? 1 : 0;
        }
    }
    live_delta(t.ctr, fresh, false);
}

// Every other item: a later item of a slot reads what the first left; a key that is no Client (or found no room)
// is reported untouched.  The first items clear their words; next_round_robin advances by the new ids.
static __global__ void __launch_bounds__(BLOCK) k_gw_open_report(uint32_t n, GwTab t, GwState* __restrict__ state,
                                                          uint32_t n_senders, const uint32_t* __restrict__ slot_of,
                                                          const uint32_t* __restrict__ pos, GwOpenOut o) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0) state->rr = (uint32_t)(((uint64_t)state->rr + pos[n]) % n_senders);
    if (i >= n) return;
    const uint32_t s = slot_of[i];
    uint32_t handle = NONE32, sender = n_senders;
    uint8_t nw = GD_GW_NOT_CLIENT;
    if (s < SLOT_RETRY) {
        if (t.last[s] == ~i) {                           // the others read ~i or 0: never their own
            t.last[s] = 0;
            return;
        }
        handle = t.slots[s].act;
        sender = slot_silo(t.slots[s].meta);
        nw = 0;
    }
    if (o.handle) o.handle[i] = handle;
    if (o.sender) o.sender[i] = sender;
    if (o.pending) o.pending[i] = 0u;
    if (o.is_new) o.is_new[i] = nw;
}

// ------------------------------------------------------------------ close
// Slot of each Client key, NONE32 if absent; vote (nullable): the first item of each slot, atomicMax(~i).
static __global__ void __launch_bounds__(BLOCK) k_gw_find(const gd_key* __restrict__ keys, uint32_t n, GwTab t,
                                                   uint32_t* __restrict__ slot_of, uint32_t* __restrict__ vote) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t tcd = keys[i].type_code_data;
    uint32_t s = NONE32;
    uint4 b;
    if (gw_cat(tcd) == CAT_CLIENT) s = find_slot(t.slots, t.mask, t.ctr->max_probe, keys[i].n0, keys[i].n1, tcd, b);
    slot_of[i] = s;
    if (vote && s != NONE32) atomicMax(&vote[s], ~i);
}

// RecordDisconnection (Gateway.cs:286-293) by the first item of each slot; the later ones find Socket == null.
static __global__ void __launch_bounds__(BLOCK) k_gw_close_apply(const uint32_t* __restrict__ pending_left, uint32_t n,
                                                          GwTab t, GwClient* __restrict__ side, int64_t now,
                                                          const uint32_t* __restrict__ slot_of,
                                                          uint8_t* __restrict__ out_found) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slot_of[i];
    if (s != NONE32 && t.last[s] == ~i) {
        t.last[s] = 0;
        GwClient c = side[s];
        if (c.connected) {
            c.connected = 0;
            c.since = now;
            if (pending_left) c.pending = pending_left[i];
            side[s] = c;
        }
    }
    if (out_found) out_found[i] = s != NONE32 ? 1 : 0;
}

// ------------------------------------------------------------------ drop, routes_expire
// flag[j] = the client in slot j is ReadyToDrop (Gateway.cs:301-305); flag[cap] = 0.
static __global__ void __launch_bounds__(BLOCK) k_gw_drop_mark(GwTab t, const GwClient* __restrict__ side, int64_t now,
                                                        int64_t timeout, uint32_t* __restrict__ flag) {
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j > t.mask + 1ull) return;
    uint32_t f = 0;
    if (j <= t.mask && slot_state(t.slots[j].meta) == SLOT_LIVE) {
        const GwClient c = side[j];
        f = !c.connected && now - c.since >= timeout ? 1u : 0u;
    }
    flag[j] = f;
}
// pos: the exclusive scan of the flags.  *n_out = the due clients; they are removed and listed only if they fit `cap`.
static __global__ void __launch_bounds__(BLOCK) k_gw_drop_emit(GwTab t, const GwClient* __restrict__ side,
                                                        const uint32_t* __restrict__ pos, uint32_t cap,
                                                        gd_key* __restrict__ out_id, uint32_t* __restrict__ out_handle,
                                                        uint32_t* __restrict__ out_pending,
                                                        uint32_t* __restrict__ n_out) {
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t total = pos[t.mask + 1ull];
    if (j == 0) *n_out = total;
    bool removed = false;
    if (total <= cap && j <= t.mask && pos[j + 1] != pos[j]) {
        Slot& sl = t.slots[j];
        const uint32_t p = pos[j];
        out_id[p] = gd_key{sl.n0, sl.n1, sl.tcd};
        out_handle[p] = sl.act;
        out_pending[p] = side[j].pending;
        sl.meta = make_meta(SLOT_TOMB, 0);
        removed = true;
    }
    live_delta(t.ctr, removed, true);
}

// DropExpiredEntries (Gateway.cs:369-382); *n_removed (zeroed by the host) counts a wave at a time.
static __global__ void __launch_bounds__(BLOCK) k_gw_routes_expire(GwTab t, const int64_t* __restrict__ time,
                                                            int64_t now, int64_t expiry,
                                                            uint32_t* __restrict__ n_removed) {
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    bool removed = false;
    if (j <= t.mask && slot_state(t.slots[j].meta) == SLOT_LIVE && now - time[j] >= expiry) {
        t.slots[j].meta = make_meta(SLOT_TOMB, 0);
        removed = true;
    }
    const unsigned long long m = __ballot(removed);
    if ((threadIdx.x & (WAVE - 1)) == 0 && m) atomicAdd(n_removed, (uint32_t)__popcll(m));
    live_delta(t.ctr, removed, true);
}

// ------------------------------------------------------------------ lookup
struct GwLookupOut {
    uint32_t *handle, *sender;
    uint8_t* connected;
    int64_t* since;
    uint32_t* pending;
    uint8_t* found;
    uint32_t* route_silo;
    int64_t* route_time;
    uint8_t* route_found;
};
static __global__ void __launch_bounds__(BLOCK) k_gw_lookup(const gd_key* __restrict__ keys, uint32_t n, GwTab ct,
                                                     const GwClient* __restrict__ cside, GwTab rt,
                                                     const int64_t* __restrict__ rtime, uint32_t n_senders,
                                                     GwLookupOut o) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t n0 = keys[i].n0, n1 = keys[i].n1, tcd = keys[i].type_code_data;
    const bool client = gw_cat(tcd) == CAT_CLIENT;
    if (o.handle || o.sender || o.connected || o.since || o.pending || o.found) {
        uint4 b;
        const uint32_t s = client ? find_slot(ct.slots, ct.mask, ct.ctr->max_probe, n0, n1, tcd, b) : NONE32;
        GwClient c{0, 0u, 0u};
        if (s != NONE32) c = cside[s];
        if (o.handle) o.handle[i] = s != NONE32 ? b.z : NONE32;
        if (o.sender) o.sender[i] = s != NONE32 ? slot_silo(b.w) : n_senders;
        if (o.connected) o.connected[i] = c.connected ? 1 : 0;
        if (o.since) o.since[i] = c.since;
        if (o.pending) o.pending[i] = c.pending;
        if (o.found) o.found[i] = s != NONE32 ? 1 : 0;
    }
    if (o.route_silo || o.route_time || o.route_found) {
        uint4 b;
        const uint32_t s = client ? find_slot(rt.slots, rt.mask, rt.ctr->max_probe, n0, n1, tcd, b) : NONE32;
        if (o.route_silo) o.route_silo[i] = s != NONE32 ? b.z : NONE32;
        if (o.route_time) o.route_time[i] = s != NONE32 ? rtime[s] : 0;
        if (o.route_found) o.route_found[i] = s != NONE32 ? 1 : 0;
    }
}

// ------------------------------------------------------------------ deliver
// One lane a message: OutboundMessageQueue.cs:65 (expiry) then TryDeliverToProxy (Gateway.cs:229-250) and
// GatewaySender.Process's connected test (:418-429).  The target's TypeCodeData word is read first: a target that
// is no Client ends there, its other 16 B unread and the table untouched.  rs (gd_gateway_send_queues only): a held
// message is decided before the proxy check.  want (nullable, with sending): SLOT_RETRY for a message that records
// a route, else NONE32 -- the route passes' slot_of.
static __global__ void __launch_bounds__(BLOCK) k_gw_deliver(const gd_key* __restrict__ target,
                                                      const gd_key* __restrict__ sending,
                                                      const uint8_t* __restrict__ rs,
                                                      const int64_t* __restrict__ ttl, uint32_t n, GwTab ct,
                                                      GwClient* __restrict__ cside, uint32_t n_senders,
                                                      uint8_t* __restrict__ out_status,
                                                      uint32_t* __restrict__ out_handle,
                                                      uint32_t* __restrict__ out_sender, uint32_t* __restrict__ want) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t st = GD_GW_NOT_PROXIED, handle = NONE32, sender = n_senders;
    bool route = false;
    const uint32_t r = rs ? (uint32_t)rs[i] : (uint32_t)GD_ROUTE_OK;
    const int64_t tl = ttl ? ttl[i] : GD_TTL_NONE;
    if (r != GD_ROUTE_OK && r != GD_ROUTE_SYSTEM_TARGET && r != GD_ROUTE_MEMBERSHIP) {
        // held: the send stage decides it
    } else if (tl != GD_TTL_NONE && tl <= 0) {
        st = GD_GW_EXPIRED;
    } else {
        const uint64_t tcd = target[i].type_code_data;
        const uint32_t cat = gw_cat(tcd);
        if (cat == CAT_GEO_CLIENT) {
            st = GD_GW_GEO_CLIENT;
        } else if (cat == CAT_CLIENT) {
            uint4 b;
            const uint32_t s = find_slot(ct.slots, ct.mask, ct.ctr->max_probe, target[i].n0, target[i].n1, tcd, b);
            if (s != NONE32) {
                handle = b.z;
                sender = slot_silo(b.w);
                if (cside[s].connected) {
                    st = GD_GW_SEND;
                } else {
                    st = GD_GW_PENDING;
                    atomicAdd(&cside[s].pending, 1u);        // integer adds: the count is order-free
                }
                route = sending && gw_cat(sending[i].type_code_data) == CAT_CLIENT;
            }
        }
    }
    out_status[i] = (uint8_t)st;
    if (out_handle) out_handle[i] = handle;
    out_sender[i] = sender;
    if (want) want[i] = route ? SLOT_RETRY : NONE32;
}

// RecordClientRoute's AddOrUpdate (Gateway.cs:352-356): the last item of each slot (word 1 holds 1 + its index)
// writes the gateway and the tick, publishes the entry and clears both words.
static __global__ void __launch_bounds__(BLOCK) k_gw_route_apply(const uint32_t* __restrict__ sending_silo, uint32_t n,
                                                          int64_t now, GwTab rt, int64_t* __restrict__ rtime,
                                                          const uint32_t* __restrict__ slot_of,
                                                          const uint8_t* __restrict__ is_new) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool fresh = false;
    if (i < n) {
        const uint32_t s = slot_of[i];
        uint32_t* win = gw_win(rt);
        if (s < SLOT_RETRY && win[s] == i + 1u) {
            win[s] = 0;                                      // the others read 1 + i or 0: never their own
            rt.last[s] = 0;
            rt.slots[s].act = sending_silo ? sending_silo[i] : NONE32;
            rtime[s] = now;
            rt.slots[s].meta = make_meta(SLOT_LIVE, 0);
            fresh = is_new[i] != 0;
        }
    }
    live_delta(rt.ctr, fresh, false);
}

// Per-tile counts of bucket ids already made (k_sendq_classify counts while it classifies): hist[d * tiles + tile],
// the layout k_radix_rowscan and k_sendq_scatter take.  Ids past B - 1 count in the last bucket, as the scatter
// clamps them.
static __global__ void __launch_bounds__(SQ_NT) k_gw_hist(const uint32_t* __restrict__ q, uint32_t n, uint32_t B,
                                                   uint32_t tiles, uint32_t* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_gwcnt[];
    for (uint32_t d = threadIdx.x; d < B; d += SQ_NT) s_gwcnt[d] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * SQ_TILE, lane = lane_id();
#pragma unroll 4
    for (int r = 0; r < SQ_IT; ++r) {
        const uint32_t i = base + r * SQ_NT + threadIdx.x;
        const bool valid = i < n;
        const uint32_t d = valid ? min(q[i], B - 1u) : 0u;
        // the lanes sharing the first valid lane's bucket (every lane, with one hot sender) take one add
        const unsigned long long live = __ballot(valid);
        const uint32_t lead = live ? (uint32_t)__ffsll((long long)live) - 1u : 0u;
        const uint32_t hd = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)lead);
        const unsigned long long hot = __ballot(valid && d == hd);
        if (valid) {
            if (d != hd) atomicAdd(&s_gwcnt[d], 1u);
            else if (lane == lead) atomicAdd(&s_gwcnt[d], (uint32_t)__popcll(hot));
        }
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < B; d += SQ_NT) hist[(size_t)d * tiles + blockIdx.x] = s_gwcnt[d];
}

// gd_gateway_send_queues: a proxied message (OutboundMessageQueue.cs:77 returns) takes GD_SEND_PROXIED and the
// bucket n_queues + 4 + its sender number over what k_sendq_classify decided without the proxy check.
static __global__ void __launch_bounds__(BLOCK) k_gw_send_merge(const uint8_t* __restrict__ gw_status,
                                                         const uint32_t* __restrict__ gw_sender, uint32_t n,
                                                         uint32_t n_queues, uint8_t* __restrict__ send_status,
                                                         uint32_t* __restrict__ queue) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = gw_status[i];
    if (g == GD_GW_SEND || g == GD_GW_PENDING) {
        send_status[i] = (uint8_t)GD_SEND_PROXIED;
        queue[i] = n_queues + 4u + gw_sender[i];
    }
}

// ------------------------------------------------------------------ ingress
// GatewayAcceptor.HandleMessage (GatewayAcceptor.cs:88-141) with Gateway.TryToReroute (Gateway.cs:171-180).
// flag (nullable): flag[i] = the message reroutes through gd_route*; flag[n] = 0.
static __global__ void __launch_bounds__(BLOCK) k_gw_ingress(const gd_key* __restrict__ target,
                                                      const gd_key* __restrict__ sending,
                                                      const uint8_t* __restrict__ direction,
                                                      const int64_t* __restrict__ ttl, uint32_t n, uint32_t overloaded,
                                                      GwTab rt, uint32_t my_silo, uint8_t* __restrict__ out_status,
                                                      uint32_t* __restrict__ out_silo, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        if (flag) flag[n] = 0;
        return;
    }
    uint32_t st, silo = NONE32;
    const int64_t tl = ttl ? ttl[i] : GD_TTL_NONE;
    if (tl != GD_TTL_NONE && tl <= 0) {
        st = GD_GWIN_EXPIRED;
    } else if (overloaded) {
        st = GD_GWIN_TOO_BUSY;
    } else {
        const uint64_t tcd = target[i].type_code_data;
        const uint32_t tc = gw_cat(tcd);
        uint32_t d = direction ? (uint32_t)direction[i] : 0u;
        if (d == 0xFFu) d = 0u;                              // header absent: Request (Message.cs:113-116)
        const bool both = d == 1u && gw_is_client(tc) && sending && gw_is_client(gw_cat(sending[i].type_code_data));
        st = tc == CAT_SYSTEM_TARGET ? GD_GWIN_SYSTEM_TARGET : GD_GWIN_REROUTE;
        if (both && tc == CAT_GEO_CLIENT) {
            st = GD_GWIN_GEO_CLIENT;
        } else if (both) {
            uint4 b;
            const uint32_t s = find_slot(rt.slots, rt.mask, rt.ctr->max_probe, target[i].n0, target[i].n1, tcd, b);
            if (s != NONE32 && b.z != NONE32) {              // a route with no gateway reroutes
                st = GD_GWIN_DIRECT;
                silo = b.z;
            }
        }
        if (st == GD_GWIN_SYSTEM_TARGET) silo = my_silo;
    }
    out_status[i] = (uint8_t)st;
    if (out_silo) out_silo[i] = silo;
    if (flag) flag[i] = st == GD_GWIN_REROUTE ? 1u : 0u;
}
// pos: the exclusive scan of the flags: the REROUTE messages in array order, and their keys.
static __global__ void __launch_bounds__(BLOCK) k_gw_ingress_emit(const gd_key* __restrict__ target, uint32_t n,
                                                           const uint32_t* __restrict__ pos,
                                                           uint32_t* __restrict__ route_idx,
                                                           uint32_t* __restrict__ n_route,
                                                           gd_key* __restrict__ route_keys) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0) *n_route = pos[n];
    if (i >= n) return;
    const uint32_t p = pos[i];
    if (pos[i + 1] == p) return;
    route_idx[p] = i;
    if (route_keys) route_keys[p] = target[i];
}

// ------------------------------------------------------------------ rebuild
// Every live entry of the old table, with its value, into the new, zeroed one (k_rehash with the value beside
// the slot).
template <typename T>
static __global__ void __launch_bounds__(BLOCK) k_gw_rehash(const Slot* __restrict__ old_slots,
                                                     const T* __restrict__ old_side, unsigned long long old_cap,
                                                     Slot* slots, T* __restrict__ side, unsigned long long mask,
                                                     DevCounters* ctr) {
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t pd = 0;
    bool placed = false;
    const Slot sl = j < old_cap ? old_slots[j] : Slot{};
    if (j < old_cap && slot_state(sl.meta) == SLOT_LIVE) {
        const DirSlots t{slots, mask};
        const uint32_t d = rehash_place(t, gd_key{sl.n0, sl.n1, sl.tcd}, sl.meta, [&](unsigned long long s) {
            slots[s].act = sl.act;
            side[s] = old_side[j];
        });
        placed = d != NONE32;
        if (placed) pd = d;
        else atomicOr(&ctr->err, GW_ERR_FULL);
    }
    claim_counters(ctr, pd, false);
    live_delta(ctr, placed, false);
}

}  // namespace gd
