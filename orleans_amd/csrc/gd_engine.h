// gd_engine.h -- libgraindispatch's engine-internal header: the handle, the launch / scratch helpers and
// the functions the engine's translation units share (eng_*.hip).  Not part of the ABI (include/
// graindispatch.h is).  Every kernel header is included here; their non-template kernels are static, so
// each translation unit keeps its own copies.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <queue>
#include <map>
#include <unordered_map>
#include <string>
#include <type_traits>
#include <vector>

#include "gd_common.h"
#include "gd_churn.h"
#include "gd_fanout.h"
#include "gd_cache.h"
#include "gd_cx.h"
#include "gd_msd.h"
#include "gd_msd2.h"
#include "gd_shard.h"
#include "gd_comm.h"
#include "gd_localcomm.h"
#include "gd_keyext.h"
#include "gd_frames.h"
#include "gd_dirops.h"
#include "gd_actdir.h"
#include "gd_bucket2.h"
#include "gd_route.h"
#include "gd_radix.h"
#include "gd_mbsort.h"
#include "graindispatch.h"

namespace gd {
struct EncTab;      // gd_encode.h
}

using namespace gd;

namespace gdx {

extern thread_local std::string g_tls_error;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

struct TimedLaunch {
    int name;
    hipEvent_t a, b;
};

}  // namespace gdx

using namespace gdx;

struct gd_handle {
    gd_config cfg{};
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // host-pointer entry points, large batches: copy-in / copy-out streams and their events
    hipStream_t cin = nullptr, cout = nullptr;
    std::vector<hipEvent_t> hp_ev;
    uint32_t host_chunk = 1u << 21;   // messages per pipelined chunk (GD_HOST_CHUNK; 0: no pipelining)
    std::string err;

    // ring snapshot
    int ring_mode = -1;
    uint32_t ring_n = 0, ring_top = 0;
    uint64_t layout_gen = 0;          // bumped whenever ring / table pointers or sizes change
                                      // (captured micro-batch graphs bake them in)
    DevBuf ring_pts, ring_own;

    // directory table
    Slot* slots = nullptr;
    unsigned long long capacity = 0;
    DevCounters* ctr = nullptr;       // device
    DevCounters ctr_host{};           // last copy
    bool ctr_stale = true;            // an untracked table write since the last copy (maybe_grow_async pulls)
    uint64_t pending_in = 0;          // entries asynchronous registrations may have added since the last copy
    DevBuf reg_retry;                 // asynchronous registrations: deferred-claim counts of the gated passes
    DevBuf dir_scr[3];                // directory batches' scratch (slot_of, win, is_new): never the bucketing's

    // scratch
    DevBuf keys_in, u32_a, u32_b, u32_c, u32_d, u8_a, out_a, out_b, out_c, hist, partials, partials2, offs;
    DevBuf fr[16];                    // header-decode scratch (host-pointer entry points)
    DevBuf fr_ext[2];                 // TargetGrain KeyExt offsets / lengths (gd_route_frames_ext*)
    DevBuf churn[5];                  // split scratch: keep mask, flags, positions, out keys/vals
    DevBuf fan_bnd;                   // k_fan_bound's scratch outputs
    DevBuf fan[8];                    // fan-out scratch: ends, total, flags, positions, host-form buffers

    // non-owner directory cache (LocalLookup mode when cache_max > 0)
    CacheSlot* cslots = nullptr;
    unsigned long long ccap = 0;
    CacheCounters* cctr = nullptr;   // device
    DevBuf cx_heap;                  // KeyExt strings of the cache's KeyExt entries (16-B aligned)
    uint64_t cx_used = 0;            // bytes of cx_heap handed out (compacted when it runs out)
    uint32_t cache_max = 0;
    uint32_t cache_nsilos = 0;
    DevBuf cache_local, cache_valid;
    DevBuf cbuf[8];                   // cache scratch
    // the cache's adaptive state and its maintainer (gd_maintain.h, eng_maintain.hip)
    CacheAge* cage = nullptr;         // LastRefreshed / ExpirationTimer per cache slot (beside cslots)
    int64_t cm_initial = 300000000, cm_max = 2400000000ll;   // initial / maximum ExpirationTimer in ticks (30 s, 240 s)
    double cm_growth = 2.0;           // exponentialTimerGrowth
    int64_t cm_clock = 0;             // the cache clock: DateTime.UtcNow of the add path (gd_cache_clock_set)
    uint64_t cm_ring_gen = ~0ull;     // layout_gen the compact owner table was built at
    uint32_t cm_nown = 0;             // distinct ring owners
    DevBuf cm_own[2];                 // compact owner index per ring position; silo of each compact owner
    DevBuf cm_scr[16];                // scan / apply scratch and the last scan's lists (held until the next scan)
    uint32_t cm_scan_n = 0, cm_scan_owners = 0;   // the held lists' sizes
    uint64_t cm_scan_bytes = 0;
    bool cm_scan_valid = false;
    DevBuf shard_dest, shard_hist;    // exchange partition scratch
    DevBuf shard_n1;                  // low N1 words of the batch (k_shard_hist -> k_shard_gather, compact u32)
    bool shard_n1_copy = true;        // GD_SHARD_N1=0: the gather reads N1 from the 24-B keys
    DevBuf up_last;                   // gd_dir_upsert: last batch item per table slot (zero between calls)

    // IsValidSilo (gd_dir_set_valid_silos): bitset over silo indices [0, n_valid); VersionTag and
    // GrainInfo.SingleInstance per slot (gd_dirops.h); dir_op numbers the mutating directory calls
    DevBuf dir_valid;
    uint32_t n_valid = 0;
    std::vector<uint8_t> valid_host;
    uint32_t* vtag = nullptr;
    uint32_t dir_op = 0;
    DevBuf act_ids;                   // ActivationId per host activation index (gd_activation_ids_set)
    uint64_t n_act_ids = 0;
    DevBuf dirop_buf[4];

    // ActivationDirectory of the receive path (gd_actdir.h): ActivationId -> context, flags
    Slot* ad_slots = nullptr;
    unsigned long long ad_cap = 0;
    DevCounters* ad_ctr = nullptr;
    DevCounters ad_host{};
    DevBuf ad_last;
    DevBuf ad_buf[8];
    DevBuf fr_recv[3];                // frames: TargetActivation / Direction scratch when the caller wants neither
    DevBuf frt_scr[8];                // gd_receive_turns_frames*: the decoded fields the caller did not ask back
    DevBuf recv_scr[2];               // receive with limits but no buckets wanted: perm / offsets scratch
    // activation stage (gd_activate.h, eng_activate.hip)
    uint64_t ad_used_ub = 0;          // live + tombstones at most: the last ad_pull plus every possible creation since
    DevBuf actv_scr[10];              // tile counts (candidates, created, gone); candidates' idx, keys, proposals,
                                      // slot_of, is_new; the call's words; the frame-fed chain's IsNewPlacement bytes

    // sender queues (gd_sendq.h, eng_send.hip): the per-silo application bucket (gd_send_configure)
    DevBuf send_tab;
    uint32_t send_nsilos = 0, send_nq = 0;   // 0: not configured
    DevBuf send_scr[2];               // (bucket, tile) counts + totals; bucket ids when the caller wants none

    // placement of unregistered grains (gd_place.h, eng_place.hip): the compatible silos in
    // SiloAddress.CompareTo order and their bitset (gd_place_configure)
    DevBuf place_sorted, place_compat;
    uint32_t place_nsilos = 0, place_ncomp = 0;   // place_nsilos 0: not configured
    bool place_local = false;         // the local silo is active, in the table and compatible
    DevBuf place_scr[7];              // tile counts, block counts; candidates' idx, keys, vals, winners, inserted

    // turn admission (gd_turns.h, eng_turns.hip)
    DevBuf turn_scr[7];               // tile counts; rank key, perm, offsets, rank (limits); wait-list key; merged flags

    // turn completion and message pump, wait-list merge (gd_pump.h, eng_pump.hip)
    DevBuf pump_scr[6];               // completions' perm, offsets; start counts, first positions; work list, its count

    // callback table (gd_callbacks.h, eng_callbacks.hip): CorrelationId -> callback handle, resend count, target silo
    DevBuf cb_tab, cb_dl, cb_ctr;     // the 16-B slots, their deadlines, CbCounters
    DevBuf cb_last;                   // two election words a slot (zero between calls)
    unsigned long long cb_cap = 0;    // slots; 0: not configured (gd_callbacks_configure)
    uint64_t cb_used_ub = 0;          // live + tombstones at most: the last read-back plus every add since
    uint32_t cb_max_resend = 0;       // MessagingOptions.MaxResendCount, ResendOnTimeout, the timer's repeat period
    bool cb_resend_on_timeout = false;
    int64_t cb_period = 0;
    DevBuf cb_scr[4];                 // slot_of, is_new / class, fire tile counts, scan flags

    // frame encoder (gd_encode.h, eng_encode.hip): the wire SiloAddress per silo index, the grain-class name
    // bytes and their offsets (gd_encode_configure)
    DevBuf enc_tab[3];
    uint32_t enc_nsilos = 0, enc_ntypes = 0, enc_maxtype = 0;   // enc_nsilos 0: not configured
    DevBuf enc_scr[3];                // plan records, output lengths, scanned offsets

    // response writer (gd_respond.h, eng_respond.hip): the RejectionInfo strings and their offsets
    // (gd_respond_configure); the silo table is the encoder's
    DevBuf rsp_tab[2];
    uint32_t rsp_ninfo = 0, rsp_maxinfo = 0;
    bool rsp_configured = false;
    DevBuf rsp_scr[3];                // plan records, output lengths, scanned offsets

    // request writer (gd_request.h, eng_request.hip): the DebugContext / GenericGrainType strings and their
    // offsets (gd_request_configure); the ActivationIds, silos and type names are the encoder's
    DevBuf req_tab[2];
    uint32_t req_nstr = 0, req_maxstr = 0;
    bool req_configured = false;
    DevBuf req_scr[4];                // plan records, output lengths, scanned offsets, the send stage's ttl

    // forward writer (gd_forward.h, eng_forward.hip): the ActivationIds, silos and type names are the encoder's
    DevBuf fwd_scr[5];                // plan records, output lengths, scanned offsets, the send stage's ttl and category
    DevBuf rej_scr[3];                // forward rejections: plan records, output lengths, scanned offsets

    // sniff stage (gd_sniff.h, eng_sniff.hip): InvalidateCacheEntry's first-matching-entry word a cache slot (NONE32
    // between calls), the entries' slots, their classes
    DevBuf inv_scr[3];
    unsigned long long inv_cap = 0;   // the cache capacity inv_scr[0] is laid out (and all NONE32) for; 0: not

    // activation collector (gd_collect.h, eng_collect.hip): quantum and nextTicket in ticks (gd_collect_configure)
    int64_t col_quantum = 0, col_next = 0;   // col_quantum 0: not configured
    DevBuf col_scr[5];                // election words (NONE32 between calls); tile counts; verdicts when the caller
                                      // wants none; quantum keys; their bucket offsets

    // gateway (gd_gateway.h, eng_gateway.hip): [0] the client table, [1] the reply routes; each the 32-B slots,
    // the values beside them (GwClient / the route's time), DevCounters + stripes, two election words a slot
    DevBuf gw_slots[2], gw_side[2], gw_ctr[2], gw_last[2];
    unsigned long long gw_cap[2] = {0, 0};
    uint64_t gw_used_ub[2] = {0, 0};  // live + tombstones at most: the last read-back plus every possible add since
    DevBuf gw_state;                  // GwState: next_round_robin, the gated passes' deferred counts
    uint32_t gw_nsenders = 0;         // 0: not configured (gd_gateway_configure)
    int64_t gw_drop_timeout = 0, gw_route_expiry = 0;
    DevBuf gw_scr[6];                 // slot_of, is_new, scan flags, bucket counts, statuses / bucket ids unasked for

    // stateless workers (gd_workers.h, eng_workers.hip): GrainId -> worker set; the 32-B slots, beside each
    // {count, max_local, slot_capacity ctx words}, DevCounters + stripes, two election words a slot
    DevBuf wk_slots, wk_side, wk_ctr, wk_last;
    unsigned long long wk_cap = 0;
    uint64_t wk_used_ub = 0;          // live + tombstones at most: the last read-back plus every possible add since
    uint32_t wk_sc = 0;               // slot_capacity; 0: not configured (gd_workers_configure)
    uint32_t wk_default_ml = 0;       // MaxLocal of a message that brings none
    DevBuf wk_state;                  // the gated passes' deferred counts, then the find pass's miss count
    DevBuf wk_scr[7];                 // slot_of, is_new, perm, offsets, rank, idle counts, scan flags

    // compact route (gd_compact.h, eng_compact.hip): the class table (class id -> TypeCodeData; gd_classes_set) on
    // the device and on the host, the count of silos too wide for 16 bits, and the simple form's 32-bit silos
    DevBuf cls_tab;
    std::vector<uint64_t> cls_host;   // empty: no table set
    DevBuf cls_wide, cls_silo;

    // The host-pointer forms of the six stages above and the collector's stage their inputs and outputs here, through HostStage
    // (below): the k-th array of a call takes slot k; STAGE_SLOTS is the widest call's need (gd_receive_activate_turns_frames).
    // One pool serves them all: each of these calls synchronises the stream before it returns and none reads
    // what an earlier one staged; a call that returned early on an error left its work on the same stream,
    // ahead of the next call's, and ensure() synchronises before it frees a slot to grow it.
    static constexpr uint32_t STAGE_SLOTS = 46;
    DevBuf stage_buf[STAGE_SLOTS];

    // KeyExt grains (gd_keyext.h): device table + heap, and the host index both are kept from
    KxSlot* kx_slots = nullptr;
    uint64_t kx_cap = 0;
    DevBuf kx_heap;
    uint64_t kx_heap_dev = 0;          // host heap bytes already on the device
    std::vector<KxSlot> kx_m;          // host index (same layout as the device table)
    std::vector<uint8_t> kx_hheap;
    uint64_t kx_live = 0, kx_tomb = 0;
    uint32_t kx_maxp = 0;
    DevBuf kx_buf[5];                  // apply / ext staging scratch

    // in-library exchange over RCCL (gd_comm.h): one communicator per handle.  The partition and
    // the RCCL rounds run on xstream; probe + bucketing on `stream`; batch i's exchange overlaps
    // batch i-1's probe + bucketing (receive/result buffers double-buffered by batch parity).
    ncclComm_t comm = nullptr;
    const Rccl* net = nullptr;        // the transport behind comm: RCCL, or the in-process one
    int n_ranks = 0, rank = -1;
    hipStream_t xstream = nullptr;
    // gd_set_bucket_stream: gd_route_bucket_device's bucketing on this stream after the route (event
    // b_ev on the handle's stream), so the next batch's route overlaps this batch's bucketing
    hipStream_t bstream = nullptr;
    hipEvent_t b_ev = nullptr;
    hipEvent_t b_fence_ev = nullptr;  // bfence: the handle's stream waits for a bucketing on bstream
    bool b_pending = false;           // a bucketing was enqueued on bstream since the last bfence
    hipEvent_t fan_ev = nullptr;   // the cascade's per-hop size read-back (fan_count_post / fan_count_wait)
    hipStream_t pstream = nullptr;    // the partition (pack) of the next batch, beside this one's rounds
    hipEvent_t x_in = nullptr, x_hdr[2] = {}, x_route[2] = {}, x_ret[2] = {}, x_done[2] = {};
    // a launch timed for tune_choose was enqueued since the last exchange call: the next call's partition
    // waits for it (route_multi), so the timings are not taken beside the pipeline's overlapped work
    bool measured_launch = false;
    hipEvent_t p_packed = nullptr, x_sent[2] = {}, x_fwd[2] = {}, x_keys[2] = {};
    bool x_done_rec[2] = {false, false}, x_sent_rec[2] = {false, false};
    DevBuf mx_send[2][7];             // per batch parity: send keys, send idx, counts (send/recv messages,
                                      // send/recv KeyExt bytes: 4 x [W]), KeyExt lengths, KeyExt byte
                                      // offsets, KeyExt blob, block starts of 2-B origin indices
    DevBuf mx[2][22];                 // per batch parity: receive / result buffers
    DevBuf mf[2][17];                 // per batch parity, GD_MULTI_FORWARD: forward send (keys, pos, idx,
                                      // src, silo, act, status, counts), forward receive (keys, idx, src,
                                      // silo, act, status), perm, offsets, compact key staging
    DevBuf mx_keys;                   // host-keys entry point: the batch, on xstream
    DevBuf mx_ext[3];                 // host-keys entry point: its KeyExt blob, offsets, lengths
    DevBuf x_scratch[4];              // xstream's own scan partials + partition scratch
    DevBuf p_scratch[4];              // pstream's
    uint32_t* h_xcnt = nullptr;       // pinned: send/recv message counts, send/recv KeyExt byte counts,
                                      // key descriptors (mine, every peer's), forward counts (12 x 256)
    gd_multi_result mres[2] = {};
    // sharded fan-out cascade (gd_fanout_multi_device): per hop the frontier and the owner-side
    // results, kept for the caller; shared expansion / partition scratch
    std::vector<std::array<DevBuf, 10>> fm_hop;
    std::vector<gd_fanout_hop> fm_res;
    uint32_t fm_n_act = 0;
    DevBuf fm_scr[6];                 // expand target / sender, partitioned target / sender, counts, visited
    DevBuf fm_graph[3];               // host-form entry point: row_off, dst, seeds
    // multi-rank directory handoff (gd_dir_handoff_multi): split / send scratch, received entries
    DevBuf ho_send[10];
    DevBuf ho_recv[11];
    gd_handoff_result ho_res{};
    bool ho_valid = false;
    uint32_t mres_n[2] = {0, 0};
    uint64_t mcalls = 0;
    uint64_t routed = 0;

    // kernel tuning (defaults measured on MI355X; GD_ROUTE_M / GD_ROUTE_NT override for A/B runs)
    bool route_xcd = true;      // route workgroups over XCD-contiguous message ranges (GD_ROUTE_XCD)
    // compact probe index (gd_cx.h): derived from the table, rebuilt after any change of it (GD_CX=0: off)
    int cx_mode = 1;            // 0 off, 1 measured (default), 2 index group reads, 3 index slot reads (GD_CX)
    bool mb_zero_copy = true;   // micro-batches: I/O from / to pinned host memory (GD_OPT_MB_ZEROCOPY)
    uint32_t mb_split = 8;      // micro-batches: redundant sorters splitting the host stores (GD_OPT_MB_SPLIT)
    bool mb_trace = false;      // micro-batches: per-phase timestamps (GD_OPT_MB_TRACE)
    bool fan_bound = false;     // a k_fan_bound launch beside each 8-B-index k_fan_route (GD_OPT_FAN_BOUND)
    uint32_t fan_bound_n = 0;   // ... before it on even launches, after it on odd ones
    bool mb_poll = true;        // micro-batches: completion by the sort's pinned count (GD_OPT_MB_POLL)
    bool walk_cih = false;      // the frame stages step over a CacheInvalidationHeader (GD_OPT_WALK_INVALIDATION)
    int tune_pin[GD_TUNE_KINDS] = {-1, -1, -1, -1, -1};   // gd_tune_set: pinned variant per kind, -1 measured
    int msd_mode = 1;           // two-level bucketing (gd_msd.h, gd_msd2.h): 0 off, 1 measured (default), 2 always (GD_MSD)
    uint32_t l2_small = 1024;   // three-pass form: ranges of at most this many messages are sorted one wave a range
    uint32_t l2_mid = MSD_MID_CAP;  // three-pass form: staged ranges up to this many messages on the 512-thread sort
    uint32_t b2_persist = 2;       // one-pass MSD scatter: persistent workgroups a CU (0: one a tile; GD_OPT_B2_PERSIST)
    uint32_t b2_order = 0;         // its tile order: 0 strided, 1 consecutive runs a workgroup (GD_OPT_B2_ORDER)
    uint32_t l2_staged = MSD_CAP;  // three-pass form: ranges up to this many messages one workgroup each, more: chunks
    uint32_t n_cu = 256;        // compute units (hipDeviceProp_t::multiProcessorCount): persistent grids
    DevBuf m3[15];              // three-pass form's scratch (msd3_bucket)
    DevBuf tune_buf;            // gd_tune_agree's send / receive records
    // per launch kind and size class: the probe variant, timed on live launches.  Variants: 0 the index
    // in 64-B group reads, 1 the directory, 2 the index in 16-B slot reads, 3 the 8-B index (24-B keys)
    static constexpr int CXV = 4;
    struct CxTune {
        int pick = -1;          // -1 measuring, else the variant
        int round = 0;
        int nvar = 0;           // the variants this entry measures (the 8-B index only where it is built)
        float best[CXV] = {1e30f, 1e30f, 1e30f, 1e30f};
        hipEvent_t a[CXV] = {}, b[CXV] = {};
        bool pending[CXV] = {};
        uint64_t n[CXV] = {};
    };
    std::map<int, CxTune> cx_tune;   // key: (kind * 64 + size class (bit length of n)) * 32 + a second class
    uint64_t tab_gen = 0;       // bumped by every launch that takes the table as a writable Slot* (untracked)
    uint32_t tab_track = 0;     // > 0: inside a directory batch that re-projects its slots (TabTrack, k_cx_sync)
    bool cx_built = false, cx_ok = false;
    const Slot* cx_slots_at = nullptr;
    uint64_t cx_cap_at = 0, cx_gen_at = 0;
    DevBuf cxi_tab, cxi_types, cxi_ctr;   // 16-B index; its type set (+ a count per slot); CxCounters
    bool cx8_ok = false;        // the 8-B index is built and current with cx
    // ... and pure: one grain class, every live entry held and none redirected (CxCounters::out8 = 0), as of
    // a counter read-back with no directory batch enqueued since -- k_route_m's PURE form, whose walks
    // need no directory fallback
    bool cx8_pure = false;
    Cx8Args cx8_layout{};       // its layout (types, bits), fixed at the build
    DevBuf cx8_tab;
    // the direct table standing in for a pure 8-B index over dense N1s (gd_probe.h CxdArgs, eng_route.hip
    // cxd_prepare).  cx_snap + tab_gen is the directory's snapshot id: every path that clears cx8_pure or
    // rebuilds / re-lays the 8-B index advances one of the two.  The table is read only under the id it was
    // built at, and built only when the previous k_route launch found the index pure under the same id.
    DevBuf cxd_tab;
    uint64_t cx_snap = 0;
    bool cxd_ok = false;
    uint32_t cxd_d = 0;                          // its entries
    uint64_t cxd_snap_at = 0;                    // the snapshot id it was built at
    bool cxd_seen = false;                       // the previous k_route launch found the index pure ...
    uint64_t cxd_seen_snap = 0;                  // ... under this snapshot id
    uint64_t cxd_builds = 0;
    CxCounters cx_ctr_host{};   // the last read-back of the index counters
    uint32_t cx_out8_at = 0, cx_held8_at = 0;   // at the build: live entries the 8-B index left out / held
    uint64_t cx_builds = 0, cx_synced = 0;      // full builds; slots re-projected by k_cx_sync (gd_stats)
    double cx_build_ms = 0.0;                   // host wall time of the last full build
    uint32_t xcd_tiles = 1;     // XCD-contiguous tile ranges in the radix scatter (GD_XCD_TILES)
    bool hist_xcd = true;       // multi-tile histograms in reverse XCD tile order (GD_HIST_XCD)
    bool compact_headers = true;    // 8-B exchange headers for uniform batches (GD_COMPACT_HEADERS=0: off)
    bool region_probe = false;      // gd_route_multi: chunks ordered by table region, region-mapped probe (GD_REGION_PROBE)
    bool idx16 = true;              // gd_route_multi: 2-B origin indices on the wire (KD_IDX16, GD_IDX16)
    bool pack_pay16 = false;        // set by route_multi around its partition: the scatter writes u16 payloads
    bool narrow_headers = true;     // compact headers as u32 N1s when every N1 < 2^32 (GD_NARROW_HEADERS=0: u64)
    bool shard_gather = true;   // exchange partition of keys: k_shard_gather (GD_SHARD_GATHER=0: k_shard_scatter, staged keys)
    const uint32_t* last_totals = nullptr;   // the last radix pass's digit totals (row scans), and their count
    uint32_t last_digits = 0;
    uint32_t radix_rank_atomic = 1;   // stable in-wave rank by ds_add_rtn (1, A/B: ab_bucket.py) or ballots (0)
    bool lane_order = true;           // gd_create's k_lane_order_check passed (else every rank by ballots)
    bool lane_order_forced_off = false;   // GD_CFG_NO_LANE_ORDER: behave as on a device without it (tests)

    // pinned host scratch for small device -> host read-backs (counts, totals)
    void* h_pin = nullptr;
    size_t h_pin_bytes = 0;

    // per-kernel timing
    int timing = 0;             // gd_set_kernel_timing: 0 off, 1 every launch, 2 the stages (StageTime) only
    std::vector<std::string> tnames;
    std::vector<double> tms;
    std::vector<uint64_t> tcount;
    std::vector<TimedLaunch> pending;
    std::vector<hipEvent_t> event_pool;
};

namespace gdx {

#define HIP_TRY(h, expr)                                                                    \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return set_err((h), GD_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define GD_TRY(expr)              \
    do {                          \
        int r_ = (expr);          \
        if (r_ != GD_OK) return r_; \
    } while (0)

#define NCCL_TRY(h, expr)                                                                          \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess)                                                                     \
            return set_err((h), GD_ERCCL, "%s: %s", #expr, (h)->net->GetErrorString(r_));          \
    } while (0)

inline uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

// f(std::integral_constant<int, MODE>) for the handle's ring mode: the kernels take it as a template argument.
template <typename F>
auto with_ring_mode(int ring_mode, F&& f) {
    switch (ring_mode) {
        case GD_RING_DIRECTORY: return f(std::integral_constant<int, GD_RING_DIRECTORY>{});
        case GD_RING_CONSISTENT: return f(std::integral_constant<int, GD_RING_CONSISTENT>{});
        default: return f(std::integral_constant<int, GD_RING_VIRTUAL_BUCKETS>{});
    }
}

struct Lane {
    const void* send;
    void* recv;
    size_t elem;            // bytes per element
    ncclDataType_t type;
    size_t per;             // elements of `type` per element
    const uint64_t* sb = nullptr;   // set: per-peer byte ranges [sb[r], sb[r+1]) sent to r and
    const uint64_t* rb = nullptr;   // [rb[r], rb[r+1]) received from r (compact headers)
    const uint64_t* rsz = nullptr;  // set (with rb): bytes received from r at rb[r] (padded layouts)
};

// ---- shared across the engine's translation units (definitions in eng_*.hip)
int set_err(gd_handle* h, int code, const char* fmt, ...);
int ensure(gd_handle* h, DevBuf& b, size_t bytes);
int ensure_own(gd_handle* h, DevBuf& b, size_t bytes);
void free_buf(DevBuf& b);
int name_id(gd_handle* h, const char* name);
hipEvent_t take_event(gd_handle* h);
int resolve_timing(gd_handle* h);
int check_ring(gd_handle* h);
RingArgs ring_args(gd_handle* h);
TableArgs table_args(gd_handle* h);
bool host_silo_valid(const gd_handle* h, uint32_t silo);
size_t ring_lds(gd_handle* h);
int pull_counters(gd_handle* h);
int fold_counters(gd_handle* h, DevCounters* c);
int alloc_table(gd_handle* h, unsigned long long cap, Slot** out);
int alloc_vtag(gd_handle* h, unsigned long long cap, uint32_t** out);
unsigned long long pow2_at_least(unsigned long long x);
int cx_ensure(gd_handle* h, bool* ok, uint64_t n);
bool cx_current(const gd_handle* h);
struct TabTrack;
int cx_sync(gd_handle* h, TabTrack& tt, const uint32_t* slot_of, uint32_t n);
bool cx_inline(gd_handle* h, TabTrack& tt, uint32_t n);
CxBuild cx_build_args(gd_handle* h);
int tune_key(int kind, uint64_t n, int sub);
int tune_nvar(int kind);
int tune_nvar_now(const gd_handle* h, int kind);
void tune_resolve(gd_handle::CxTune& t, int nvar);
int tune_choose(gd_handle* h, int kind, uint64_t n, int* meas, int nvar, int sub = 0);
int cx_choose(gd_handle* h, int kind, uint64_t n, int* meas, int nvar = gd_handle::CXV);
Cx8Args cx8_args(gd_handle* h);
CxArgs cx_args(gd_handle* h);
int route_n1_device(gd_handle* h, const void* n1s, uint32_t n1w, uint64_t tcd, uint32_t n, uint32_t* silo,
                    uint32_t* act, uint8_t* status, const uint32_t* rcnt = nullptr, uint32_t world = 0,
                    uint32_t* src = nullptr);
int route_region_device(gd_handle* h, const void* k, uint32_t n1w, uint64_t tcd, uint32_t m, const uint32_t* seg,
                        uint32_t world, uint32_t* silo, uint32_t* act, uint8_t* status);
int route_cached(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t* silo, uint32_t* act, uint8_t* status,
                 bool touch);
int route_cached_keyext(gd_handle* h, const gd_key* keys, const ExtArgs& x, uint32_t n, uint32_t* silo, uint32_t* act,
                        uint8_t* st);
int route_device(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t* silo, uint32_t* act, uint8_t* status,
                 bool touch = true);
int route_bound_device(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t* silo, uint32_t* act,
                       uint8_t* status);
KxArgs kx_args(gd_handle* h);
int keyext_pass(gd_handle* h, const gd_key* keys, const ExtArgs& x, uint32_t n, uint32_t* silo, uint32_t* act,
                uint8_t* st);
int ring_owner_device(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t* silo);
int bucket_device(gd_handle* h, const uint32_t* acts, uint32_t n, uint32_t n_act, uint32_t* perm, uint32_t* offsets,
                  uint32_t* rank_out = nullptr);
int sync(gd_handle* h);
int pinned_scratch(gd_handle* h, size_t bytes);
int check_not_capturing(gd_handle* h, const char* call);
int read_back(gd_handle* h, const void* d, uint32_t* out, size_t words);
int sync_checked(gd_handle* h);
int report_device_error(gd_handle* h);
int maybe_grow_table(gd_handle* h, uint64_t incoming);
int grow_table(gd_handle* h, uint64_t incoming);
int fwd_pack(gd_handle* h, const gd_key* keys, const uint8_t* st, const uint32_t* silo, uint32_t n, uint32_t n_shards,
             uint32_t my_rank, void* out_keys, uint32_t* out_pos, uint32_t* counts, const uint32_t* n1 = nullptr);
bool host_pinned(const void* p);
// The probe index up to which the routes read their key stream non-temporally (route_mode).
constexpr uint64_t ROUTE_NT_INDEX_BYTES = 64ull << 20;
#if GD_DIRECT_INDEX
int cxd_prepare(gd_handle* h, bool cx, int var, bool* use, CxdArgs* d);
#endif
int compact_route_device(gd_handle* h, const uint8_t* cls, const void* n1s, uint32_t n1w, uint32_t n, uint32_t* act,
                         uint16_t* silo16, uint8_t* status, uint32_t* wide);
int bucket_after_route(gd_handle* h, const uint32_t* d_act, uint32_t n, uint32_t n_act, uint32_t* d_perm,
                       uint32_t* d_offsets);
int route_bucket_host_pipelined(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t n_act, uint32_t* out_silo,
                                uint32_t* out_act, uint8_t* out_status, uint32_t* out_perm, uint32_t* out_offsets);
int register_core(gd_handle* h, const gd_key* dk, const gd_val* dvals, uint32_t n, gd_val* out_vals,
                  uint8_t* out_ins, bool async = false);
int unregister_core(gd_handle* h, const gd_key* dk, const uint32_t* dacts, uint32_t n, uint8_t* out_removed);
int maybe_grow_async(gd_handle* h, uint64_t incoming);
int bfence(gd_handle* h);
int slot_words(gd_handle* h);
int claim_passes(gd_handle* h, bool actdir, const gd_key* dk, uint32_t n, uint32_t* slot_of, uint8_t* is_new,
                 const gd_val* vals, const TableArgs& vt, uint32_t* last, uint32_t first_pass, const char* call);
int split_count(gd_handle* h, const uint8_t* keep, uint32_t n_keep, uint64_t* total);
uint64_t grain_tcd(int32_t type_code);
int fan_count(gd_handle* h, const uint32_t* row_off, uint32_t n_nodes, const uint32_t* frontier, uint32_t nf,
              uint64_t* total);
int route_nodes(gd_handle* h, const uint32_t* nodes, uint32_t n, uint64_t tcd, uint32_t* silo, uint32_t* act,
                uint8_t* status);
int frontier_next_dev(gd_handle* h, const uint32_t* offsets, uint32_t n_act, uint8_t* visited, uint32_t* out,
                      const uint32_t** d_nf);
int fan_count_dev(gd_handle* h, const uint32_t* row_off, uint32_t n_nodes, const uint32_t* frontier,
                  const uint32_t* d_nf, uint32_t nf_max, uint32_t* nf, uint64_t* total);
void comm_release(gd_handle* h);
int need_comm(gd_handle* h);
int exchange_round(gd_handle* h, const char* name, const uint32_t* sc, const uint64_t* soff, const uint32_t* rc,
                   const uint64_t* roff, const Lane* lanes, int n_lanes);
int counts_round(gd_handle* h, uint32_t* dcnt, std::vector<uint32_t>& sc, std::vector<uint32_t>& rc);
bool is_keyext_cat(uint64_t tcd);
uint32_t kx_hash_host(const gd_key& k, const uint8_t* s, int32_t len);
int host_ext(gd_handle* h, const gd_key_ext* ext, uint32_t i, const uint8_t*& s, int32_t& len);
int kx_commit(gd_handle* h, std::vector<uint64_t>& dirty);
int stage_ext(gd_handle* h, const gd_key_ext* ext, uint32_t n, gd_key_ext* dx);
bool ext_ok(const gd_key_ext* ext, uint32_t n);
int grow_act_ids(gd_handle* h, uint64_t need);
int check_dir_err(gd_handle* h, const char* what);
int merge_core(gd_handle* h, const gd_key* dk, const gd_val* dvals, const int32_t* dtags, uint32_t n,
               uint8_t* d_status, gd_val* d_dropped);
AdArgs ad_args(gd_handle* h);
int check_frames_args(gd_handle* h, const void* buf, const void* off, uint32_t n, const gd_frame_fields* out);
int decode_frames_device(gd_handle* h, const uint8_t* buf, uint64_t len, const uint64_t* off, uint32_t n,
                         const gd_frame_fields* out, bool ext = false, const gd_frame_turn_fields* turn = nullptr);
struct HostStage;
void stage_frame_outputs(HostStage& io, uint32_t n, const gd_frame_fields* want, const gd_frame_turn_fields* twant,
                         gd_frame_fields* dev, gd_frame_turn_fields* tdev);
int frame_scratch(gd_handle* h, uint32_t n, const gd_frame_fields* want, gd_frame_fields* dev);
int frame_results(gd_handle* h, uint32_t n, const gd_frame_fields* want, const gd_frame_fields* dev);
// ---- the stages that write frames into one contiguous output (eng_frameout.hip)
// The ActivationIds, wire silos and grain-class names of gd_encode_configure as the kernels take them.
EncTab enc_tab(gd_handle* h);
// A stage's scratch: scr[0] n plan records of plan_bytes (+ plan_pad, where the writer reads past them), scr[1] n
// output lengths, scr[2] n + 1 scanned offsets (+ 16 bytes of slack).
int frameout_scratch(gd_handle* h, DevBuf* scr, uint32_t n, size_t plan_bytes, size_t plan_pad = 0);
// offs[j] = the first output byte of frame order[j] (order null: j), offs[n] the total, from the planner's lens;
// out_off the same as u64; ERR_ENC_FULL when the total exceeds out_cap.  tag names the scan's profile row.
int frameout_offsets(gd_handle* h, const uint32_t* lens, const uint32_t* order, uint32_t n, uint32_t* offs,
                     uint64_t out_cap, uint64_t* out_off, const char* tag);
// The end of a host-pointer call: io's outputs (out_off among them) come down, then the out_off[n] bytes of d_out
// when they fit cap; *out_total = out_off[n].  Returns sync_checked's result.
int frameout_fetch(gd_handle* h, HostStage& io, const uint64_t* out_off, uint32_t n, uint8_t* out_buf,
                   const uint8_t* d_out, uint64_t cap, uint64_t* out_total);
int bucket_lsd(gd_handle* h, const uint32_t* acts, uint32_t n, uint32_t n_act, uint32_t* perm, uint32_t* offsets,
               uint32_t* rank_out);
bool msd3_split(uint32_t n_act, uint32_t* a_out, uint32_t* ra_out);
int frontier_next(gd_handle* h, const uint32_t* offsets, uint32_t n_act, uint8_t* visited, uint32_t* out,
                  uint32_t* out_n);
int route_frames_device(gd_handle* h, const uint8_t* buf, uint64_t len, const uint64_t* off, uint32_t n,
                        uint32_t n_act, const gd_frame_fields* out, uint32_t* silo, uint32_t* act, uint8_t* status,
                        uint32_t* perm, uint32_t* offsets, bool ext = false);
int receive_device(gd_handle* h, const gd_key* tg, const gd_key* ta, const uint8_t* dir, const uint32_t* fflags,
                   uint32_t n, uint32_t n_ctx, const gd_recv_limits* lim, uint32_t* ctx, uint8_t* st, uint32_t* perm,
                   uint32_t* offsets);
int receive_frames_device(gd_handle* h, const uint8_t* buf, uint64_t len, const uint64_t* off, uint32_t n,
                          uint32_t n_ctx, const gd_recv_limits* lim, const gd_frame_fields* out, uint32_t* ctx,
                          uint8_t* st, uint32_t* perm, uint32_t* offsets, const gd_frame_turn_fields* turn = nullptr);
int grow(gd_handle* h, DevBuf& b, size_t bytes);
int comm_setup(gd_handle* h);
int kx_rehash(gd_handle* h, uint64_t cap);
int kx_upload_all(gd_handle* h);
int cache_check(gd_handle* h);
int cache_rehash(gd_handle* h, unsigned long long cap);
int cx_reserve(gd_handle* h, uint64_t need);
int ad_reserve(gd_handle* h, uint64_t incoming);
int ad_pull(gd_handle* h);
int ad_rehash(gd_handle* h, unsigned long long cap);
// The activation stage on device arrays (eng_activate.hip); the chained forms call it between the receive and the
// turn stage (eng_turns.hip).
struct ActivateArgs {
    const uint32_t* ctx;
    const uint8_t* recv_status;
    const gd_key* target_activation;
    const uint8_t* direction;
    const int64_t* ttl;
    const uint8_t* new_placement;
    int64_t ttl_age;
    uint32_t n, n_ctx;
    int terminating;
    uint32_t ctx_base;
    const uint32_t* new_ctx;
    uint32_t cap_new;
    uint8_t* kind;
    uint32_t* ctx_out;
    uint8_t* status_out;
    uint32_t *new_idx, *n_new, *gone_idx, *n_gone, *n_proposed;
};
int check_activate_args(gd_handle* h, const ActivateArgs& a, const char* call);
int activate_device(gd_handle* h, const ActivateArgs& a, bool host_form, bool* refused, const char* call);
int frame_new_placement_device(gd_handle* h, const uint8_t* buf, uint64_t len, const uint64_t* off, const uint8_t* st,
                               uint32_t n, const uint8_t** out);
int fan_args_ok(gd_handle* h, const uint32_t* row_off, const uint32_t* dst, uint32_t nf, const uint32_t* frontier,
                uint64_t* out_n);
int fan_route(gd_handle* h, const uint32_t* row_off, const uint32_t* dst, const uint32_t* frontier, uint32_t nf,
              uint32_t total, uint64_t tcd, uint32_t* target, uint32_t* sender, uint32_t* silo, uint32_t* act,
              uint8_t* status, const uint32_t* d_nf = nullptr, bool dev_total = false);
int cache_pull(gd_handle* h, CacheCounters* c);
CacheArgs cache_args(gd_handle* h);
// AddOrUpdate / Remove / MarkAsFresh of a batch in order (kinds NULL: every item an add); eng_cache.hip.
int cache_batch_impl(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, const uint8_t* kinds, const gd_val* vals,
                     const int32_t* versions, uint32_t n, uint8_t* out_status);
int cache_touch(gd_handle* h, uint32_t* hit, const uint32_t* cslot, uint32_t n);
int split_emit(gd_handle* h, int move, gd_key* d_keys, gd_val* d_vals);
int set_bitset(gd_handle* h, DevBuf& b, const std::vector<uint32_t>& bits);
int mb_enqueue(gd_microbatch* mb, uint32_t n, bool count_done);
template <class Op>
int scan_device(gd_handle* h, uint32_t* data, uint32_t n, bool reverse, bool inclusive, const char* tag,
                uint32_t* out = nullptr);
template <bool NODES>
int shard_pack(gd_handle* h, const void* recs, const uint32_t* payload, uint32_t n, uint64_t tcd, uint32_t n_shards,
               void* out_recs, uint32_t* out_pay, uint32_t* counts, const ExtArgs& ext = ExtArgs{},
               uint32_t* kdesc = nullptr, uint32_t regions = 1);

// A launch argument that is the directory table as a writable Slot* (the kernel may change it).
template <typename T>
bool writes_table(const gd_handle*, const T&) { return false; }
inline bool writes_table(const gd_handle* h, Slot* p) { return p != nullptr && p == h->slots; }

// Launch a kernel on the handle's stream; with GD_CFG_KERNEL_TIMING bracket it by events.  A kernel
// handed the table as a writable Slot* invalidates the compact probe index (tab_gen), unless it runs
// inside a TabTrack scope, whose batch re-projects the slots it touched (cx_sync).
template <typename K, typename... Args>
int launch(gd_handle* h, const char* name, dim3 grid, dim3 block, size_t lds, K kernel, Args... args) {
    if (grid.x == 0) return GD_OK;
    if (!h->tab_track && (writes_table(h, args) || ...)) {
        h->tab_gen++;
        h->ctr_stale = true;
    }
    hipEvent_t a = nullptr, b = nullptr;
    if (h->timing == 1) {
        a = take_event(h);
        b = take_event(h);
        HIP_TRY(h, hipEventRecord(a, h->stream));
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, h->stream, args...);
    HIP_TRY(h, hipGetLastError());
    if (h->timing == 1) {
        HIP_TRY(h, hipEventRecord(b, h->stream));
        h->pending.push_back(TimedLaunch{name_id(h, name), a, b});
    }
    return GD_OK;
}

// Stage timing (gd_set_kernel_timing 2): one event pair around a whole stage -- e.g. every launch of a
// bucketing -- recorded under `name`, with no events between its kernels (per-launch events add ~5 us a
// kernel and so inflate a many-kernel stage).
struct StageTime {
    gd_handle* h;
    int name = -1;
    hipEvent_t a = nullptr, b = nullptr;
    StageTime(gd_handle* hh, const char* nm) : h(hh) {
        if (h->timing != 2) return;
        name = name_id(h, nm);
        a = take_event(h);
        b = take_event(h);
        (void)hipEventRecord(a, h->stream);
    }
    ~StageTime() {
        if (name < 0) return;
        (void)hipEventRecord(b, h->stream);
        h->pending.push_back(TimedLaunch{name, a, b});
    }
};

// A directory batch whose table writes keep the probe indexes current: the slots it touched are
// re-projected by cx_sync (which calls done()); a batch that ends early (an error) leaves the indexes
// stale instead, and the next large route rebuilds them.
struct TabTrack {
    gd_handle* h;
    bool was_current;
    bool synced = false;
    explicit TabTrack(gd_handle* hh);
    ~TabTrack() {
        --h->tab_track;
        if (!synced) h->tab_gen++;
    }
};

// Brackets a launch chosen by cx_choose / tune_choose with the tune entry's events.
struct CxMeasure {
    gd_handle* h;
    int slot;
    uint64_t n;
    CxMeasure(gd_handle* hh, int sl, uint64_t nn) : h(hh), slot(sl), n(nn) {
        if (slot >= 0) (void)hipEventRecord(h->cx_tune[slot / gd_handle::CXV].a[slot % gd_handle::CXV], h->stream);
    }
    ~CxMeasure() {
        if (slot < 0) return;
        auto& t = h->cx_tune[slot / gd_handle::CXV];
        const int v = slot % gd_handle::CXV;
        (void)hipEventRecord(t.b[v], h->stream);
        t.n[v] = n;
        t.pending[v] = true;
    }
};

template <typename T>
int h2d(gd_handle* h, DevBuf& b, const T* src, size_t count) {
    GD_TRY(ensure(h, b, count * sizeof(T)));
    if (count) HIP_TRY(h, hipMemcpyAsync(b.p, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return GD_OK;
}

template <typename T>
int d2h(gd_handle* h, T* dst, const DevBuf& b, size_t count) {
    if (count && dst) HIP_TRY(h, hipMemcpyAsync(dst, b.p, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    return GD_OK;
}

// The staging of one host-pointer call through the handle's stage_buf pool: inputs up, outputs down.
//   * Slots are positional: the k-th in / out / out_if / hold of a call takes slot k, whether or not an
//     optional array is there, so calls that toggle optional arrays reuse the same allocations.  More than
//     STAGE_SLOTS arrays in a call is GD_ESTATE.
//   * A slot holds at least count * sizeof(T) + pad bytes: pad is the tail a kernel's wide accesses may
//     touch past count, and each call states its own.
//   * Nothing here synchronises: in() and fetch() enqueue copies on the handle's stream, and the entry point
//     ends as it chooses (sync, sync_checked, a counter read-back).
// After a failure every later in / out / hold gives null and enqueues nothing; status() is the first failure.
struct HostStage {
    gd_handle* h;
    int rc = GD_OK;
    uint32_t used = 0, n_down = 0;
    struct Down {
        void* dst;
        const void* src;
        size_t bytes;
    } down[gd_handle::STAGE_SLOTS];

    explicit HostStage(gd_handle* hh) : h(hh) {}

    // The next slot; null for an absent array (want false) and after a failure.
    DevBuf* take(bool want) {
        const uint32_t k = used++;
        if (rc != GD_OK || !want) return nullptr;
        if (k < gd_handle::STAGE_SLOTS) return &h->stage_buf[k];
        rc = set_err(h, GD_ESTATE, "host staging: more than %u arrays in one call", gd_handle::STAGE_SLOTS);
        return nullptr;
    }
    // src's count elements on the device; a null src gives null and copies nothing.
    template <typename T>
    const T* in(const T* src, size_t count) {
        DevBuf* b = take(src != nullptr);
        if (b) rc = h2d(h, *b, src, count);
        return b && rc == GD_OK ? (const T*)b->p : nullptr;
    }
    // A device array that fetch() leaves alone: the call brings down what it needs of it, fetch(dst, d, count).
    template <typename T>
    T* hold(size_t count, size_t pad = 0, bool want = true) {
        DevBuf* b = take(want);
        if (b) rc = ensure(h, *b, count * sizeof(T) + pad);
        return b && rc == GD_OK ? (T*)b->p : nullptr;
    }
    // A device array whose first count elements fetch() brings down to dst (a null dst: nowhere).
    template <typename T>
    T* out(T* dst, size_t count, size_t pad = 0) {
        T* d = hold<T>(count, pad);
        if (d && dst && count) down[n_down++] = Down{dst, d, count * sizeof(T)};
        return d;
    }
    // out() for an optional output: a null dst takes the slot, allocates nothing and gives null.
    template <typename T>
    T* out_if(T* dst, size_t count, size_t pad = 0) {
        return dst ? out(dst, count, pad) : hold<T>(0, 0, false);
    }
    int status() const { return rc; }
    // Enqueue the copies out() remembered, in slot order.
    int fetch() {
        for (uint32_t i = 0; i < n_down; ++i)
            HIP_TRY(h, hipMemcpyAsync(down[i].dst, down[i].src, down[i].bytes, hipMemcpyDeviceToHost, h->stream));
        n_down = 0;
        return GD_OK;
    }
    // Enqueue one copy of count elements from a device array of this call.
    template <typename T>
    int fetch(T* dst, const void* d, size_t count) {
        if (count && dst) HIP_TRY(h, hipMemcpyAsync(dst, d, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
        return GD_OK;
    }
};

// ---- the pipelined host route (gd_route / gd_route_bucket and their compact forms on pinned buffers)
// One per-message array of the call: elem bytes a message, its host and its device end.
struct HpStream {
    void* host;
    void* dev;
    size_t elem;
};
// An array brought down whole after the last chunk (and the bucketing).
struct HpTail {
    void* host;
    const void* dev;
    size_t bytes;
};

// Host buffers, large batch: the PCIe copies overlap the kernels.  Chunk k's inputs (up[]) go up on the
// copy-in stream while chunk k-1 is routed on the handle's stream -- route(off, cnt) enqueues it -- and
// chunk k-2's routes (down[]) come down on the copy-out stream (PCIe is full duplex); the bucketing
// (d_perm != nullptr: of d_act into d_perm / d_offs) needs the whole batch, so it and the tail[] copies
// follow the last chunk.  Bounded by the slower direction's bytes instead of the sum of both.  Used when
// the caller's buffers are pinned (gd_host_alloc).
template <typename Route>
int host_pipeline(gd_handle* h, uint32_t n, const HpStream* up, int n_up, const HpStream* down, int n_down, Route route,
                  const uint32_t* d_act, uint32_t n_act, uint32_t* d_perm, uint32_t* d_offs, const HpTail* tail,
                  int n_tail) {
    if (!h->cin) HIP_TRY(h, hipStreamCreateWithFlags(&h->cin, hipStreamNonBlocking));
    if (!h->cout) HIP_TRY(h, hipStreamCreateWithFlags(&h->cout, hipStreamNonBlocking));
    const uint32_t C = h->host_chunk;
    const uint32_t nch = (uint32_t)(((uint64_t)n + C - 1) / C);
    while (h->hp_ev.size() < 2 * (size_t)nch + 2) {
        hipEvent_t e;
        HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->hp_ev.push_back(e);
    }
    hipEvent_t* ev = h->hp_ev.data();
    HIP_TRY(h, hipEventRecord(ev[2 * nch], h->stream));        // earlier work on the handle's stream
    HIP_TRY(h, hipStreamWaitEvent(h->cin, ev[2 * nch], 0));
    for (uint32_t k = 0; k < nch; ++k) {
        const size_t off = (size_t)k * C;
        const uint32_t cnt = (uint32_t)std::min<size_t>(C, n - off);
        for (int s = 0; s < n_up; ++s)
            HIP_TRY(h, hipMemcpyAsync((char*)up[s].dev + off * up[s].elem, (const char*)up[s].host + off * up[s].elem,
                                      (size_t)cnt * up[s].elem, hipMemcpyHostToDevice, h->cin));
        HIP_TRY(h, hipEventRecord(ev[2 * k], h->cin));
        HIP_TRY(h, hipStreamWaitEvent(h->stream, ev[2 * k], 0));
        GD_TRY(route(off, cnt));
        HIP_TRY(h, hipEventRecord(ev[2 * k + 1], h->stream));
        HIP_TRY(h, hipStreamWaitEvent(h->cout, ev[2 * k + 1], 0));
        for (int s = 0; s < n_down; ++s)
            HIP_TRY(h, hipMemcpyAsync((char*)down[s].host + off * down[s].elem,
                                      (const char*)down[s].dev + off * down[s].elem, (size_t)cnt * down[s].elem,
                                      hipMemcpyDeviceToHost, h->cout));
    }
    const bool bucket = d_perm != nullptr;          // else routes only, no bucketing
    if (bucket) GD_TRY(bucket_device(h, d_act, n, n_act, d_perm, d_offs));
    if (bucket || n_tail) {
        HIP_TRY(h, hipEventRecord(ev[2 * nch + 1], h->stream));
        HIP_TRY(h, hipStreamWaitEvent(h->cout, ev[2 * nch + 1], 0));
        for (int s = 0; s < n_tail; ++s)
            HIP_TRY(h, hipMemcpyAsync(tail[s].host, tail[s].dev, tail[s].bytes, hipMemcpyDeviceToHost, h->cout));
    }
    HIP_TRY(h, hipStreamSynchronize(h->cout));
    return bucket ? sync_checked(h) : sync(h);
}

// ---- the stages that keep a table of their own (the callback table, the gateway's two)
// The claim passes of a batch (gd_dirbatch.h) over the `passes` words of `retry`, zeroed here: run(p, gate,
// word) launches pass p, which counts the items it defers into `word` and, with a gate, runs only if the gate
// word is not zero.  Pass 0, then (sync_passes, the host forms) one pass after each read-back of a count that is
// not zero; else passes - 1 gated ones, *unsettled = the last one's word for the caller's flag (null otherwise).
template <typename F>
int claim_pass_driver(gd_handle* h, uint32_t* retry, uint32_t passes, bool sync_passes, const char* call,
                      const uint32_t** unsettled, F run) {
    *unsettled = nullptr;
    HIP_TRY(h, hipMemsetAsync(retry, 0, sizeof(uint32_t) * passes, h->stream));
    GD_TRY(run(0u, (const uint32_t*)nullptr, &retry[0]));
    if (sync_passes) {
        for (uint32_t p = 1;; ++p) {
            uint32_t deferred = 0;
            GD_TRY(read_back(h, &retry[(p - 1) % passes], &deferred, 1));
            if (!deferred) return GD_OK;
            if (p > 4096) return set_err(h, GD_ETIMEOUT, "%s: the claims did not settle", call);
            HIP_TRY(h, hipMemsetAsync(&retry[p % passes], 0, 4, h->stream));
            GD_TRY(run(p, (const uint32_t*)nullptr, &retry[p % passes]));
        }
    }
    for (uint32_t p = 1; p < passes; ++p) GD_TRY(run(p, (const uint32_t*)&retry[p - 1], &retry[p]));
    *unsettled = &retry[passes - 1];
    return GD_OK;
}

// Room for `incoming` new entries at load <= 0.75, counting tombstones.  Without a read-back while the bound kept
// on the host (used_ub: every add since the last read-back counted as a new slot) allows it; else pull(live,
// tomb) reads the counters and, if need be, rebuild(cap, live) rebuilds the table: at the same capacity while the
// live entries fill at most half of it, else at double (and on until the batch fits).
template <typename Pull, typename Rebuild>
int table_reserve(gd_handle* h, uint64_t& used_ub, unsigned long long cap, uint64_t incoming, const char* call,
                  Pull pull, Rebuild rebuild) {
    if ((used_ub + incoming) * 4 <= cap * 3) {
        used_ub += incoming;
        return GD_OK;
    }
    GD_TRY(check_not_capturing(h, call));
    uint64_t live = 0, tomb = 0;
    GD_TRY(pull(live, tomb));
    if ((live + tomb + incoming) * 4 > cap * 3) {
        if (live * 2 > cap) cap *= 2;
        while ((live + incoming) * 4 > cap * 3) cap *= 2;
        GD_TRY(rebuild(cap, live));
        tomb = 0;
    }
    used_ub = live + tomb + incoming;
    return GD_OK;
}

// A zeroed table of `cap` slots of slot_bytes, the values beside them (side_bytes a slot) and two election
// words a slot: all three, or none and GD_EFULL.
inline int table_alloc(gd_handle* h, const char* what, unsigned long long cap, size_t slot_bytes, size_t side_bytes,
                       DevBuf& slots, DevBuf& side, DevBuf& last) {
    int r = ensure(h, slots, (size_t)cap * slot_bytes);
    if (r == GD_OK) r = ensure(h, side, (size_t)cap * side_bytes);
    if (r == GD_OK) r = ensure(h, last, (size_t)cap * 8);
    if (r != GD_OK) {
        free_buf(slots);
        free_buf(side);
        free_buf(last);
        return set_err(h, GD_EFULL, "%s table: no memory for %llu slots", what, cap);
    }
    HIP_TRY(h, hipMemsetAsync(slots.p, 0, (size_t)cap * slot_bytes, h->stream));
    HIP_TRY(h, hipMemsetAsync(last.p, 0, (size_t)cap * 8, h->stream));
    return GD_OK;
}

// The end of a rebuild: once the stream is done with the old table, the new buffers take its place.
inline int table_swap(gd_handle* h, DevBuf* const (&old)[3], const DevBuf (&fresh)[3], unsigned long long& cap,
                      unsigned long long new_cap) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < 3; ++k) {
        free_buf(*old[k]);
        *old[k] = fresh[k];
    }
    cap = new_cap;
    return GD_OK;
}

// Device error bits just read back are cleared (they are reported once); ERR_UNSETTLED among them: votes may be
// left in the election words (two a slot), which are zeroed.
inline int table_err_clear(gd_handle* h, uint32_t* d_err, uint32_t err, const DevBuf& last, unsigned long long cap) {
    HIP_TRY(h, hipMemsetAsync(d_err, 0, 4, h->stream));
    if (err & ERR_UNSETTLED) HIP_TRY(h, hipMemsetAsync(last.p, 0, (size_t)cap * 8, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GD_OK;
}

}  // namespace gdx