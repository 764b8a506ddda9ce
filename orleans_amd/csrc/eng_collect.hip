// eng_collect.hip -- libgraindispatch: the activation collector (gd_collect.h):
// Catalog/ActivationCollector.cs over per-context arrays -- idle tickets, the stale scan, the condemned list.
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_collect.h"

namespace {

constexpr uint64_t COL_MAX_QUANTA = 1ull << 28;

// The argument checks every call shares; the configuration is asked for after them.
int check_col(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const void* items, uint32_t n) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (!st) return set_err(h, GD_EINVAL, "null collector state");
    if (n_ctx && (!st->ticket || !st->became_idle || !st->age_limit || !st->flags))
        return set_err(h, GD_EINVAL, "null collector array");
    if (n && !items) return set_err(h, GD_EINVAL, "null argument");
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "collect: n > 2^31");
    if (n_ctx >= 0xFFFFFFFDu) return set_err(h, GD_EINVAL, "n_ctx too large");
    if (!h->col_quantum) return set_err(h, GD_ESTATE, "gd_collect_configure has not been called");
    return GD_OK;
}

int check_scan(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const void* ctx_flags, const void* num_running,
               const void* out_ctx, const void* out_n) {
    GD_TRY(check_col(h, st, n_ctx, nullptr, 0));
    if (!out_n) return set_err(h, GD_EINVAL, "null argument");
    if (n_ctx && (!ctx_flags || !num_running || !out_ctx)) return set_err(h, GD_EINVAL, "null context array");
    return GD_OK;
}

ColArgs col_args(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, int64_t now) {
    return ColArgs{st->ticket, st->became_idle, st->keep_alive_until, st->age_limit, st->flags,
                   h->col_quantum, h->col_next, now, n_ctx};
}

uint32_t stride_grid(gd_handle* h, uint64_t n) { return std::min<uint32_t>(blocks_for(n, BLOCK), h->n_cu * 16u); }

// The election words of the list forms: one a context, NONE32 between calls.
int elect_words(gd_handle* h, uint32_t n_ctx, uint32_t** win) {
    DevBuf& b = h->col_scr[0];
    const size_t need = (size_t)n_ctx * 4;
    const bool fresh = !(b.p && b.bytes >= need);
    GD_TRY(ensure(h, b, need));
    if (fresh) HIP_TRY(h, hipMemsetAsync(b.p, 0xFF, b.bytes, h->stream));
    *win = (uint32_t*)b.p;
    return GD_OK;
}

// The launches of a list form from its election to k_col_unelect.  If one of them fails the words may stay
// elected, so the buffer is dropped: the next list form allocates a new one and fills it with NONE32.
template <class F>
int elected(gd_handle* h, F&& launches) {
    const int rc = launches();
    if (rc != GD_OK) {
        (void)hipStreamSynchronize(h->stream);
        free_buf(h->col_scr[0]);
    }
    return rc;
}

int schedule_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint32_t* ctx, uint32_t n,
                    int64_t now, uint8_t* status) {
    if (!n) return GD_OK;
    StageTime stage(h, "stage:collect_schedule");
    uint32_t* win = nullptr;
    GD_TRY(elect_words(h, n_ctx, &win));
    const dim3 g(blocks_for(n, BLOCK)), b(BLOCK);
    const ColArgs a = col_args(h, st, n_ctx, now);
    return elected(h, [&]() -> int {
        GD_TRY(launch(h, "k_col_elect", g, b, 0, k_col_elect, ctx, n, n_ctx, win));
        GD_TRY(launch(h, "k_col_schedule", g, b, 0, k_col_schedule, a, ctx, n, (const uint32_t*)win, status));
        if (status)
            GD_TRY(launch(h, "k_col_schedule_dup", g, b, 0, k_col_schedule_dup, ctx, n, n_ctx, (const uint32_t*)win, status));
        return launch(h, "k_col_unelect", g, b, 0, k_col_unelect, ctx, n, n_ctx, win);
    });
}

int cancel_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint32_t* ctx, uint32_t n,
                  uint8_t* out) {
    if (!n) return GD_OK;
    StageTime stage(h, "stage:collect_cancel");
    uint32_t* win = nullptr;
    GD_TRY(elect_words(h, n_ctx, &win));
    const dim3 g(blocks_for(n, BLOCK)), b(BLOCK);
    return elected(h, [&]() -> int {
        GD_TRY(launch(h, "k_col_elect", g, b, 0, k_col_elect, ctx, n, n_ctx, win));
        GD_TRY(launch(h, "k_col_cancel", g, b, 0, k_col_cancel, col_args(h, st, n_ctx, 0), ctx, n, (const uint32_t*)win, out));
        return launch(h, "k_col_unelect", g, b, 0, k_col_unelect, ctx, n, n_ctx, win);
    });
}

int touch_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint8_t* ctx_flags,
                 const uint32_t* ctx, const uint8_t* turn, uint32_t n, int64_t now, uint8_t* ok) {
    StageTime stage(h, "stage:collect_touch");
    return launch(h, "k_col_touch", dim3(stride_grid(h, n)), dim3(BLOCK), 0, k_col_touch, col_args(h, st, n_ctx, now),
                  ctx_flags, ctx, turn, n, ok);
}

int idle_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint8_t* event, int64_t now,
                uint8_t* ok) {
    StageTime stage(h, "stage:collect_idle");
    return launch(h, "k_col_idle", dim3(stride_grid(h, n_ctx)), dim3(BLOCK), 0, k_col_idle, col_args(h, st, n_ctx, now),
                  event, ok);
}

// The quanta ScanStale dequeues at `now` (:166-190, :211).
int stale_quanta(gd_handle* h, int64_t now, uint64_t* n_q) {
    *n_q = h->col_next > now ? 0ull : (uint64_t)(now - h->col_next) / (uint64_t)h->col_quantum + 1ull;
    if (*n_q > COL_MAX_QUANTA) return set_err(h, GD_EINVAL, "gd_collect_scan_stale: more than 2^28 quanta to dequeue");
    return GD_OK;
}

// Both scans.  all: ScanAll with age_all; else ScanStale over n_q quanta from the handle's nextTicket, which the
// caller advances.
int scan_device_form(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, uint8_t* ctx_flags,
                     const uint32_t* num_running, const uint32_t* woff, int64_t now, bool all, int64_t age_all,
                     uint32_t n_q, uint32_t* out_ctx, uint32_t* out_n, uint8_t* verdict) {
    StageTime stage(h, all ? "stage:collect_scan_all" : "stage:collect_scan_stale");
    if (!n_ctx) {
        HIP_TRY(h, hipMemsetAsync(out_n, 0, 4, h->stream));
        return GD_OK;
    }
    DevBuf* S = h->col_scr;
    const uint32_t tiles = blocks_for(n_ctx, COL_TILE);
    const bool by_ticket = !all && n_q > 1;
    GD_TRY(ensure(h, S[1], ((size_t)tiles + 1) * 4));
    if (!verdict) {
        GD_TRY(ensure(h, S[2], n_ctx));
        verdict = (uint8_t*)S[2].p;
    }
    if (by_ticket) {
        GD_TRY(ensure(h, S[3], (size_t)n_ctx * 4));
        GD_TRY(ensure(h, S[4], ((size_t)n_q + 2) * 4));
    }
    uint32_t* tile_cnt = (uint32_t*)S[1].p;
    const ColArgs a = col_args(h, st, n_ctx, now);
    const ColScan s{ctx_flags, num_running, woff, h->col_next + (int64_t)n_q * h->col_quantum, age_all, n_q, verdict,
                    by_ticket ? (uint32_t*)S[3].p : nullptr};
    if (all) GD_TRY(launch(h, "k_col_scan_all", dim3(tiles), dim3(COL_NT), 0, k_col_scan<true>, a, s, tile_cnt, tiles));
    else GD_TRY(launch(h, "k_col_scan_stale", dim3(tiles), dim3(COL_NT), 0, k_col_scan<false>, a, s, tile_cnt, tiles));
    if (by_ticket) {
        // ascending ticket, then ascending context: the stable bucketing of every context by its quantum index,
        // the contexts that are not condemned in the trailing bucket n_q
        uint32_t* off = (uint32_t*)S[4].p;
        GD_TRY(bucket_device(h, (const uint32_t*)S[3].p, n_ctx, n_q, out_ctx, off));
        return launch(h, "k_col_total", dim3(1), dim3(WAVE), 0, k_col_total, (const uint32_t*)off, n_q, out_n);
    }
    GD_TRY(scan_device<OpAdd>(h, tile_cnt, tiles + 1, false, false, "collect"));
    return launch(h, "k_col_list", dim3(tiles), dim3(COL_NT), 0, k_col_list, (const uint8_t*)verdict, n_ctx,
                  (const uint32_t*)tile_cnt, tiles, out_ctx, out_n);
}

int count_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, int64_t now, int64_t shortest,
                 int64_t recency, uint64_t* out) {
    StageTime stage(h, "stage:collect_count");
    HIP_TRY(h, hipMemsetAsync(out, 0, 8, h->stream));
    return launch(h, "k_col_count", dim3(stride_grid(h, n_ctx)), dim3(BLOCK), 0, k_col_count, col_args(h, st, n_ctx, now),
                  shortest, recency, (unsigned long long*)out);
}

// The state's arrays of a host form on the device; back() brings down the ones a call may have written.
struct HostState {
    gd_collect_state d{};
    const gd_collect_state* st;
    uint32_t n_ctx;
    HostState(HostStage& io, const gd_collect_state* s, uint32_t n) : st(s), n_ctx(n) {
        d.ticket = const_cast<int64_t*>(io.in((const int64_t*)s->ticket, n));
        d.became_idle = const_cast<int64_t*>(io.in((const int64_t*)s->became_idle, n));
        d.keep_alive_until = io.in(s->keep_alive_until, n);
        d.age_limit = io.in(s->age_limit, n);
        d.flags = const_cast<uint8_t*>(io.in((const uint8_t*)s->flags, n));
    }
    int back(HostStage& io, bool ticket, bool idle, bool flags) {
        if (ticket) GD_TRY(io.fetch(st->ticket, d.ticket, n_ctx));
        if (idle) GD_TRY(io.fetch(st->became_idle, d.became_idle, n_ctx));
        if (flags) GD_TRY(io.fetch(st->flags, d.flags, n_ctx));
        return GD_OK;
    }
};

int scan_host_form(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, uint8_t* ctx_flags,
                   const uint32_t* num_running, const uint32_t* woff, int64_t now, bool all, int64_t age_all,
                   uint32_t* out_ctx, uint32_t* out_n, uint8_t* out_verdict, const char* call) {
    GD_TRY(check_scan(h, st, n_ctx, ctx_flags, num_running, out_ctx, out_n));
    uint64_t n_q = 0;
    if (!all) GD_TRY(stale_quanta(h, now, &n_q));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, call));
    HostStage io(h);
    HostState hs(io, st, n_ctx);
    uint8_t* dcf = const_cast<uint8_t*>(io.in((const uint8_t*)ctx_flags, n_ctx));
    const uint32_t* dnr = io.in(num_running, n_ctx);
    const uint32_t* dwo = io.in(woff, (size_t)n_ctx + 1);
    uint32_t* dout = io.hold<uint32_t>(n_ctx);
    uint32_t* dn = io.out(out_n, 1);
    uint8_t* dv = io.out_if(out_verdict, n_ctx);
    GD_TRY(io.status());
    GD_TRY(scan_device_form(h, &hs.d, n_ctx, dcf, dnr, dwo, now, all, age_all, (uint32_t)n_q, dout, dn, dv));
    h->col_next += (int64_t)n_q * h->col_quantum;
    GD_TRY(hs.back(io, !all, false, true));
    GD_TRY(io.fetch(ctx_flags, dcf, n_ctx));
    GD_TRY(io.fetch());
    GD_TRY(sync_checked(h));
    GD_TRY(io.fetch(out_ctx, dout, std::min(*out_n, n_ctx)));
    return sync_checked(h);
}

}  // namespace

extern "C" {

int gd_collect_configure(gd_handle* h, int64_t quantum_ticks, int64_t now) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (quantum_ticks <= 0) return set_err(h, GD_EINVAL, "gd_collect_configure: the quantum is not positive");
    h->col_quantum = quantum_ticks;
    h->col_next = ((now - 1) / quantum_ticks + 1) * quantum_ticks;   // MakeTicketFromDateTime (:37, :371)
    return GD_OK;
}

int gd_collect_next_ticket(gd_handle* h, int64_t* out) {
    if (!h) return set_err(nullptr, GD_EINVAL, "null handle");
    if (!out) return set_err(h, GD_EINVAL, "null argument");
    if (!h->col_quantum) return set_err(h, GD_ESTATE, "gd_collect_configure has not been called");
    *out = h->col_next;
    return GD_OK;
}

int gd_collect_schedule_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint32_t* d_ctx,
                               uint32_t n, int64_t now, uint8_t* d_status) {
    GD_TRY(check_col(h, st, n_ctx, d_ctx, n));
    HIP_TRY(h, hipSetDevice(h->device));
    return schedule_device(h, st, n_ctx, d_ctx, n, now, d_status);
}

int gd_collect_schedule(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint32_t* ctx, uint32_t n,
                        int64_t now, uint8_t* out_status) {
    GD_TRY(check_col(h, st, n_ctx, ctx, n));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_collect_schedule"));
    HostStage io(h);
    HostState hs(io, st, n_ctx);
    const uint32_t* dctx = io.in(ctx, n);
    uint8_t* dst = io.out_if(out_status, n);
    GD_TRY(io.status());
    GD_TRY(schedule_device(h, &hs.d, n_ctx, dctx, n, now, dst));
    GD_TRY(hs.back(io, true, false, true));
    GD_TRY(io.fetch());
    return sync_checked(h);
}

int gd_collect_cancel_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint32_t* d_ctx,
                             uint32_t n, uint8_t* d_cancelled) {
    GD_TRY(check_col(h, st, n_ctx, d_ctx, n));
    HIP_TRY(h, hipSetDevice(h->device));
    return cancel_device(h, st, n_ctx, d_ctx, n, d_cancelled);
}

int gd_collect_cancel(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint32_t* ctx, uint32_t n,
                      uint8_t* out_cancelled) {
    GD_TRY(check_col(h, st, n_ctx, ctx, n));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_collect_cancel"));
    HostStage io(h);
    HostState hs(io, st, n_ctx);
    const uint32_t* dctx = io.in(ctx, n);
    uint8_t* dout = io.out_if(out_cancelled, n);
    GD_TRY(io.status());
    GD_TRY(cancel_device(h, &hs.d, n_ctx, dctx, n, dout));
    GD_TRY(hs.back(io, false, false, true));
    GD_TRY(io.fetch());
    return sync_checked(h);
}

int gd_collect_touch_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint8_t* d_ctx_flags,
                            const uint32_t* d_ctx, const uint8_t* d_turn, uint32_t n, int64_t now, uint8_t* d_ok) {
    GD_TRY(check_col(h, st, n_ctx, d_ctx, n));
    if (n && n_ctx && !d_ctx_flags) return set_err(h, GD_EINVAL, "null context array");
    HIP_TRY(h, hipSetDevice(h->device));
    return touch_device(h, st, n_ctx, d_ctx_flags, d_ctx, d_turn, n, now, d_ok);
}

int gd_collect_touch(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint8_t* ctx_flags,
                     const uint32_t* ctx, const uint8_t* turn, uint32_t n, int64_t now, uint8_t* out_ok) {
    GD_TRY(check_col(h, st, n_ctx, ctx, n));
    if (n && n_ctx && !ctx_flags) return set_err(h, GD_EINVAL, "null context array");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_collect_touch"));
    HostStage io(h);
    HostState hs(io, st, n_ctx);
    const uint8_t* dcf = io.in(ctx_flags, n_ctx);
    const uint32_t* dctx = io.in(ctx, n);
    const uint8_t* dturn = io.in(turn, n);
    uint8_t* dok = io.out_if(out_ok, n);
    GD_TRY(io.status());
    GD_TRY(touch_device(h, &hs.d, n_ctx, dcf, dctx, dturn, n, now, dok));
    GD_TRY(hs.back(io, true, false, false));
    GD_TRY(io.fetch());
    return sync_checked(h);
}

int gd_collect_idle_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint8_t* d_event,
                           int64_t now, uint8_t* d_ok) {
    GD_TRY(check_col(h, st, n_ctx, d_event, n_ctx));
    HIP_TRY(h, hipSetDevice(h->device));
    return idle_device(h, st, n_ctx, d_event, now, d_ok);
}

int gd_collect_idle(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint8_t* event, int64_t now,
                    uint8_t* out_ok) {
    GD_TRY(check_col(h, st, n_ctx, event, n_ctx));
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_collect_idle"));
    HostStage io(h);
    HostState hs(io, st, n_ctx);
    const uint8_t* dev = io.in(event, n_ctx);
    uint8_t* dok = io.out_if(out_ok, n_ctx);
    GD_TRY(io.status());
    GD_TRY(idle_device(h, &hs.d, n_ctx, dev, now, dok));
    GD_TRY(hs.back(io, true, true, false));
    GD_TRY(io.fetch());
    return sync_checked(h);
}

int gd_collect_scan_stale_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, uint8_t* d_ctx_flags,
                                 const uint32_t* d_num_running, const uint32_t* d_wait_offsets, int64_t now,
                                 uint32_t* d_out_ctx, uint32_t* d_out_n, uint8_t* d_verdict) {
    GD_TRY(check_scan(h, st, n_ctx, d_ctx_flags, d_num_running, d_out_ctx, d_out_n));
    uint64_t n_q = 0;
    GD_TRY(stale_quanta(h, now, &n_q));
    HIP_TRY(h, hipSetDevice(h->device));
    if (n_q > 1 && n_ctx) GD_TRY(check_not_capturing(h, "gd_collect_scan_stale_device over more than one quantum"));
    GD_TRY(scan_device_form(h, st, n_ctx, d_ctx_flags, d_num_running, d_wait_offsets, now, false, 0, (uint32_t)n_q,
                            d_out_ctx, d_out_n, d_verdict));
    h->col_next += (int64_t)n_q * h->col_quantum;
    return GD_OK;
}

int gd_collect_scan_stale(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, uint8_t* ctx_flags,
                          const uint32_t* num_running, const uint32_t* wait_offsets, int64_t now, uint32_t* out_ctx,
                          uint32_t* out_n, uint8_t* out_verdict) {
    return scan_host_form(h, st, n_ctx, ctx_flags, num_running, wait_offsets, now, false, 0, out_ctx, out_n,
                          out_verdict, "gd_collect_scan_stale");
}

int gd_collect_scan_all_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, uint8_t* d_ctx_flags,
                               const uint32_t* d_num_running, const uint32_t* d_wait_offsets, int64_t now,
                               int64_t age_limit_ticks, uint32_t* d_out_ctx, uint32_t* d_out_n, uint8_t* d_verdict) {
    GD_TRY(check_scan(h, st, n_ctx, d_ctx_flags, d_num_running, d_out_ctx, d_out_n));
    HIP_TRY(h, hipSetDevice(h->device));
    return scan_device_form(h, st, n_ctx, d_ctx_flags, d_num_running, d_wait_offsets, now, true, age_limit_ticks, 0,
                            d_out_ctx, d_out_n, d_verdict);
}

int gd_collect_scan_all(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, uint8_t* ctx_flags,
                        const uint32_t* num_running, const uint32_t* wait_offsets, int64_t now,
                        int64_t age_limit_ticks, uint32_t* out_ctx, uint32_t* out_n, uint8_t* out_verdict) {
    return scan_host_form(h, st, n_ctx, ctx_flags, num_running, wait_offsets, now, true, age_limit_ticks, out_ctx,
                          out_n, out_verdict, "gd_collect_scan_all");
}

int gd_collect_count_recent_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, int64_t now,
                                   int64_t shortest_age_limit, int64_t recency, uint64_t* d_count) {
    GD_TRY(check_col(h, st, n_ctx, nullptr, 0));
    if (!d_count) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return count_device(h, st, n_ctx, now, shortest_age_limit, recency, d_count);
}

int gd_collect_count_recent(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, int64_t now,
                            int64_t shortest_age_limit, int64_t recency, uint64_t* out_count) {
    GD_TRY(check_col(h, st, n_ctx, nullptr, 0));
    if (!out_count) return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_collect_count_recent"));
    HostStage io(h);
    HostState hs(io, st, n_ctx);
    uint64_t* dc = io.out(out_count, 1);
    GD_TRY(io.status());
    GD_TRY(count_device(h, &hs.d, n_ctx, now, shortest_age_limit, recency, dc));
    GD_TRY(io.fetch());
    return sync_checked(h);
}

}  // extern "C"
