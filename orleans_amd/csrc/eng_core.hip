// eng_core.hip -- libgraindispatch: scratch, the probe index and measured choices, table growth, the exchange partition.
// The route launches: eng_route.hip; the scans and the bucketing: eng_bucket.hip.
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"


namespace gdx {

thread_local std::string g_tls_error = "";



}  // namespace gdx


namespace gdx {

int set_err(gd_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    g_tls_error = buf;
    return code;
}


// A bucketing gd_route_bucket_device left running on the bucket stream (gd_set_bucket_stream) uses the
// handle's scratch (u32_a..d, hist, partials, m3): every entry point that takes scratch on the handle's
// own stream waits for it first (ensure() calls this).  The route itself takes no scratch,
// so the next batch's route still overlaps this batch's bucketing.
int bfence(gd_handle* h) {
    if (!h->b_pending || !h->bstream || h->bstream == h->stream) return GD_OK;
    HIP_TRY(h, hipEventRecord(h->b_fence_ev, h->bstream));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->b_fence_ev, 0));
    h->b_pending = false;
    return GD_OK;
}

int ensure(gd_handle* h, DevBuf& b, size_t bytes) {
    GD_TRY(bfence(h));
    return ensure_own(h, b, bytes);
}

// ensure() for a buffer no bucketing touches (the directory batches' dir_scr): no bfence.
int ensure_own(gd_handle* h, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return GD_OK;
    if (b.p) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
    }
    size_t want = std::max<size_t>(bytes, 256);
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) return set_err(h, GD_ENOMEM, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
    b.bytes = want;
    return GD_OK;
}

void free_buf(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

int name_id(gd_handle* h, const char* name) {
    for (size_t i = 0; i < h->tnames.size(); ++i)
        if (h->tnames[i] == name) return (int)i;
    h->tnames.emplace_back(name);
    h->tms.push_back(0.0);
    h->tcount.push_back(0);
    return (int)h->tnames.size() - 1;
}

hipEvent_t take_event(gd_handle* h) {
    if (!h->event_pool.empty()) {
        hipEvent_t e = h->event_pool.back();
        h->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}


int resolve_timing(gd_handle* h) {
    if (h->pending.empty()) return GD_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->bstream) HIP_TRY(h, hipStreamSynchronize(h->bstream));
    if (h->xstream) HIP_TRY(h, hipStreamSynchronize(h->xstream));
    if (h->pstream) HIP_TRY(h, hipStreamSynchronize(h->pstream));
    for (auto& t : h->pending) {
        float ms = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms, t.a, t.b));
        h->tms[t.name] += ms;
        h->tcount[t.name] += 1;
        h->event_pool.push_back(t.a);
        h->event_pool.push_back(t.b);
    }
    h->pending.clear();
    return GD_OK;
}


int check_ring(gd_handle* h) {
    if (h->ring_mode < 0 || h->ring_n == 0) return set_err(h, GD_ESTATE, "no ring installed (gd_ring_set)");
    return GD_OK;
}

RingArgs ring_args(gd_handle* h) {
    return RingArgs{(const uint32_t*)h->ring_pts.p, (const uint32_t*)h->ring_own.p, h->ring_n, h->ring_top,
                    h->cfg.my_silo, h->cfg.seed_silo};
}

TableArgs table_args(gd_handle* h) {
    return TableArgs{h->slots, h->capacity - 1, h->ctr, (const uint32_t*)h->dir_valid.p, h->n_valid};
}

bool host_silo_valid(const gd_handle* h, uint32_t silo) {
    return h->n_valid == 0 || silo >= h->n_valid || h->valid_host[silo];
}

size_t ring_lds(gd_handle* h) { return (size_t)h->ring_n * 2 * sizeof(uint32_t); }

// The striped live / tomb deltas (gd_hash.h CTR_STRIPES) into the counters, before a read-back.
int fold_counters(gd_handle* h, DevCounters* c) {
    hipLaunchKernelGGL(k_ctr_fold, dim3(1), dim3(64), 0, h->stream, c);
    HIP_TRY(h, hipGetLastError());
    return GD_OK;
}

int pull_counters(gd_handle* h) {
    GD_TRY(fold_counters(h, h->ctr));
    HIP_TRY(h, hipMemcpyAsync(&h->ctr_host, h->ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, h->stream));
    if (h->cx_built && h->cxi_ctr.p)   // the index counters ride along (cx_ensure's rebuild rule)
        HIP_TRY(h, hipMemcpyAsync(&h->cx_ctr_host, h->cxi_ctr.p, sizeof(CxCounters), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->ctr_stale = false;
    h->pending_in = 0;
    // every batch enqueued so far is done: the index is pure again if no batch left anything out
    if (h->tab_track == 0 && h->cx_built && h->cxi_ctr.p)
        h->cx8_pure = h->cx8_ok && h->cx8_layout.ntypes == 1 && h->cx_ctr_host.out8 == 0;
    return GD_OK;
}

int alloc_table(gd_handle* h, unsigned long long cap, Slot** out) {
    if (cap > (1ull << 32)) return set_err(h, GD_EINVAL, "table of %llu slots: at most 2^32 (home_slot)", cap);
    Slot* s = nullptr;
    hipError_t e = hipMalloc(&s, cap * sizeof(Slot));
    if (e != hipSuccess) return set_err(h, GD_ENOMEM, "table hipMalloc(%llu slots): %s", cap, hipGetErrorString(e));
    e = hipMemsetAsync(s, 0, cap * sizeof(Slot), h->stream);
    if (e != hipSuccess) {
        (void)hipFree(s);
        return set_err(h, GD_EHIP, "table memset: %s", hipGetErrorString(e));
    }
    *out = s;
    return GD_OK;
}

int alloc_vtag(gd_handle* h, unsigned long long cap, uint32_t** out) {
    uint32_t* v = nullptr;
    hipError_t e = hipMalloc(&v, cap * sizeof(uint32_t));
    if (e != hipSuccess) return set_err(h, GD_ENOMEM, "version tags hipMalloc(%llu): %s", cap, hipGetErrorString(e));
    e = hipMemsetAsync(v, 0, cap * sizeof(uint32_t), h->stream);
    if (e != hipSuccess) {
        (void)hipFree(v);
        return set_err(h, GD_EHIP, "version tags memset: %s", hipGetErrorString(e));
    }
    *out = v;
    return GD_OK;
}

unsigned long long pow2_at_least(unsigned long long x) {
    unsigned long long c = 1024;
    while (c < x) c <<= 1;
    return c;
}

// ---- compact probe indexes (gd_cx.h) ----------------------------------------------
bool cx_current(const gd_handle* h) {
    return h->cx_built && h->cx_slots_at == h->slots && h->cx_cap_at == h->capacity && h->cx_gen_at == h->tab_gen;
}

TabTrack::TabTrack(gd_handle* hh) : h(hh), was_current(cx_current(hh)) {
    ++h->tab_track;
    h->cx8_pure = false;                 // until a read-back after the batch shows the index still pure
    h->cx_snap++;                        // the direct table, if any, is stale from here on
}

static uint32_t bit_len(uint64_t x) {
    uint32_t b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

CxBuild cx_build_args(gd_handle* h) {
    return CxBuild{(uint4*)h->cxi_tab.p, (unsigned long long*)h->cxi_types.p,
                   h->cx8_ok ? (unsigned long long*)h->cx8_tab.p : nullptr, h->cx8_layout};
}

// Grid of the table-wide index passes: CXT_IT slots a thread a round, at most 16 workgroups a CU.
static uint32_t cx_grid(gd_handle* h) {
    return std::max<uint32_t>(1, std::min<uint64_t>(blocks_for(h->capacity, BLOCK * CXT_IT), (uint64_t)h->n_cu * 16));
}

// The full build: k_cx_types, one read-back (types, counts, widths), the 8-B layout, k_cx_project.
// The 8-B index takes the most populous types (up to CX8_TYPES) and the activation / silo widths of the
// live entries; fewer types when the three fields would not fit 31 bits, narrower activations last
// (wider ones are then redirect entries: their keys probe the directory).
static int cx_build(gd_handle* h) {
    const auto t0 = std::chrono::steady_clock::now();
    const unsigned long long cap = h->capacity;
    GD_TRY(ensure(h, h->cxi_tab, cap * 16));
    GD_TRY(ensure(h, h->cx8_tab, cap * 8));
    GD_TRY(ensure(h, h->cxi_types, CX_TYPES * 12));
    GD_TRY(ensure(h, h->cxi_ctr, sizeof(CxCounters)));
    unsigned long long* types = (unsigned long long*)h->cxi_types.p;
    uint32_t* counts = (uint32_t*)(types + CX_TYPES);
    CxCounters* ctr = (CxCounters*)h->cxi_ctr.p;
    HIP_TRY(h, hipMemsetAsync(types, 0xFF, CX_TYPES * 8, h->stream));
    HIP_TRY(h, hipMemsetAsync(counts, 0, CX_TYPES * 4, h->stream));
    HIP_TRY(h, hipMemsetAsync(ctr, 0, sizeof(CxCounters), h->stream));
    const dim3 g(cx_grid(h)), b(BLOCK);
    GD_TRY(launch(h, "k_cx_types", g, b, 0, k_cx_types, (const Slot*)h->slots, cap, types, counts, ctr));
    CxCounters c{};
    unsigned long long ht[CX_TYPES];
    uint32_t hc[CX_TYPES];
    HIP_TRY(h, hipMemcpyAsync(&c, ctr, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(ht, types, sizeof ht, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(hc, counts, sizeof hc, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<std::pair<uint32_t, unsigned long long>> by_count;
    for (uint32_t t = 0; t < CX_TYPES; ++t)
        if (ht[t] != CX_NO_TYPE) by_count.emplace_back(hc[t], ht[t]);
    std::stable_sort(by_count.begin(), by_count.end(),
                     [](const auto& x, const auto& y) { return x.first > y.first; });
    uint32_t n8 = (uint32_t)std::min<size_t>(CX8_TYPES, by_count.size());
    uint32_t ab = std::max<uint32_t>(2, bit_len((uint64_t)c.act_max + 2));
    const uint32_t sb = std::max<uint32_t>(1, bit_len((uint64_t)c.silo_max + 1));
    for (;;) {
        const uint32_t tb = n8 > 1 ? bit_len(n8 - 1) : 0;
        if (ab + sb + tb <= 31) break;
        if (tb > 0) {
            n8 = 1u << (tb - 1);                       // fewer types before narrower activations
            continue;
        }
        ab = sb + tb >= 29 ? 0 : 31 - sb - tb;
        break;
    }
    Cx8Args p8{};
    p8.slots = (const uint4*)h->cx8_tab.p;
    p8.cap = cap;
    p8.ntypes = n8;
    for (uint32_t k = 0; k < n8; ++k) p8.tcd[k] = by_count[k].second;
    p8.ab = ab;
    p8.sb = sb;
    h->cx8_layout = p8;
    h->cx8_ok = ab >= 2;
    uint32_t held8 = 0;
    for (uint32_t k = 0; k < n8; ++k) held8 += by_count[k].first;
    h->cx_held8_at = held8;
    GD_TRY(launch(h, "k_cx_project", g, b, 0, k_cx_project, (const Slot*)h->slots, cap, cx_build_args(h), ctr));
    HIP_TRY(h, hipMemcpyAsync(&h->cx_ctr_host, ctr, sizeof(CxCounters), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->cx_ok = true;
    h->cx_built = true;
    h->cx_out8_at = h->cx_ctr_host.out8;              // the build's own: the baseline of the rebuild rule
    h->cx8_pure = h->cx8_ok && h->cx8_layout.ntypes == 1 && h->cx_ctr_host.out8 == 0;
    h->cx_builds++;
    h->cx_snap++;                                     // the 8-B index was re-laid
    h->cx_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GD_OK;
}

// Re-projects the slots a directory batch touched (slot_of[n]) when the indexes were current before it.
// Only enqueued: its counters come back with the next pull_counters, and when the batches' new entries
// no longer fit the 8-B layout (a new grain class, wider activations or silos) beyond an eighth of the
// entries it held, cx_ensure rebuilds with a new layout.
int cx_sync(gd_handle* h, TabTrack& tt, const uint32_t* slot_of, uint32_t n) {
    tt.synced = true;
    if (!tt.was_current || n == 0) return GD_OK;   // a stale index stays stale: the next large route rebuilds
    GD_TRY(launch(h, "k_cx_sync", dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, k_cx_sync, slot_of, n,
                  (const Slot*)h->slots, cx_build_args(h), (CxCounters*)h->cxi_ctr.p));
    h->cx_synced += n;
    return GD_OK;
}

// A directory batch that projects its slots inside its commit kernel: true (and the batch counted as
// synced) when the indexes were current before it; false leaves a stale index stale.
bool cx_inline(gd_handle* h, TabTrack& tt, uint32_t n) {
    tt.synced = true;
    if (!tt.was_current || !h->cx_ok) return false;
    h->cx_synced += n;
    return true;
}

// The index for the current table: rebuilt (two streaming passes + one host sync) when the table
// changed since the last build by a write that did not re-project its slots (gd_dir_rehash, clear,
// merge, silo removal, split, handoff); false when GD_OPT_PROBE = 0.  n: the messages of the launch
// asking.  A stale index is rebuilt only for a launch of at least capacity / 16 messages: a small route
// after such a change takes the directory probe instead of a full-table pass and a host sync (ADVICE
// r03); the next large launch rebuilds.
int cx_ensure(gd_handle* h, bool* ok, uint64_t n) {
    *ok = false;
    if (!h->cx_mode || !h->slots || h->capacity < CX8_GROUP) return GD_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;   // a captured graph keeps the directory probe
    HIP_TRY(h, hipStreamIsCapturing(h->stream, &cs));
    if (cs != hipStreamCaptureStatusNone) return GD_OK;
    if (cx_current(h)) {
        const CxCounters& c = h->cx_ctr_host;
        if (!(h->cx8_ok && c.out8 > h->cx_out8_at && c.out8 - h->cx_out8_at > h->cx_held8_at / 8 + 4096)) {
            *ok = h->cx_ok;
            return GD_OK;
        }
        h->tab_gen++;                               // the 8-B layout no longer fits the directory: rebuild
    }
    if (h->cx_mode == 1 && n < h->capacity / 16) return GD_OK;
    GD_TRY(cx_build(h));
    for (auto& kt : h->cx_tune) {                   // a new table: measure the probes again (not the bucketing)
        if (kt.first / (64 * 32) == GD_TUNE_BUCKET) continue;
        auto& t = kt.second;
        for (int v = 0; v < gd_handle::CXV; ++v) {
            if (t.pending[v]) (void)hipEventSynchronize(t.b[v]);
            t.best[v] = 1e30f;
            t.pending[v] = false;
        }
        t.pick = -1;
        t.round = 0;
    }
    h->cx_slots_at = h->slots;
    h->cx_cap_at = h->capacity;
    h->cx_gen_at = h->tab_gen;
    *ok = h->cx_ok;
    return GD_OK;
}

// The probe variant for a launch of `kind` (0 keys, 1 N1s, 2 fan-out, 3 node ids) over n messages when
// the index is available: 0 the index read in 64-B groups, 1 the directory, 2 the index read one 16-B
// slot at a time.  GD_CX=2: always 0.  GD_CX=1 times the three on the first six eligible launches of the
// kind and size class (bit length of n: the fan-out's hops differ 10x in size, and per-message cost
// with them), twice each in turn, between HIP events read back without a stream sync at the next
// choice, and keeps the fastest per message.  All give the same results; which is fastest depends on
// the key distribution (a Zipf-hot set favours small reads, a uniform one the index's group reads,
// DESIGN 5).  nvar: the variants this launch kind has (2: no 16-B-read form).  *meas: the tune entry
// this launch is timed into (key * CXV + variant), or -1.
// The tune entry's key: kind, size class (bit length of n), a second shape class.
int tune_key(int kind, uint64_t n, int sub) {
    int cls = 0;
    while (cls < 63 && (n >> cls) > 1) ++cls;
    return (kind * 64 + cls) * 32 + std::max(0, std::min(31, sub));
}

// Variants of a tune kind (GD_TUNE_*): the 24-B-key and N1 probes have three, the rest two.
int tune_nvar(int kind) { return kind <= 1 ? 4 : (kind <= 3 ? 3 : 2); }

// Variants a launch of `kind` has on this handle now: kinds 0 / 1 and 2 / 3 have the 8-B index as their
// last variant only where it is built (cx_ensure), kind 4 (the bucketing form) always two.
int tune_nvar_now(const gd_handle* h, int kind) {
    if (kind <= 1) return h->cx8_ok ? 4 : 3;
    if (kind <= 3) return h->cx8_ok ? 3 : 2;
    return 2;
}

// Folds the entry's finished timings in (events read without a stream sync, unless the entry has
// timed every variant twice and only waits for them) and picks when every variant is timed.
void tune_resolve(gd_handle::CxTune& t, int nvar) {
    constexpr int V = gd_handle::CXV;
    bool any_pending = false;
    for (int v = 0; v < V; ++v) {
        if (!t.pending[v]) continue;
        if (hipEventQuery(t.b[v]) != hipSuccess && t.pick < 0 && t.round >= 2 * nvar) (void)hipEventSynchronize(t.b[v]);
        if (hipEventQuery(t.b[v]) == hipSuccess) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, t.a[v], t.b[v]) == hipSuccess && t.n[v])
                t.best[v] = std::min(t.best[v], ms / (float)t.n[v]);
            t.pending[v] = false;
        }
        any_pending = any_pending || t.pending[v];
    }
    if (t.pick < 0 && t.round >= 2 * nvar && !any_pending) {
        t.pick = 0;
        for (int v = 1; v < nvar; ++v)
            if (t.best[v] < t.best[t.pick]) t.pick = v;
    }
}

// The probe variant for a launch of `kind` (0 keys, 1 N1s, 2 fan-out, 3 node ids) over n messages when
// the index is available: 0 the index read in 64-B groups, 1 the directory, 2 the index read one 16-B
// slot at a time; kind 4: the bucketing form.  A variant pinned by gd_tune_set is taken at once.
// Else the first launches of the kind and size class (bit length of n: the fan-out's hops differ 10x
// in size, and per-message cost with them) time the variants, twice each in turn, between HIP events
// read back without a stream sync at the next choice, and the fastest per message is kept (or the one
// gd_tune_agree settled on).  All give the same results; which is fastest depends on the key
// distribution (a Zipf-hot set favours small reads, a uniform one the index's group reads).
// nvar: the variants this launch kind has.  *meas: the tune entry this launch is timed into
// (key * CXV + variant), or -1.
int tune_choose(gd_handle* h, int kind, uint64_t n, int* meas, int nvar, int sub) {
    constexpr int V = gd_handle::CXV;
    *meas = -1;
    if (h->tune_pin[kind] >= 0 && h->tune_pin[kind] < nvar) return h->tune_pin[kind];
    const int key = tune_key(kind, n, sub);
    auto& t = h->cx_tune[key];
    if (t.pick >= nvar || (t.pick < 0 && t.nvar && t.nvar != nvar)) {
        // a pick (gd_tune_agree's, or this entry's own) of a variant this launch does not have -- the
        // 8-B index not built here, or no longer -- or timings taken over another variant set: measure
        // again over the variants this launch has
        for (int v = 0; v < V; ++v) {
            if (t.pending[v] && t.b[v]) (void)hipEventSynchronize(t.b[v]);
            t.pending[v] = false;
            t.best[v] = 1e30f;
            t.n[v] = 0;
        }
        t.pick = -1;
        t.round = 0;
    }
    t.nvar = nvar;
    tune_resolve(t, nvar);
    if (t.pick >= 0) return t.pick;
    const int v = t.round % nvar;
    if (t.round < 2 * nvar && !t.pending[v]) {
        if (!t.a[v]) (void)hipEventCreate(&t.a[v]);
        if (!t.b[v]) (void)hipEventCreate(&t.b[v]);
        *meas = key * V + v;
        ++t.round;
        h->measured_launch = true;
    }
    return v;
}

int cx_choose(gd_handle* h, int kind, uint64_t n, int* meas, int nvar) {
    *meas = -1;
    // variants: 0 index groups, 1 directory; kinds 0 / 1: 2 index slots, 3 the 8-B index; kinds 2 / 3:
    // 2 the 8-B index (when built: nvar says)
    if (h->cx_mode == 2) return 0;
    if (h->cx_mode == 3) return kind <= 1 && nvar > 2 ? 2 : 0;
    if (h->cx_mode == 4) return kind <= 1 ? (nvar > 3 ? 3 : 0) : ((kind == 2 || kind == 3) && nvar > 2 ? 2 : 0);
    return tune_choose(h, kind, n, meas, nvar);
}


Cx8Args cx8_args(gd_handle* h) { return h->cx8_layout; }

CxArgs cx_args(gd_handle* h) {
    return CxArgs{(const uint4*)h->cxi_tab.p, h->capacity, (const unsigned long long*)h->cxi_types.p};
}


int sync(gd_handle* h) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->bstream && h->bstream != h->stream) HIP_TRY(h, hipStreamSynchronize(h->bstream));
    return GD_OK;
}

// h->h_pin holds at least `bytes` (page-locked: the small read-backs are true async copies).
int pinned_scratch(gd_handle* h, size_t bytes) {
    if (h->h_pin_bytes >= bytes) return GD_OK;
    if (h->h_pin) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipHostFree(h->h_pin));
        h->h_pin = nullptr;
        h->h_pin_bytes = 0;
    }
    const size_t b = std::max<size_t>(bytes, 64 * 1024);
    HIP_TRY(h, hipHostMalloc(&h->h_pin, b));
    h->h_pin_bytes = b;
    return GD_OK;
}

// A call that reads back, grows scratch or times its variants is refused inside a hipGraph capture, before
// anything is launched.
int check_not_capturing(gd_handle* h, const char* call) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(h, hipStreamIsCapturing(h->stream, &cs));
    if (cs != hipStreamCaptureStatusNone) return set_err(h, GD_ESTATE, "%s inside a stream capture", call);
    return GD_OK;
}

// `words` u32 words at device address d through the pinned scratch; the stream is idle on return.
int read_back(gd_handle* h, const void* d, uint32_t* out, size_t words) {
    GD_TRY(pinned_scratch(h, words * 4));
    HIP_TRY(h, hipMemcpyAsync(h->h_pin, d, words * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    memcpy(out, h->h_pin, words * 4);
    return GD_OK;
}

// The device error bits of the last counter read-back (pull_counters) as the call's result: cleared on
// the device, so each error is reported once.
int report_device_error(gd_handle* h) {
    const uint32_t e = h->ctr_host.err;
    if (!e) return GD_OK;
    HIP_TRY(h, hipMemsetAsync(&h->ctr->err, 0, sizeof(uint32_t), h->stream));
    GD_TRY(sync(h));
    if (e == ERR_CTX_RANGE)
        return set_err(h, GD_EINVAL, "an ActivationDirectory entry's context index is not below n_ctx");
    if (e == 128u)   // ERR_ENC_FULL (gd_frameout.h)
        return set_err(h, GD_EFULL, "gd_encode_frames: the encoded frames need more than out_cap bytes (out_off[n])");
    if (e == 256u)   // ERR_SNIFF_FULL (gd_sniff.h)
        return set_err(h, GD_EFULL, "gd_sniff_frames: the batch holds more than ent_cap entries (ent_off[n])");
    if (e & 2u) return set_err(h, GD_EFULL, "the directory table is full (device error bits 0x%x)", e);
    if (e & 4u)
        return set_err(h, GD_EINVAL, "a registration's silo index is above 0xFFFE (device error bits 0x%x)", e);
    if (e & ERR_UNSETTLED)
        return set_err(h, GD_ETIMEOUT, "an asynchronous registration's claims did not settle (device error bits 0x%x)", e);
    return set_err(h, GD_EFULL, "device error bits 0x%x", e);
}

// Surface device-side error bits after a synchronising call.
int sync_checked(gd_handle* h) {
    GD_TRY(pull_counters(h));
    return report_device_error(h);
}

// maybe_grow_table without the read-back while the last copy of the counters is current (no untracked
// table write since) and, with every asynchronous registration since counted as new entries, the table
// stays at load <= 0.75.
int maybe_grow_async(gd_handle* h, uint64_t incoming) {
    if (!h->ctr_stale) {
        const unsigned long long used = h->ctr_host.live + h->ctr_host.tomb + h->pending_in + incoming;
        if (used * 4 <= h->capacity * 3) return GD_OK;
    }
    return maybe_grow_table(h, incoming);
}

int maybe_grow_table(gd_handle* h, uint64_t incoming) {
    GD_TRY(pull_counters(h));
    return grow_table(h, incoming);
}

// maybe_grow_table after a read-back of the counters (pull_counters, sync_checked) with nothing enqueued since.
int grow_table(gd_handle* h, uint64_t incoming) {
    const unsigned long long used = h->ctr_host.live + h->ctr_host.tomb + incoming;
    if (used * 4 <= h->capacity * 3) return GD_OK;  // keep load <= 0.75
    unsigned long long cap = h->capacity;
    while ((h->ctr_host.live + incoming) * 2 > cap) cap <<= 1;
    return gd_dir_rehash(h, cap);
}

// ---- exchange partition (gd_shard.h) -------------------------------------------------
template <int MODE, bool NODES>
int shard_hist_t(gd_handle* h, const void* recs, uint32_t n, uint64_t tcd, uint32_t n_shards, uint32_t bits,
                 uint32_t tiles, uint8_t* dest, uint32_t* hist, const ExtArgs& ext, uint32_t* kdesc, uint32_t regions) {
    uint32_t* n1lo = !NODES && kdesc && h->shard_n1_copy ? (uint32_t*)h->shard_n1.p : nullptr;
    if (!NODES && !ext.len)           // no KeyExt strings in the batch: the instantiation without their path
        return launch(h, "k_shard_hist", dim3(tiles), dim3(SH_NT), ring_lds(h), k_shard_hist<MODE, NODES, false>, recs,
                      n, tcd, ring_args(h), n_shards, bits, tiles, dest, hist, ext, kdesc, n1lo, regions);
    return launch(h, "k_shard_hist", dim3(tiles), dim3(SH_NT), ring_lds(h), k_shard_hist<MODE, NODES>, recs, n, tcd,
                  ring_args(h), n_shards, bits, tiles, dest, hist, ext, kdesc, n1lo, regions);
}

template <int BITS, bool NODES>
int shard_scatter_t(gd_handle* h, const void* recs, const uint32_t* payload, const uint8_t* dest, uint32_t n,
                    uint32_t n_shards, uint32_t tiles, const uint32_t* gscan, void* out, uint32_t* out_pay,
                    const uint32_t* kdesc) {
    // keys with a compaction descriptor: the compact case by k_shard_gather, the other by the staged
    // kernel (each returns at once in the other's case)
    if constexpr (!NODES)
        if (h->pack_pay16) {         // route_multi's 2-B origin indices (KD_IDX16); keys with a descriptor
            uint16_t* op = reinterpret_cast<uint16_t*>(out_pay);
            if (h->shard_gather)
                GD_TRY(launch(h, "k_shard_scatter", dim3(tiles), dim3(SH_NT), 0, k_shard_gather<BITS, uint16_t>,
                              (const gd_key*)recs, payload, dest, n, n_shards, tiles, gscan, out, op, kdesc,
                              h->shard_n1_copy ? (const uint32_t*)h->shard_n1.p : nullptr));
            if (h->shard_gather)
                return launch(h, "k_shard_scatter", dim3(tiles), dim3(SH_NT), 0,
                              k_shard_scatter<BITS, false, true, uint16_t>, recs, payload, dest, n, n_shards, tiles,
                              gscan, out, op, kdesc);
            return launch(h, "k_shard_scatter", dim3(tiles), dim3(SH_NT), 0, k_shard_scatter<BITS, false, false, uint16_t>,
                          recs, payload, dest, n, n_shards, tiles, gscan, out, op, kdesc);
        }
    if constexpr (!NODES)
        if (h->shard_gather && kdesc) {
            GD_TRY(launch(h, "k_shard_scatter", dim3(tiles), dim3(SH_NT), 0, k_shard_gather<BITS>,
                          (const gd_key*)recs, payload, dest, n, n_shards, tiles, gscan, out, out_pay, kdesc,
                          h->shard_n1_copy ? (const uint32_t*)h->shard_n1.p : nullptr));
            return launch(h, "k_shard_scatter", dim3(tiles), dim3(SH_NT), 0, k_shard_scatter<BITS, false, true>, recs,
                          payload, dest, n, n_shards, tiles, gscan, out, out_pay, kdesc);
        }
    return launch(h, "k_shard_scatter", dim3(tiles), dim3(SH_NT), 0, k_shard_scatter<BITS, NODES>, recs, payload, dest,
                  n, n_shards, tiles, gscan, out, out_pay, kdesc);
}

template <bool NODES>
int shard_finish(gd_handle* h, const void* recs, const uint32_t* payload, uint32_t n, uint32_t n_shards, uint32_t bits,
                 uint32_t tiles, const uint8_t* dest, uint32_t* hist, void* out_recs, uint32_t* out_pay,
                 uint32_t* counts, const uint32_t* kdesc = nullptr, uint32_t group = 1);

// Stable partition of n records (gd_key or u32 node ids) by destination rank, payload alongside
// (payload == nullptr: the batch index); counts[d] per destination.  kdesc != nullptr (keys): the
// header-compaction descriptor (k_key_desc) is built, and a compact batch is written as N1 only.
// regions = N_REGIONS (keys): each rank's chunk is ordered by the grains' table region on the owner
// (then batch order), for the owner's region-mapped probe; counts stay per rank.
template <bool NODES>
int shard_pack(gd_handle* h, const void* recs, const uint32_t* payload, uint32_t n, uint64_t tcd, uint32_t n_shards,
               void* out_recs, uint32_t* out_pay, uint32_t* counts, const ExtArgs& ext,
               uint32_t* kdesc, uint32_t regions) {
    GD_TRY(check_ring(h));
    if (kdesc) HIP_TRY(h, hipMemsetAsync(kdesc, 0, 16, h->stream));
    if (n == 0) {
        if (kdesc)
            GD_TRY(launch(h, "k_key_desc", dim3(1), dim3(64), 0, k_key_desc, (const gd_key*)recs, n, kdesc,
                          h->narrow_headers ? 1u : 0u));
        return launch(h, "k_fill", dim3(1), dim3(BLOCK), 0, k_fill_u32, counts, n_shards, 0u);
    }
    if (NODES || n_shards * regions > 256) regions = 1;
    const uint32_t n_dest = n_shards * regions;
    const uint32_t tiles = blocks_for(n, SH_TILE);
    if ((uint64_t)tiles * n_dest > 0xFFFFFFFFull) return set_err(h, GD_EINVAL, "batch too large to partition");
    GD_TRY(ensure(h, h->shard_dest, (size_t)n));
    GD_TRY(ensure(h, h->shard_hist, (size_t)tiles * n_dest * 4));
    if (!NODES && kdesc) GD_TRY(ensure(h, h->shard_n1, (size_t)n * 4));
    uint8_t* dest = (uint8_t*)h->shard_dest.p;
    uint32_t* hist = (uint32_t*)h->shard_hist.p;
    uint32_t bits = 1;
    while ((1u << bits) < n_dest) ++bits;
    GD_TRY(with_ring_mode(h->ring_mode, [&](auto mode) {
        return shard_hist_t<decltype(mode)::value, NODES>(h, recs, n, tcd, n_shards, bits, tiles, dest, hist, ext, kdesc,
                                                          regions);
    }));
    return shard_finish<NODES>(h, recs, payload, n, n_shards, bits, tiles, dest, hist, out_recs, out_pay, counts,
                               kdesc, regions);
}

// Forward partition of routed messages by the rank hosting their activation (k_fwd_hist): keys
// move, out_pos[j] = the message's position in the input.
// n1 (optional): the messages' keys are u32 N1s (one TypeCodeData, N0 = 0) and move as such.
int fwd_pack(gd_handle* h, const gd_key* keys, const uint8_t* st, const uint32_t* silo, uint32_t n, uint32_t n_shards,
             uint32_t my_rank, void* out_keys, uint32_t* out_pos, uint32_t* counts, const uint32_t* n1) {
    if (n == 0)
        return launch(h, "k_fill", dim3(1), dim3(BLOCK), 0, k_fill_u32, counts, n_shards, 0u);
    const uint32_t tiles = blocks_for(n, SH_TILE);
    if ((uint64_t)tiles * n_shards > 0xFFFFFFFFull) return set_err(h, GD_EINVAL, "batch too large to partition");
    GD_TRY(ensure(h, h->shard_dest, (size_t)n));
    GD_TRY(ensure(h, h->shard_hist, (size_t)tiles * n_shards * 4));
    uint8_t* dest = (uint8_t*)h->shard_dest.p;
    uint32_t* hist = (uint32_t*)h->shard_hist.p;
    uint32_t bits = 1;
    while ((1u << bits) < n_shards) ++bits;
    GD_TRY(launch(h, "k_fwd_hist", dim3(tiles), dim3(SH_NT), 0, k_fwd_hist, st, silo, n, n_shards, my_rank, bits, tiles,
                  dest, hist));
    if (n1) return shard_finish<true>(h, n1, nullptr, n, n_shards, bits, tiles, dest, hist, out_keys, out_pos, counts);
    return shard_finish<false>(h, keys, nullptr, n, n_shards, bits, tiles, dest, hist, out_keys, out_pos, counts);
}

template <bool NODES>
int shard_finish(gd_handle* h, const void* recs, const uint32_t* payload, uint32_t n, uint32_t n_shards, uint32_t bits,
                 uint32_t tiles, const uint8_t* dest, uint32_t* hist, void* out_recs, uint32_t* out_pay,
                 uint32_t* counts, const uint32_t* kdesc, uint32_t group) {
    GD_TRY(scan_device<OpAdd>(h, hist, tiles * n_shards * group, false, false, "shard"));
    // k_shard_counts also completes the compaction descriptor (kdesc, keys only)
    GD_TRY(launch(h, "k_shard_counts", dim3(1), dim3(256), 0, k_shard_counts, (const uint32_t*)hist, tiles, n_shards, n,
                  counts, NODES ? nullptr : (const gd_key*)recs, NODES ? nullptr : const_cast<uint32_t*>(kdesc),
                  h->narrow_headers ? 1u : 0u, group));
    const uint32_t* gs = hist;
    n_shards *= group;                  // the scatter's destinations: (rank, region) pairs
    switch (bits) {
        case 1: return shard_scatter_t<1, NODES>(h, recs, payload, dest, n, n_shards, tiles, gs, out_recs, out_pay,
                                                   kdesc);
        case 2: return shard_scatter_t<2, NODES>(h, recs, payload, dest, n, n_shards, tiles, gs, out_recs, out_pay,
                                                   kdesc);
        case 3: return shard_scatter_t<3, NODES>(h, recs, payload, dest, n, n_shards, tiles, gs, out_recs, out_pay,
                                                   kdesc);
        case 4: return shard_scatter_t<4, NODES>(h, recs, payload, dest, n, n_shards, tiles, gs, out_recs, out_pay,
                                                   kdesc);
        case 5: return shard_scatter_t<5, NODES>(h, recs, payload, dest, n, n_shards, tiles, gs, out_recs, out_pay,
                                                   kdesc);
        case 6: return shard_scatter_t<6, NODES>(h, recs, payload, dest, n, n_shards, tiles, gs, out_recs, out_pay,
                                                   kdesc);
        case 7: return shard_scatter_t<7, NODES>(h, recs, payload, dest, n, n_shards, tiles, gs, out_recs, out_pay,
                                                   kdesc);
        default: return shard_scatter_t<8, NODES>(h, recs, payload, dest, n, n_shards, tiles, gs, out_recs, out_pay,
                                                  kdesc);
    }
}


}  // namespace gdx

namespace gdx {
template int shard_pack<true>(gd_handle*, const void*, const uint32_t*, uint32_t, uint64_t, uint32_t, void*, uint32_t*,
                              uint32_t*, const ExtArgs&, uint32_t*, uint32_t);
template int shard_pack<false>(gd_handle*, const void*, const uint32_t*, uint32_t, uint64_t, uint32_t, void*, uint32_t*,
                               uint32_t*, const ExtArgs&, uint32_t*, uint32_t);
}  // namespace gdx
