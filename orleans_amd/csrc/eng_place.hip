// eng_place.hip -- libgraindispatch: the batched placement of unregistered grains: after the route, the
// messages left GD_ROUTE_MISS get a silo by their placement strategy, register in batch order through the directory
// batch (register_core, unchanged) and leave addressed (gd_place.h), alone or followed by the bucketing.
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"
#include "gd_place.h"

namespace {

// The argument checks that need no handle (so a caller's mistake is reported the same with or without one).
int check_place_args(gd_handle* h, int default_strategy) {
    if (default_strategy < GD_PLACE_NONE || default_strategy > GD_PLACE_GIVEN)
        return set_err(h, GD_EINVAL, "default_strategy %d not in 0..3", default_strategy);
    return GD_OK;
}

int check_place_state(gd_handle* h, const char* call) {
    if (!h) return set_err(nullptr, GD_ESTATE, "%s: null handle (no gd_place_configure)", call);
    if (!h->place_nsilos) return set_err(h, GD_ESTATE, "%s before gd_place_configure", call);
    if (h->cache_max)
        return set_err(h, GD_ESTATE, "%s on a handle in cache mode: placement is the directory owner's", call);
    return GD_OK;
}

// The route, then the placement of its misses, on device arrays (strategy / given / new_idx may be null).
// *n_new / *n_prop are host words.  A batch without a candidate costs the mark, the scan and one read-back.
int place_device(gd_handle* h, const gd_key* keys, uint32_t n, const uint8_t* strategy, uint32_t default_strategy,
                 const uint32_t* given, uint32_t act_base, uint32_t* silo, uint32_t* act, uint8_t* status,
                 uint8_t* placed, uint32_t* new_idx, uint32_t* n_new, uint32_t* n_prop) {
    *n_new = 0;
    *n_prop = 0;
    if (n == 0) return GD_OK;
    if (n > (1u << 31)) return set_err(h, GD_EINVAL, "route place: n > 2^31");
    GD_TRY(route_device(h, keys, n, silo, act, status));
    StageTime stage(h, "stage:place");
    const uint32_t tiles = blocks_for(n, PL_TILE);
    GD_TRY(ensure(h, h->place_scr[0], ((size_t)tiles + 1) * 4));
    uint32_t* tile_cnt = (uint32_t*)h->place_scr[0].p;
    const PlaceArgs a{(const uint32_t*)h->place_sorted.p, (const uint32_t*)h->place_compat.p,
                      (const uint32_t*)h->dir_valid.p, h->place_nsilos, h->place_ncomp, h->n_valid, h->cfg.my_silo,
                      h->place_local ? 1u : 0u, h->place_nsilos <= PL_TAB_LDS_SILOS ? 1u : 0u};
    const uint32_t wide = (((uintptr_t)status | (uintptr_t)placed) & 15u) == 0 ? 1u : 0u;
    GD_TRY(launch(h, "k_place_mark", dim3(tiles), dim3(PL_NT), pl_mark_lds(a), k_place_mark, (const uint8_t*)status, keys,
                  strategy, default_strategy, given, n, a, tiles, wide, placed, tile_cnt));
    GD_TRY(scan_device<OpAdd>(h, tile_cnt, tiles + 1, false, false, "place"));
    uint32_t m = 0;
    GD_TRY(read_back(h, tile_cnt + tiles, &m, 1));
    if (m == 0) return GD_OK;
    if ((uint64_t)act_base + m > (uint64_t)GD_ACT_MULTI)
        return set_err(h, GD_EINVAL, "route place: act_base %u + %u proposals reaches GD_ACT_MULTI", act_base, m);
    GD_TRY(ensure(h, h->place_scr[2], (size_t)m * 4));
    GD_TRY(ensure(h, h->place_scr[3], (size_t)m * sizeof(gd_key)));
    GD_TRY(ensure(h, h->place_scr[4], (size_t)m * sizeof(gd_val)));
    GD_TRY(ensure(h, h->place_scr[5], (size_t)m * sizeof(gd_val)));
    GD_TRY(ensure(h, h->place_scr[6], (size_t)m));
    uint32_t* idx = (uint32_t*)h->place_scr[2].p;
    gd_key* ckeys = (gd_key*)h->place_scr[3].p;
    gd_val* cvals = (gd_val*)h->place_scr[4].p;
    gd_val* win = (gd_val*)h->place_scr[5].p;
    uint8_t* ins = (uint8_t*)h->place_scr[6].p;
    GD_TRY(launch(h, "k_place_gather", dim3(tiles), dim3(PL_NT), 0, k_place_gather, (const uint8_t*)placed, keys, strategy,
                  default_strategy, given, n, a, wide, (const uint32_t*)tile_cnt, act_base, m, idx, ckeys, cvals));
    // AddSingleActivation for the candidates in batch order: deduplicates, grows the table, re-projects the
    // probe indexes; synchronous
    GD_TRY(register_core(h, ckeys, cvals, m, win, ins, false));
    const uint32_t blocks = blocks_for(m, PL_NT);
    GD_TRY(ensure(h, h->place_scr[1], ((size_t)blocks + 1) * 4));
    uint32_t* blk_cnt = (uint32_t*)h->place_scr[1].p;
    GD_TRY(launch(h, "k_place_apply", dim3(blocks), dim3(PL_NT), 0, k_place_apply, (const uint32_t*)idx,
                  (const gd_val*)win, (const uint8_t*)ins, m, n, silo, act, status, placed, blk_cnt, blocks));
    GD_TRY(scan_device<OpAdd>(h, blk_cnt, blocks + 1, false, false, "place_new"));
    if (new_idx)
        GD_TRY(launch(h, "k_place_new", dim3(blocks), dim3(PL_NT), 0, k_place_new, (const uint32_t*)idx,
                      (const gd_val*)win, (const uint8_t*)ins, m, (const uint32_t*)blk_cnt, new_idx, n));
    GD_TRY(read_back(h, blk_cnt + blocks, n_new, 1));
    *n_prop = m;
    return GD_OK;
}

struct PlaceHost {
    const uint8_t* strategy;
    const uint32_t* given;
    uint8_t* placed;
    uint32_t* new_idx;
};

// Host-pointer forms: keys and the optional inputs up, room for the outputs (silo / act / status: out_a..c).
int place_inputs(gd_handle* h, HostStage& io, const gd_key* keys, uint32_t n, const uint8_t* strategy,
                 const uint32_t* given, uint8_t* out_placed, bool want_new, PlaceHost* d) {
    GD_TRY(h2d(h, h->keys_in, keys, n));
    d->strategy = io.in(strategy, n);
    d->given = io.in(given, n);
    GD_TRY(ensure(h, h->out_a, (size_t)n * 4 + 4));
    GD_TRY(ensure(h, h->out_b, (size_t)n * 4 + 4));
    GD_TRY(ensure(h, h->out_c, (size_t)n + 4));
    d->placed = io.out(out_placed, n, 4);
    d->new_idx = io.hold<uint32_t>(n, 4, want_new);   // the first n_new come down (place_outputs)
    return io.status();
}

int place_outputs(gd_handle* h, HostStage& io, const PlaceHost& d, uint32_t n, uint32_t n_new, uint32_t* out_silo,
                  uint32_t* out_act, uint8_t* out_status, uint32_t* out_new_idx) {
    GD_TRY(d2h(h, out_silo, h->out_a, n));
    GD_TRY(d2h(h, out_act, h->out_b, n));
    GD_TRY(d2h(h, out_status, h->out_c, n));
    GD_TRY(io.fetch());
    return io.fetch(out_new_idx, d.new_idx, n_new);
}

}  // namespace

extern "C" {

int gd_place_configure(gd_handle* h, const gd_silo_addr* silos, uint32_t n_silos, const uint8_t* compatible,
                       int local_active) {
    if (n_silos < 1 || n_silos > PL_MAX_SILOS)
        return set_err(h, GD_EINVAL, "gd_place_configure: n_silos %u not in 1..%u", n_silos, PL_MAX_SILOS);
    if (!h || !silos) return set_err(h, GD_EINVAL, "gd_place_configure: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    // context.GetCompatibleSilos(target).OrderBy(s => s) (HashBasedPlacementDirector.cs:11), here, once
    std::vector<uint32_t> sorted;
    std::vector<uint32_t> bits((n_silos + 31) / 32 + 1, 0);
    for (uint32_t s = 0; s < n_silos; ++s)
        if (!compatible || compatible[s]) {
            sorted.push_back(s);
            bits[s >> 5] |= 1u << (s & 31);
        }
    std::stable_sort(sorted.begin(), sorted.end(),
                     [&](uint32_t x, uint32_t y) { return gd_silo_compare(&silos[x], &silos[y]) < 0; });
    const uint32_t my = h->cfg.my_silo;
    GD_TRY(sync(h));                               // a batch in flight reads the table it was enqueued with
    h->place_nsilos = 0;
    GD_TRY(h2d(h, h->place_sorted, sorted.data(), sorted.size()));
    GD_TRY(set_bitset(h, h->place_compat, bits));
    GD_TRY(sync(h));
    h->place_ncomp = (uint32_t)sorted.size();
    h->place_local = local_active && my < n_silos && (!compatible || compatible[my]);
    h->place_nsilos = n_silos;
    return GD_OK;
}

int gd_route_place_device(gd_handle* h, const gd_key* d_keys, uint32_t n, const uint8_t* d_strategy,
                          int default_strategy, const uint32_t* d_given_silo, uint32_t act_base, uint32_t* d_silo,
                          uint32_t* d_act, uint8_t* d_status, uint8_t* d_placed, uint32_t* d_new_idx,
                          uint32_t* out_n_new, uint32_t* out_n_proposed) {
    GD_TRY(check_place_args(h, default_strategy));
    GD_TRY(check_place_state(h, "gd_route_place_device"));
    if (!out_n_new || !out_n_proposed || (n && (!d_keys || !d_silo || !d_act || !d_status || !d_placed)))
        return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_route_place_device"));
    return place_device(h, d_keys, n, d_strategy, (uint32_t)default_strategy, d_given_silo, act_base, d_silo, d_act,
                        d_status, d_placed, d_new_idx, out_n_new, out_n_proposed);
}

int gd_route_place(gd_handle* h, const gd_key* keys, uint32_t n, const uint8_t* strategy, int default_strategy,
                   const uint32_t* given_silo, uint32_t act_base, uint32_t* out_silo, uint32_t* out_act,
                   uint8_t* out_status, uint8_t* out_placed, uint32_t* out_new_idx, uint32_t* out_n_new,
                   uint32_t* out_n_proposed) {
    GD_TRY(check_place_args(h, default_strategy));
    GD_TRY(check_place_state(h, "gd_route_place"));
    if (!out_n_new || !out_n_proposed || (n && (!keys || !out_silo || !out_act || !out_status || !out_placed)))
        return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_route_place"));
    HostStage io(h);
    PlaceHost d;
    GD_TRY(place_inputs(h, io, keys, n, strategy, given_silo, out_placed, out_new_idx != nullptr, &d));
    GD_TRY(place_device(h, (const gd_key*)h->keys_in.p, n, d.strategy, (uint32_t)default_strategy, d.given, act_base,
                        (uint32_t*)h->out_a.p, (uint32_t*)h->out_b.p, (uint8_t*)h->out_c.p, d.placed, d.new_idx,
                        out_n_new, out_n_proposed));
    GD_TRY(place_outputs(h, io, d, n, *out_n_new, out_silo, out_act, out_status, out_new_idx));
    return sync_checked(h);
}

int gd_route_place_bucket_device(gd_handle* h, const gd_key* d_keys, uint32_t n, const uint8_t* d_strategy,
                                 int default_strategy, const uint32_t* d_given_silo, uint32_t act_base,
                                 uint32_t* d_silo, uint32_t* d_act, uint8_t* d_status, uint8_t* d_placed,
                                 uint32_t* d_new_idx, uint32_t* out_n_new, uint32_t* out_n_proposed, uint32_t n_act,
                                 uint32_t* d_perm, uint32_t* d_offsets) {
    GD_TRY(check_place_args(h, default_strategy));
    GD_TRY(check_place_state(h, "gd_route_place_bucket_device"));
    if (!out_n_new || !out_n_proposed || !d_offsets ||
        (n && (!d_keys || !d_silo || !d_act || !d_status || !d_placed || !d_perm)))
        return set_err(h, GD_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_route_place_bucket_device"));
    GD_TRY(place_device(h, d_keys, n, d_strategy, (uint32_t)default_strategy, d_given_silo, act_base, d_silo, d_act,
                        d_status, d_placed, d_new_idx, out_n_new, out_n_proposed));
    return bucket_device(h, d_act, n, n_act, d_perm, d_offsets);
}

int gd_route_place_bucket(gd_handle* h, const gd_key* keys, uint32_t n, const uint8_t* strategy,
                          int default_strategy, const uint32_t* given_silo, uint32_t act_base, uint32_t* out_silo,
                          uint32_t* out_act, uint8_t* out_status, uint8_t* out_placed, uint32_t* out_new_idx,
                          uint32_t* out_n_new, uint32_t* out_n_proposed, uint32_t n_act, uint32_t* out_perm,
                          uint32_t* out_offsets) {
    GD_TRY(check_place_args(h, default_strategy));
    GD_TRY(check_place_state(h, "gd_route_place_bucket"));
    if (!out_n_new || !out_n_proposed || !out_offsets ||
        (n && (!keys || !out_silo || !out_act || !out_status || !out_placed || !out_perm)))
        return set_err(h, GD_EINVAL, "null argument");
    if (n_act == 0xFFFFFFFFu) return set_err(h, GD_EINVAL, "n_act too large");
    HIP_TRY(h, hipSetDevice(h->device));
    GD_TRY(check_not_capturing(h, "gd_route_place_bucket"));
    HostStage io(h);
    PlaceHost d;
    GD_TRY(place_inputs(h, io, keys, n, strategy, given_silo, out_placed, out_new_idx != nullptr, &d));
    GD_TRY(ensure(h, h->u8_a, (size_t)n * 4 + 4));   // perm
    GD_TRY(ensure(h, h->offs, ((size_t)n_act + 2) * 4));
    GD_TRY(place_device(h, (const gd_key*)h->keys_in.p, n, d.strategy, (uint32_t)default_strategy, d.given, act_base,
                        (uint32_t*)h->out_a.p, (uint32_t*)h->out_b.p, (uint8_t*)h->out_c.p, d.placed, d.new_idx,
                        out_n_new, out_n_proposed));
    GD_TRY(bucket_device(h, (const uint32_t*)h->out_b.p, n, n_act, (uint32_t*)h->u8_a.p, (uint32_t*)h->offs.p));
    GD_TRY(place_outputs(h, io, d, n, *out_n_new, out_silo, out_act, out_status, out_new_idx));
    GD_TRY(d2h(h, out_perm, h->u8_a, n));
    GD_TRY(d2h(h, out_offsets, h->offs, (size_t)n_act + 2));
    return sync_checked(h);
}

}  // extern "C"
