// eng_bucket.hip -- libgraindispatch: the device-wide scan and the bucketing drivers (the LSD radix passes,
// the one-pass and the three-pass two-level forms).
// Shared handle and helpers: gd_engine.h.
#include "gd_engine.h"

namespace gdx {

// The tune entry's second class for the bucketing form (kind 4): the messages a 1,024-activation range
// holds, as a bit length (it decides whether ranges are staged in LDS).
int bucket_sub(uint64_t n, uint32_t n_act) {
    int per_range = 0;
    while (per_range < 31 && ((uint64_t)n / ((n_act >> MSD_SHIFT) + 1) >> per_range) > 1) ++per_range;
    return per_range;
}

// ---- scans -------------------------------------------------------------------
// Scan of data[0..n) into out (default: in place).
template <class Op>
int scan_device(gd_handle* h, uint32_t* data, uint32_t n, bool reverse, bool inclusive, const char* tag,
                uint32_t* out) {
    if (n == 0) return GD_OK;
    if (!out) out = data;
    // too many 1,024-entry tiles to fold but few 4,096-entry ones: the wide tiles, 2 launches
    if (blocks_for(n, SCAN_TILE) > 2048 && blocks_for(n, 4 * SCAN_TILE) <= 4096) {
        const uint32_t nbw = blocks_for(n, 4 * SCAN_TILE);
        GD_TRY(ensure(h, h->partials, (size_t)nbw * sizeof(uint32_t)));
        uint32_t* part = (uint32_t*)h->partials.p;
        GD_TRY(launch(h, "k_scan_reduce", dim3(nbw), dim3(BLOCK), 0, k_scan_reduce<Op, 16>, (const uint32_t*)data, n,
                      reverse, part));
        return launch(h, "k_scan_down", dim3(nbw), dim3(BLOCK), 0, k_scan_down<Op, 16>, (const uint32_t*)data, out, n,
                      reverse, inclusive, (const uint32_t*)part, nbw);
    }
    const uint32_t nb = blocks_for(n, SCAN_TILE);
    GD_TRY(ensure(h, h->partials, (size_t)nb * sizeof(uint32_t)));
    uint32_t* part = (uint32_t*)h->partials.p;
    (void)tag;
    GD_TRY(launch(h, "k_scan_reduce", dim3(nb), dim3(BLOCK), 0, k_scan_reduce<Op>, (const uint32_t*)data, n, reverse, part));
    // few blocks (<= 2048: each block then reads <= 8 aggregates per thread): every block folds its
    // predecessors' aggregates itself (2 launches);
    // many: the aggregates are scanned in between -- by the same two-launch fold scan one level
    // up while that has <= 1024 blocks (4 launches), else by one block (3 launches)
    const bool fold = nb <= 2048;
    if (!fold) {
        const uint32_t nb2 = blocks_for(nb, SCAN_TILE);
        if (nb2 <= 1024) {
            GD_TRY(ensure(h, h->partials2, (size_t)nb2 * sizeof(uint32_t)));
            uint32_t* part2 = (uint32_t*)h->partials2.p;
            // partials are in logical order already: scan them forward, exclusive, in place
            GD_TRY(launch(h, "k_scan_reduce", dim3(nb2), dim3(BLOCK), 0, k_scan_reduce<Op>, (const uint32_t*)part, nb,
                          false, part2));
            GD_TRY(launch(h, "k_scan_down", dim3(nb2), dim3(BLOCK), 0, k_scan_down<Op>, (const uint32_t*)part, part, nb,
                          false, false, (const uint32_t*)part2, nb2));
        } else {
            GD_TRY(launch(h, "k_scan_partials", dim3(1), dim3(BLOCK), 0, k_scan_partials<Op>, part, nb));
        }
    }
    return launch(h, "k_scan_down", dim3(nb), dim3(BLOCK), 0, k_scan_down<Op>, (const uint32_t*)data, out, n, reverse,
                  inclusive, (const uint32_t*)part, fold ? nb : 0u);
}

// ---- K3 bucketing -------------------------------------------------------------
template <int BITS, int NT, int IT>
int radix_pass_t(gd_handle* h, const uint32_t* kin, const uint32_t* vin, uint32_t n, uint32_t clamp, uint32_t shift,
                 uint32_t* kout, uint32_t* vout, bool first,
                 uint32_t* offsets, uint32_t* rank_out, FillArgs fill, Pack pk) {
    constexpr uint32_t TILE = NT * IT;
    const uint32_t tiles = blocks_for(n, TILE);
    const uint32_t R = 1u << BITS;
    // the digit-major counts, then (row scans) the R digit totals
    GD_TRY(ensure(h, h->hist, ((size_t)R * tiles + R) * sizeof(uint32_t)));
    uint32_t* hist = (uint32_t*)h->hist.p;
    // below 1024 tiles, 4 per workgroup would leave fewer workgroups than the 256 CUs; up to 12,288
    // tiles (48M keys) 4 per workgroup in reverse XCD order also leaves the scatter's keys in L2
    // (f2 hop 3, 43M keys: bucketing -8%); at cfg 3's 16,384 tiles it is neutral, one stays
    const uint32_t tpb = tiles >= 1024 && tiles <= 12288 ? 4u : 1u;
    // multi-tile histograms walk the scatter's XCD tile ranges backwards (hist_t0)
    const uint32_t hxr = h->hist_xcd && h->xcd_tiles ? 1u : 0u;
    if (pk.in) {
        // packed records: the histogram reads the u16 high-key array (bucket_device enables the
        // packing only for the 512 x 8 tiles and digits of at most 8 bits)
        if constexpr (BITS <= 8 && NT == 512 && IT == 8) {
            const uint16_t* kb16 = reinterpret_cast<const uint16_t*>(vin);
            if (tpb == 4)
                GD_TRY(launch(h, "k_radix_hist", dim3(blocks_for(tiles, 4)), dim3(NT), 0, k_radix_hist16<BITS, NT, IT, 4>,
                              kb16, n, shift - pk.b1, tiles, hist, hxr));
            else
                GD_TRY(launch(h, "k_radix_hist", dim3(tiles), dim3(NT), 0, k_radix_hist16<BITS, NT, IT, 1>, kb16, n,
                              shift - pk.b1, tiles, hist, hxr));
        } else {
            return set_err(h, GD_EINVAL, "packed radix records need 512 x 8 tiles and <= 8-bit digits");
        }
    } else if constexpr (BITS <= 9) {
        if (tpb == 4)
            GD_TRY(launch(h, "k_radix_hist", dim3(blocks_for(tiles, 4)), dim3(NT), 0, k_radix_hist_multi<BITS, NT, IT, 4>,
                          kin, n, clamp, shift, tiles, hist, fill, hxr));
        else
            GD_TRY(launch(h, "k_radix_hist", dim3(tiles), dim3(NT), 0, k_radix_hist<BITS, NT, IT>, kin, n, clamp, shift,
                          tiles, hist, fill));
    } else {
        GD_TRY(launch(h, "k_radix_hist", dim3(tiles), dim3(NT), 0, k_radix_hist<BITS, NT, IT>, kin, n, clamp, shift, tiles,
                      hist, fill));
    }
    // one scan launch per digit row (the scatter adds the digit bases)
    const uint32_t* totals = hist + (size_t)R * tiles;
    h->last_totals = totals;
    h->last_digits = R;
    GD_TRY(launch(h, "k_radix_rowscan", dim3(R), dim3(BLOCK), 0, k_radix_rowscan, hist, tiles, hist + (size_t)R * tiles));
    if (first)
        return launch(h, "k_radix_scatter", dim3(tiles), dim3(NT), 0, k_radix_scatter<BITS, true, NT, IT>, kin, vin, n,
                      clamp, shift, tiles, (const uint32_t*)hist, kout, vout, h->radix_rank_atomic, offsets, h->xcd_tiles,
                      rank_out, totals, pk);
    return launch(h, "k_radix_scatter", dim3(tiles), dim3(NT), 0, k_radix_scatter<BITS, false, NT, IT>, kin, vin, n,
                  clamp, shift, tiles, (const uint32_t*)hist, kout, vout, h->radix_rank_atomic, offsets, h->xcd_tiles,
                  rank_out, totals, pk);
}

template <int BITS>
int radix_pass(gd_handle* h, const uint32_t* kin, const uint32_t* vin, uint32_t n, uint32_t clamp, uint32_t shift,
               uint32_t* kout, uint32_t* vout, bool first, uint32_t* offsets, uint32_t* rank_out, FillArgs fill, Pack pk) {
    // 512 threads x 8 messages (tools/ab_bucket.py: beat 256 x 16, 1024 x 4 and 512 x 16 by 10-20 %)
    return radix_pass_t<BITS, 512, 8>(h, kin, vin, n, clamp, shift, kout, vout, first, offsets, rank_out, fill, pk);
}

int radix_dispatch(gd_handle* h, int bits, const uint32_t* kin, const uint32_t* vin, uint32_t n, uint32_t clamp,
                   uint32_t shift, uint32_t* kout, uint32_t* vout, bool first,
                 uint32_t* offsets, uint32_t* rank_out, FillArgs fill, Pack pk) {
    switch (bits) {
        case 4: return radix_pass<4>(h, kin, vin, n, clamp, shift, kout, vout, first, offsets, rank_out, fill, pk);
        case 5: return radix_pass<5>(h, kin, vin, n, clamp, shift, kout, vout, first, offsets, rank_out, fill, pk);
        case 6: return radix_pass<6>(h, kin, vin, n, clamp, shift, kout, vout, first, offsets, rank_out, fill, pk);
        case 7: return radix_pass<7>(h, kin, vin, n, clamp, shift, kout, vout, first, offsets, rank_out, fill, pk);
        case 8: return radix_pass<8>(h, kin, vin, n, clamp, shift, kout, vout, first, offsets, rank_out, fill, pk);
        case 9: return radix_pass<9>(h, kin, vin, n, clamp, shift, kout, vout, first, offsets, rank_out, fill, pk);
        case 10: return radix_pass<10>(h, kin, vin, n, clamp, shift, kout, vout, first, offsets, rank_out, fill, pk);
        default: return radix_pass<11>(h, kin, vin, n, clamp, shift, kout, vout, first, offsets, rank_out, fill, pk);
    }
}

// The one-pass form's MSD pass (gd_bucket2.h): 8K-item tiles (512 threads, two workgroups a CU, 32-B
// index runs at R ~ 1,024; 65 against 76 us on 16K tiles at cfg 2), digit min(act, n_act) >> shift.
// K16: the range-local keys as u16 (the one-pass form); else the whole clamped key as u32 (pass A of
// the three-pass form).  Leaves the digit totals in last_totals.
template <int RMAX, int KOUT, bool BALLOT>
int msd_pass(gd_handle* h, const uint32_t* acts, uint32_t n, uint32_t n_act, uint32_t R, uint32_t shift, uint32_t* k1,
             uint32_t* v1, B2Pack pk = B2Pack{0, 0, 32}, uint32_t ku = 0) {
    const uint2 clamp = make_uint2(n_act, ku ? ku : n_act);      // keys >= n_act -> ku (b2_clamp)
    const uint32_t tiles = blocks_for(n, B2_TILE);
    const uint32_t hxr = h->hist_xcd && h->xcd_tiles ? 1u : 0u;
    GD_TRY(ensure(h, h->hist, ((size_t)R * tiles + R) * sizeof(uint32_t)));
    uint32_t* hist = (uint32_t*)h->hist.p;
    // 4 tiles a histogram workgroup from 1,024 tiles up (20.3 / 21.3 / 24.7 us at cfg 2 for 1 / 2 / 4,
    // profiles/r03_msd_htpb_ab.txt: 4 is the fastest; fewer tiles leave CUs idle)
    if (tiles >= 1024)
        GD_TRY(launch(h, "k_radix_hist", dim3(blocks_for(tiles, 4)), dim3(B2_NT), 0, k_b2_hist<B2_NT, B2_IT, 4, RMAX>,
                      acts, n, clamp, R, tiles, hist, shift, hxr));
    else
        GD_TRY(launch(h, "k_radix_hist", dim3(tiles), dim3(B2_NT), 0, k_b2_hist<B2_NT, B2_IT, 1, RMAX>, acts, n, clamp,
                      R, tiles, hist, shift, hxr));
    const uint32_t* tot = hist + (size_t)R * tiles;
    GD_TRY(launch(h, "k_radix_rowscan", dim3(R), dim3(BLOCK), 0, k_radix_rowscan, hist, tiles, hist + (size_t)R * tiles));
    // GD_OPT_B2_PERSIST k > 0, the one-pass form (KEY16): k persistent workgroups a CU (a multiple of 8 in
    // all), each looping over its tiles with the next tile's loads under the current write-out.  cfg 2:
    // k_radix_scatter 0.0626 -> 0.0597 ms at k = 2, 0.087 at k = 1; pass A of the three-pass form at cfg 3
    // (Zipf, 8-K tiles) 0.173 -> 0.19 ms, so that pass keeps one workgroup a tile
    // (profiles/r05_b2_persist_ab.txt).  The ballot ranks keep it too (their persistent form spills).  The
    // persistent form addresses the activations by 32-bit byte offsets: batches up to 2^30 messages.
    bool persisted = false;
    if constexpr (KOUT == B2_KEY16 && !BALLOT) if (h->b2_persist && n <= (1u << 30)) {
        const uint32_t grid = std::min<uint32_t>(tiles, std::max<uint32_t>(8, (h->b2_persist * h->n_cu) & ~7u));
        GD_TRY(launch(h, "k_radix_scatter", dim3(grid), dim3(B2_NT), 0,
                      k_b2_scatter<B2_NT, B2_IT, RMAX, KOUT, BALLOT, true>, acts, n, clamp, R, tiles,
                      (const uint32_t*)hist, tot, k1, v1, shift, h->xcd_tiles, pk, h->b2_order));
        persisted = true;
    }
    if (!persisted)
        GD_TRY(launch(h, "k_radix_scatter", dim3(tiles), dim3(B2_NT), 0, k_b2_scatter<B2_NT, B2_IT, RMAX, KOUT, BALLOT>,
                      acts, n, clamp, R, tiles, (const uint32_t*)hist, tot, k1, v1, shift, h->xcd_tiles, pk, 0u));
    h->last_totals = tot;
    h->last_digits = R;
    return GD_OK;
}

// The one-pass two-level bucketing (gd_msd.h): a stable MSD pass on the high digit min(act, n_act) >> 10,
// then k_msd_local sorts each 1,024-activation range in LDS and writes its starts.  Needs (n_act >> 10)
// + 1 <= B2_RMAX2.
template <bool BALLOT>
int msd_bucket(gd_handle* h, const uint32_t* acts, uint32_t n, uint32_t n_act, uint32_t* perm, uint32_t* offsets,
               uint32_t* rank_out) {
    // The MSD pass clamps the keys at ku, the first key of a range past n_act's, rather than at n_act: the
    // unrouted messages (act >= n_act: directory misses, which a directory under churn sends in numbers)
    // get a range of their own, copied in order (msd_range_kp, L <= 1), instead of turning n_act's range
    // into a hot one ranked in chunks by one workgroup (1 % misses at cfg 2: k_msd_local 0.045 ->
    // 0.47 ms, tools/churn_probe.py).
    const uint32_t ku = msd_unrouted_key(n_act);
    const uint32_t R = (ku >> MSD_SHIFT) + 1;
    if (R > MSD_MAX_RANGES) return set_err(h, GD_EINVAL, "two-level bucketing: n_act too large");
    GD_TRY(ensure(h, h->u32_a, (size_t)n * 4));
    GD_TRY(ensure(h, h->u32_c, (size_t)n * 4));
    uint32_t* k1 = (uint32_t*)h->u32_a.p;
    uint32_t* v1 = (uint32_t*)h->u32_c.p;
    GD_TRY((msd_pass<B2_RMAX2, B2_KEY16, BALLOT>(h, acts, n, n_act, R, MSD_SHIFT, k1, v1, B2Pack{0, 0, 32}, ku)));
    return launch(h, "k_msd_local", dim3(std::min<uint32_t>(R, h->n_cu)), dim3(MSD_NT), 0, k_msd_local<BALLOT>,
                  (const uint16_t*)k1, (const uint32_t*)v1, h->last_totals, R, n, n_act, perm, offsets, rank_out);
}

// Three-pass form's split of k' = n_act >> 10: pass B's digit bits a (low part), pass A's kb - a.
// False when the one-pass form applies or k' needs more than 18 bits (n_act >= 2^28).
bool msd3_split(uint32_t n_act, uint32_t* a_out, uint32_t* ra_out) {
    const uint32_t km = n_act >> MSD_SHIFT;
    if (km + 1 <= MSD_MAX_RANGES) return false;
    uint32_t kb = 0;
    while (kb < 32 && (km >> kb) != 0) ++kb;
    if (kb > 18) return false;
    // pass B takes the smaller half: a 17-bit k' (BASELINE cfg 3) as 9 + 8 bits, pass B's 256 digits
    // writing twice the run length of 512 (k_seg_scatter 0.240 -> 0.218 ms, step 2.094 -> 2.035 ms,
    // profiles/r04_msd3_split_ab.jsonl)
    const uint32_t a = kb / 2;
    *a_out = a;
    *ra_out = (km >> a) + 1;
    return true;
}

// The three-pass two-level bucketing (gd_msd2.h), for n_act past the one-pass form's digit: pass A
// (MSD on d2 = k' >> a), pass B (segmented MSD on d1 = k' & (2^a - 1), one flat scan for the
// positions), then the level-2 work lists (thin ranges a wave each, staged ranges a workgroup each,
// hot ranges in chunks).  Grids of the level-2 kernels are bounded and loop over device-side counts.
template <bool BALLOT>
int msd3_bucket(gd_handle* h, const uint32_t* acts, uint32_t n, uint32_t n_act, uint32_t* perm, uint32_t* offsets,
                uint32_t* rank_out) {
    uint32_t a = 0, RA = 0;
    if (!msd3_split(n_act, &a, &RA)) return set_err(h, GD_EINVAL, "three-pass bucketing: n_act out of range");
    const uint32_t R = (n_act >> MSD_SHIFT) + 1, RB = 1u << a;
    const uint32_t tbound = blocks_for(n, SEG_TILE) + RA;
    // ranges past t_staged messages are chunked (k_l2_classify): at most n / (t_staged + 1) of them,
    // whatever GD_OPT_L2_STAGED / GD_OPT_L2_SMALL say
    const uint32_t t_staged = std::max(h->l2_small, h->l2_staged);
    const uint32_t cr_bound = std::min(R, n / (t_staged + 1) + 1);
    const uint32_t ch_bound = n / CH_CAP + cr_bound;
    GD_TRY(ensure(h, h->u32_a, (size_t)n * 4));
    GD_TRY(ensure(h, h->u32_b, (size_t)n * 4));
    GD_TRY(ensure(h, h->u32_c, (size_t)n * 4));
    GD_TRY(ensure(h, h->u32_d, (size_t)n * 4));
    DevBuf* m = h->m3;
    GD_TRY(ensure(h, m[0], (size_t)(RA + 1) * 4));                 // segment starts
    GD_TRY(ensure(h, m[1], (size_t)(RA + 1) * 4));                 // segment tile bases
    GD_TRY(ensure(h, m[2], (size_t)tbound * 4));                   // tile -> segment
    GD_TRY(ensure(h, m[3], (size_t)RB * tbound * 4));              // pass B counts, flat-scanned
    GD_TRY(ensure(h, m[4], (size_t)(R + 1) * 4));                  // range starts
    GD_TRY(ensure(h, m[5], (size_t)L2_CTR_WORDS * 4));
    GD_TRY(ensure(h, m[6], (size_t)R * 4));                        // thin ranges
    GD_TRY(ensure(h, m[7], (size_t)R * 4));                        // staged ranges
    GD_TRY(ensure(h, m[14], (size_t)R * 4));                       // mid ranges
    GD_TRY(ensure(h, m[8], (size_t)cr_bound * 4 * 4));             // chunked ranges
    // chunk-scan items: 1 a range of <= CS_DIRECT chunks, else CS_SLABS a piece of CS_ROWS chunks
    const uint32_t it_bound = cr_bound + CS_SLABS * (ch_bound / CS_DIRECT + blocks_for(ch_bound, CS_ROWS));
    GD_TRY(ensure(h, m[13], (size_t)it_bound * 4));
    GD_TRY(ensure(h, m[9], (size_t)ch_bound * 4));                 // chunk -> chunked range
    GD_TRY(ensure(h, m[10], (size_t)ch_bound * MSD_L * 4));        // per-chunk activation counts
    GD_TRY(ensure(h, m[11], (size_t)cr_bound * MSD_L * 4));        // per-range activation totals
    GD_TRY(ensure(h, m[12], (size_t)it_bound * CS_COLS * 4));        // per-item (slab x piece) column sums
    uint32_t* kA = (uint32_t*)h->u32_a.p;
    uint32_t* vA = (uint32_t*)h->u32_c.p;
    uint16_t* kB = (uint16_t*)h->u32_b.p;
    uint32_t* vB = (uint32_t*)h->u32_d.p;
    uint32_t* seg_start = (uint32_t*)m[0].p;
    uint32_t* seg_tb = (uint32_t*)m[1].p;
    uint32_t* tile_seg = (uint32_t*)m[2].p;
    uint32_t* hseg = (uint32_t*)m[3].p;
    // pass A: d2 = k' >> a.  Pass B needs the key's low a + 10 bits P: as a u16 of P's high bits with
    // the hb bits below them in the index word's spare top bits (6-B records) when the index leaves
    // room (BASELINE cfg 3: P 19 bits, 26-bit indices), else the whole key (8-B records)
    uint32_t ib = 1;
    while (ib < 32 && ((n - 1) >> ib) != 0) ++ib;
    const uint32_t pbits = a + MSD_SHIFT, hb = pbits > 16 ? pbits - 16 : 0;
    const bool pk = hb == 0 || ib + hb <= 32;
    const B2Pack bp{pbits, hb, hb ? ib : 32u};
    if (pk) GD_TRY((msd_pass<SEG_RMAX, B2_PACK, BALLOT>(h, acts, n, n_act, RA, MSD_SHIFT + a, kA, vA, bp)));
    else GD_TRY((msd_pass<SEG_RMAX, B2_KEY32, BALLOT>(h, acts, n, n_act, RA, MSD_SHIFT + a, kA, vA)));
    const SegIn in{(const uint16_t*)kA, (const uint32_t*)kA, (const uint32_t*)vA, hb, bp.ib};
    GD_TRY(launch(h, "k_seg_table", dim3(blocks_for(tbound, 1024)), dim3(1024), 0, k_seg_table, h->last_totals, RA, tbound, seg_start, seg_tb,
                  tile_seg, (uint32_t*)m[5].p));
    // pass B: d1 inside each d2 segment; one flat scan gives every (segment, digit, tile) its position
    if (pk)
        GD_TRY(launch(h, "k_seg_hist", dim3(tbound), dim3(SEG_NT), 0, k_seg_hist<true>, in, (const uint32_t*)tile_seg,
                      (const uint32_t*)seg_start, (const uint32_t*)seg_tb, RB, hseg));
    else
        GD_TRY(launch(h, "k_seg_hist", dim3(tbound), dim3(SEG_NT), 0, k_seg_hist<false>, in, (const uint32_t*)tile_seg,
                      (const uint32_t*)seg_start, (const uint32_t*)seg_tb, RB, hseg));
    GD_TRY(scan_device<OpAdd>(h, hseg, RB * tbound, false, false, "seg"));
    if (pk)
        GD_TRY(launch(h, "k_seg_scatter", dim3(tbound), dim3(SEG_NT), 0, k_seg_scatter<true, BALLOT>, in,
                      (const uint32_t*)tile_seg, (const uint32_t*)seg_start, (const uint32_t*)seg_tb, RB,
                      (const uint32_t*)hseg, kB, vB, h->xcd_tiles));
    else
        GD_TRY(launch(h, "k_seg_scatter", dim3(tbound), dim3(SEG_NT), 0, k_seg_scatter<false, BALLOT>, in,
                      (const uint32_t*)tile_seg, (const uint32_t*)seg_start, (const uint32_t*)seg_tb, RB,
                      (const uint32_t*)hseg, kB, vB, h->xcd_tiles));
    // level 2
    uint32_t* cr = (uint32_t*)m[8].p;
    const L2Lists l{(uint32_t*)m[4].p, (uint32_t*)m[6].p, (uint32_t*)m[7].p, (uint32_t*)m[14].p, cr, cr + cr_bound,
                    cr + 2 * cr_bound,
                    (uint32_t*)m[9].p, cr + 3 * cr_bound, (uint32_t*)m[13].p, (uint32_t*)m[5].p};
    GD_TRY(launch(h, "k_l2_classify", dim3(blocks_for(R, CL_NT)), dim3(CL_NT), 0, k_l2_classify, (const uint32_t*)hseg,
                  (const uint32_t*)seg_start, (const uint32_t*)seg_tb, a, R, n, h->l2_small,
                  std::max(h->l2_small, h->l2_mid), t_staged, l));
    // persistent grids sized to what the chip holds at once (a second round of workgroups would wait for
    // the first to finish its whole share): k_l2_small 4 a CU (32 KB of LDS, 8 waves each), the range
    // sort 1 a CU (135 KB), the chunk scatter 2 (72 KB), the chunk histogram 4 and the scan 2 a CU
    const uint32_t cu8 = (h->n_cu + 7) & ~7u;
    GD_TRY(launch(h, "k_l2_small", dim3(std::min<uint32_t>(blocks_for(R, L2_SMALL_WAVES), 4 * cu8)),
                  dim3(L2_SMALL_WAVES * WAVE), 0, k_l2_small<BALLOT>, (const uint16_t*)kB, (const uint32_t*)vB, l, n, n_act, perm,
                  offsets, rank_out));
    GD_TRY(launch(h, "k_msd_local_mid", dim3(std::min<uint32_t>(R, 3 * cu8)), dim3(MSD_MID_NT), 0,
                  k_msd_local_list<MSD_MID_NT, MSD_MID_RW, BALLOT>, (const uint16_t*)kB, (const uint32_t*)vB,
                  (const uint32_t*)l.rs, (const uint32_t*)l.mid, (const uint32_t*)(l.ctr + 5), n, n_act, perm, offsets,
                  rank_out));
    GD_TRY(launch(h, "k_msd_local", dim3(std::min<uint32_t>(R, cu8)), dim3(MSD_NT), 0, k_msd_local_list<MSD_NT, MSD_RW, BALLOT>,
                  (const uint16_t*)kB, (const uint32_t*)vB, (const uint32_t*)l.rs, (const uint32_t*)l.staged,
                  (const uint32_t*)(l.ctr + 1), n, n_act, perm, offsets, rank_out));
    uint32_t* hh = (uint32_t*)m[10].p;
    uint32_t* tot = (uint32_t*)m[11].p;
    // the chunk grids are multiples of 8 (chunk_walk: one contiguous chunk range an XCD)
    GD_TRY(launch(h, "k_l2_chunk_hist", dim3(4 * cu8), dim3(CH_NT), 0, k_l2_chunk_hist,
                  (const uint16_t*)kB, l, hh));
    uint32_t* ptot = (uint32_t*)m[12].p;
    GD_TRY(launch(h, "k_l2_chunk_ptot", dim3(2 * cu8), dim3(MSD_NT), 0, k_l2_chunk_ptot, l, (const uint32_t*)hh, ptot));
    GD_TRY(launch(h, "k_l2_chunk_scan", dim3(2 * cu8), dim3(MSD_NT), 0, k_l2_chunk_scan, l, hh, (const uint32_t*)ptot,
                  tot));
    return launch(h, "k_l2_chunk_scatter", dim3(2 * cu8), dim3(CH_NT), 0, k_l2_chunk_scatter<BALLOT>,
                  (const uint16_t*)kB, (const uint32_t*)vB, l, (const uint32_t*)hh, (const uint32_t*)tot, n, n_act, perm,
                  offsets, rank_out);
}


// Stable partition of indices 0..n-1 by min(acts[i], n_act).  rank_out (optional): the inverse
// permutation, rank_out[perm[p]] = p.  Forms with identical output: LSD passes of <= 8 bits plus the
// bucket starts (bucket_lsd); for batches of at least 2^20 messages the two-level forms -- one MSD pass
// + the in-LDS range sort for n_act < 1056 x 1024 (msd_bucket), two MSD passes + the level-2 work lists
// up to n_act < 2^28 (msd3_bucket).  GD_MSD=1 (default) times the two-level form against the LSD
// passes on the first launches of each batch shape (tune_choose, kind 4) and keeps the faster, 2
// always takes the two-level form.
int bucket_device(gd_handle* h, const uint32_t* acts, uint32_t n, uint32_t n_act, uint32_t* perm, uint32_t* offsets,
                  uint32_t* rank_out) {
    if (n_act == 0xFFFFFFFFu) return set_err(h, GD_EINVAL, "n_act too large");
    if (h->bstream && h->bstream != h->stream) {
        // the bucketing scratch is the bucket stream's (gd_set_bucket_stream): a bucketing enqueued on
        // another stream waits for it
        HIP_TRY(h, hipEventRecord(h->b_ev, h->bstream));
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->b_ev, 0));
    }
    StageTime stage(h, "stage:bucket");
    uint32_t a3 = 0, ra3 = 0;
    const bool one = (msd_unrouted_key(n_act) >> MSD_SHIFT) + 1 <= MSD_MAX_RANGES;
    const bool three = !one && msd3_split(n_act, &a3, &ra3);
    if (h->msd_mode && n >= (1u << 20) && (one || three)) {
        int meas = -1;
        // keyed by the batch size and by the messages a range holds (which decide whether ranges are
        // staged in LDS): a handle bucketing 16M messages over 1M and over 10k activations keeps one
        // choice for each
        const int per_range = bucket_sub(n, n_act);
        const int var = h->msd_mode == 2 ? 1 : tune_choose(h, 4, n, &meas, 2, per_range);
        CxMeasure mm(h, meas, n);
        // ranks by ds_add_rtn lane order (default) or by ballots (GD_OPT_STABLE_RANK 0; gd_create's
        // choice on a device without that order)
        if (var == 1 && h->radix_rank_atomic)
            return one ? msd_bucket<false>(h, acts, n, n_act, perm, offsets, rank_out)
                       : msd3_bucket<false>(h, acts, n, n_act, perm, offsets, rank_out);
        if (var == 1)
            return one ? msd_bucket<true>(h, acts, n, n_act, perm, offsets, rank_out)
                       : msd3_bucket<true>(h, acts, n, n_act, perm, offsets, rank_out);
        return bucket_lsd(h, acts, n, n_act, perm, offsets, rank_out);
    }
    return bucket_lsd(h, acts, n, n_act, perm, offsets, rank_out);
}

constexpr uint32_t RADIX_MAX_BITS = 8;   // widest LSD digit (9- and 10-bit digits measured slower at cfg 3)

int bucket_lsd(gd_handle* h, const uint32_t* acts, uint32_t n, uint32_t n_act, uint32_t* perm, uint32_t* offsets,
               uint32_t* rank_out) {
    const uint32_t n_off = n_act + 2;
    if (n == 0) return launch(h, "k_fill", dim3(blocks_for(n_off, BLOCK)), dim3(BLOCK), 0, k_fill_u32, offsets, n_off, n);
    // the first pass's histogram fills the starts (n = the empty-bucket value)
    const FillArgs fill{offsets, n_off, n};
    uint32_t key_bits = 1;
    while (key_bits < 32 && (n_act >> key_bits) != 0) ++key_bits;
    const uint32_t passes = (key_bits + RADIX_MAX_BITS - 1) / RADIX_MAX_BITS;
    const uint32_t bits = std::max<uint32_t>(4, (key_bits + passes - 1) / passes);
    GD_TRY(ensure(h, h->u32_a, (size_t)n * 4));
    GD_TRY(ensure(h, h->u32_b, (size_t)n * 4));
    GD_TRY(ensure(h, h->u32_c, (size_t)n * 4));
    GD_TRY(ensure(h, h->u32_d, (size_t)n * 4));
    uint32_t* kb[2] = {(uint32_t*)h->u32_a.p, (uint32_t*)h->u32_b.p};
    uint32_t* vb[2] = {(uint32_t*)h->u32_c.p, (uint32_t*)h->u32_d.p};
    const uint32_t* kin = acts;
    const uint32_t* vin = nullptr;
    // packed records between the passes (gd_radix.h Pack): the key bits above the first digit fit
    // a u16 and the index fits beside the first digit in a u32 (BASELINE cfg 2: 14 + 24 + 7 bits)
    uint32_t ib = 1;
    while (ib < 32 && ((n - 1) >> ib) != 0) ++ib;
    const bool pack = passes >= 2 && bits <= 8 &&
                      key_bits - bits <= 16 && ib + bits <= 32;
    for (uint32_t p = 0; p < passes; ++p) {
        uint32_t* kout = kb[p & 1];
        uint32_t* vout = (p + 1 == passes) ? perm : vb[p & 1];
        // the last pass writes the bucket starts itself (no sorted keys)
        const bool last = p + 1 == passes;
        const Pack pk{ib, bits, pack && p > 0, pack && p + 1 < passes};
        GD_TRY(radix_dispatch(h, (int)bits, kin, vin, n, n_act, p * bits, kout, vout, p == 0,
                              last ? offsets : nullptr, p + 1 == passes ? rank_out : nullptr,
                              p == 0 ? fill : FillArgs{nullptr, 0u, 0u}, pk));
        kin = kout;
        vin = vout;
    }
    // the last pass's digit spans <= RS_RANGE * RS_MAX_SUB activations: one workgroup per digit
    // range, carried by the pass's digit bases; a wider digit takes the device-wide scan
    const uint32_t last_shift = (passes - 1) * bits;
    if (h->last_totals && last_shift < 32 && (1u << last_shift) <= RS_RANGE * RS_MAX_SUB)
        return launch(h, "k_starts_rangescan", dim3((n_act >> last_shift) + 1), dim3(RS_THREADS), 0, k_starts_rangescan,
                      offsets, n_act + 1, last_shift, h->last_totals, h->last_digits);
    return scan_device<OpMin>(h, offsets, n_act + 1, true, true, "offsets");
}

template int scan_device<OpAdd>(gd_handle*, uint32_t*, uint32_t, bool, bool, const char*, uint32_t*);
template int scan_device<OpMin>(gd_handle*, uint32_t*, uint32_t, bool, bool, const char*, uint32_t*);

}  // namespace gdx
