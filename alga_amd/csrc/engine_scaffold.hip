// alga_amd/csrc/engine_scaffold.hip -- C ABI of the scaffolds (include/alga_amd.h: alga_scaffold_placed_device, alga_write_scaffold_fasta_device;
// kernels in scaffold_kernels.hip).
//
// Host side: the check runs on a workspace and ends in one read-back (the refusal flags); only then are the result buffers touched, so a refused
// call leaves an earlier result as it was.  Then: the link keys, a read-back of their count, sort_u64_u32 on the bits the keys use, the heads and
// their scan, a read-back of the bundle count (the bundle arrays are allocated at their size), the bundles with best / second per end, choice,
// joins, the two rounds of pointer jumping (cycles, then ranks and starts), the per-contig kernel, two scans and the layout.  The counters, the
// target lengths and the scaffold lengths come back at the end (the N50s are computed here).  No step walks on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "engine_internal.h"
#include "gfa_kernels.h"
#include "ingest_kernels.h"
#include "scaffold_kernels.h"

using namespace alga;

namespace {

int check_params(alga_engine *e, const alga_scaffold_params *p) {
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "scaffold parameters must not be NULL");
    if (p->insert < 0 || p->insert > (1 << 20)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "scaffold: insert must be in [0, 2^20]");
    if (p->max_insert < 1 || p->max_insert > (1 << 20)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "scaffold: max_insert must be in [1, 2^20]");
    if (p->min_links < 1) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "scaffold: min_links must be >= 1");
    if (p->max_second_percent < 1 || p->max_second_percent > 100) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "scaffold: max_second_percent must be in [1, 100]");
    if (p->min_gap < 1 || p->min_gap > (1 << 20)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "scaffold: min_gap must be in [1, 2^20]");
    if (p->flags || p->reserved[0] || p->reserved[1]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "scaffold: flags and reserved must be 0");
    return ALGA_OK;
}

int scaffold_impl(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const alga_placements *pl, const alga_scaffold_params *p, hipStream_t s,
                  alga_scaffolds *out, alga_scaffold_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t R = (uint64_t) pl->n_reads, T = (uint64_t) pl->n_targets, n_ends = 2 * T;
    int rc;
    AlgaEvents<3> evs;
    if ((rc = evs.create(e))) return rc;
    if ((rc = alga_ensure(e, e->sc_cnt, SC_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->sc_cnt.p, *hc = e->h_counters;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, SC_COUNTERS * sizeof(unsigned long long), s));
    const ScReads rd{nodes->len, nodes->stride_words, R, d_pair_off, pl->d_target, pl->d_pos, pl->d_state};
    const ScTargets tg{pl->d_col_off, (uint32_t) T};
    const uint32_t mb = (uint32_t) e->opt_scaffold_max_blocks;               // 8192 unless a test lowers it

    // the check: nothing of the result is written before its verdict
    launch_sc_check(rd, tg, cnt, mb, s);
    if ((rc = alga_check_launch(e, "k_sc_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, SC_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[SC_BAD] & SC_BAD_PAIR) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "scaffold: pair_off holds a value above 2, differs between a node and its twin, or names a mate that does not point back");
    if (hc[SC_BAD] & SC_BAD_LEN) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "scaffold: a uniquely placed read has a length below 1 or above 16 * stride_words");
    if (hc[SC_BAD] & SC_BAD_PLACE) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "scaffold: a uniquely placed read does not fit its placement: not the node set that was placed");

    // from here on the result is rewritten
    e->sc_valid = false;
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    uint64_t n_links = 0, n_bundles = 0;
    const bool paired = d_pair_off && R;
    if (paired) {
        int ebits = 1;
        while (ebits < 32 && (n_ends >> ebits)) ebits++;                     // the ends are below 2^ebits
        const unsigned long long sentinel = ebits < 32 ? 1ull << (32 + ebits) : ~0ull;
        const int bits = ebits < 32 ? 33 + ebits : 64;
        for (int j = 0; j < 2; j++) {
            if ((rc = alga_ensure(e, e->sc_keys[j], (R + 2) * sizeof(unsigned long long)))) return rc;
            if ((rc = alga_ensure(e, e->sc_vals[j], (R + 2) * sizeof(uint32_t)))) return rc;
        }
        if ((rc = alga_ensure(e, e->sc_span, (R + 2) * sizeof(uint32_t)))) return rc;
        launch_sc_links(rd, tg, p->max_insert, sentinel, (unsigned long long *) e->sc_keys[0].p, (uint32_t *) e->sc_vals[0].p, (uint32_t *) e->sc_span.p, cnt, mb, s);
        if ((rc = alga_check_launch(e, "k_sc_links"))) return rc;
        HIP_TRY(e, hipMemcpyAsync(hc, cnt, SC_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        n_links = hc[SC_LINKS];
        if (n_links) {
            const size_t temp = sort_u64_u32_temp_bytes(R);
            if ((rc = alga_ensure(e, e->sort_temp, temp))) return rc;
            if ((rc = alga_ensure(e, e->sc_heads, (n_links + 2) * sizeof(uint32_t)))) return rc;
            if ((rc = alga_ensure(e, e->sc_pos, (n_links + 2) * sizeof(uint32_t)))) return rc;
            if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(n_links + 1)))) return rc;
            // the links come first: the sentinel is above every key
            HIP_TRY(e, sort_u64_u32(e->sort_temp.p, temp, (const unsigned long long *) e->sc_keys[0].p, (unsigned long long *) e->sc_keys[1].p, (const uint32_t *) e->sc_vals[0].p,
                                    (uint32_t *) e->sc_vals[1].p, R, bits, s));
            launch_sc_heads((const unsigned long long *) e->sc_keys[1].p, n_links, (uint32_t *) e->sc_heads.p, cnt, mb, s);
            if ((rc = alga_check_launch(e, "k_sc_heads"))) return rc;
            launch_exclusive_scan((const uint32_t *) e->sc_heads.p, n_links, (uint32_t *) e->sc_pos.p, (uint64_t *) e->scan_scratch.p, s);
            if ((rc = alga_check_launch(e, "scan(bundle heads)"))) return rc;
            HIP_TRY(e, hipMemcpyAsync(hc, cnt, SC_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
            HIP_TRY(e, hipStreamSynchronize(s));
            n_bundles = hc[SC_BUNDLES];
        }
    }

    // the bundle arrays at their size, the per-end workspaces
    for (DevBuf *b : {&e->sc_ba, &e->sc_bb, &e->sc_blinks, &e->sc_bgap, &e->sc_bstart}) if ((rc = alga_ensure(e, *b, (n_bundles + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->sc_bspan, (n_bundles + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->sc_bstate, n_bundles + 16))) return rc;
    if ((rc = alga_ensure(e, e->sc_best, (2 * n_ends + 2) * sizeof(unsigned long long)))) return rc;      // best, second
    if ((rc = alga_ensure(e, e->sc_choice, (n_ends + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->sc_partner, (2 * n_ends + 2) * sizeof(uint32_t)))) return rc;              // partner, join bundle
    if ((rc = alga_ensure(e, e->sc_estate, n_ends + 16))) return rc;
    ChainWork w;
    if ((rc = alga_chain_work(e, T, &w))) return rc;
    unsigned long long *best = (unsigned long long *) e->sc_best.p, *second = best + n_ends;
    uint32_t *choice = (uint32_t *) e->sc_choice.p, *partner = (uint32_t *) e->sc_partner.p, *join_bundle = partner + n_ends;
    const ScBundles bd{n_bundles, (uint32_t *) e->sc_ba.p, (uint32_t *) e->sc_bb.p, (uint32_t *) e->sc_blinks.p, (const unsigned long long *) e->sc_bspan.p,
                       (int32_t *) e->sc_bgap.p, (uint8_t *) e->sc_bstate.p};
    const ScParams sp{p->insert, p->min_links, p->max_second_percent, p->min_gap};
    HIP_TRY(e, hipMemsetAsync(e->sc_bspan.p, 0, (n_bundles + 1) * sizeof(unsigned long long), s));
    HIP_TRY(e, hipMemsetAsync(best, 0, (2 * n_ends + 2) * sizeof(unsigned long long), s));
    HIP_TRY(e, hipMemsetAsync(partner, 0xFF, (2 * n_ends + 2) * sizeof(uint32_t), s));
    if (n_bundles) {
        launch_sc_bundle_fill((const uint32_t *) e->sc_vals[1].p, (const uint32_t *) e->sc_span.p, (const uint32_t *) e->sc_heads.p, (const uint32_t *) e->sc_pos.p, n_links,
                              n_bundles, (uint32_t *) e->sc_bstart.p, (unsigned long long *) e->sc_bspan.p, mb, s);
        if ((rc = alga_check_launch(e, "k_sc_bundle_fill"))) return rc;
        launch_sc_bundles((const unsigned long long *) e->sc_keys[1].p, (const uint32_t *) e->sc_bstart.p, bd, sp, best, cnt, mb, s);
        if ((rc = alga_check_launch(e, "k_sc_bundles"))) return rc;
    }
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    launch_sc_second(bd, best, second, mb, s);
    if ((rc = alga_check_launch(e, "k_sc_second"))) return rc;
    launch_sc_choice(best, second, n_ends, p->max_second_percent, choice, (uint8_t *) e->sc_estate.p, cnt, mb, s);
    if ((rc = alga_check_launch(e, "k_sc_choice"))) return rc;
    launch_sc_joins(bd, choice, partner, join_bundle, mb, s);
    if ((rc = alga_check_launch(e, "k_sc_joins"))) return rc;

    // the joins into paths (the chain core, chain_kernels.h)
    const bool may_join = n_bundles && T;                                     // without a bundle there is no join: no cycle, and every path is one contig
    const ChainLists *l;
    if ((rc = alga_chain_cycles(e, w, partner, n_ends, may_join, mb, s, &l))) return rc;
    if (l) launch_sc_cycle_drop(*l, (uint32_t) T, partner, join_bundle, bd.state, cnt, mb, s);
    if ((rc = alga_check_launch(e, "k_sc_cycle_drop"))) return rc;
    launch_sc_rank_init(tg, partner, join_bundle, bd.gap, p->min_gap, w.set[0], mb, s);
    if ((rc = alga_chain_ranks(e, w, n_ends, may_join, mb, s, &l))) return rc;

    // the per-contig and per-scaffold arrays
    for (DevBuf *b : {&e->sc_scaffold, &e->sc_rank, &e->sc_gapafter, &e->sc_jlinks, &e->sc_smembers}) if ((rc = alga_ensure(e, *b, (T + 2) * sizeof(uint32_t)))) return rc;
    for (DevBuf *b : {&e->sc_start, &e->sc_slen}) if ((rc = alga_ensure(e, *b, (T + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->sc_orient, T + 16))) return rc;
    if ((rc = alga_ensure(e, e->sc_soff, (T + 2) * sizeof(uint32_t)))) return rc;
    const ScLayout lo{(int32_t *) e->sc_scaffold.p, (int32_t *) e->sc_rank.p, (uint8_t *) e->sc_orient.p, (unsigned long long *) e->sc_start.p, (int32_t *) e->sc_gapafter.p,
                      (uint32_t *) e->sc_jlinks.p, (uint32_t *) e->sc_soff.p, (int32_t *) e->sc_smembers.p, (unsigned long long *) e->sc_slen.p, (uint8_t *) e->sc_estate.p};
    launch_sc_place(tg, *l, partner, join_bundle, bd.gap, bd.links, p->min_gap, lo, w.head, w.first, w.members, cnt, mb, s);
    if ((rc = alga_check_launch(e, "k_sc_place"))) return rc;
    if ((rc = alga_chain_scans(e, w, T, "scan(scaffolds)", s))) return rc;
    launch_sc_layout(tg, *l, w.head, w.first_scan, w.members_scan, lo, cnt, mb, s);
    if ((rc = alga_check_launch(e, "k_sc_layout"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, SC_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t S = hc[SC_SCAFFOLDS];

    e->sc_valid = true; e->sc_targets = T; e->sc_scaffolds = S; e->sc_longest = hc[SC_LONGEST]; e->sc_pl_serial = e->pl_serial;
    out->n_targets = (int64_t) T; out->n_bundles = (int64_t) n_bundles; out->n_scaffolds = (int64_t) S; out->n_members = (int64_t) hc[SC_MEMBERS];
    out->d_b_a = bd.a; out->d_b_b = bd.b; out->d_b_links = bd.links; out->d_b_span = (const uint64_t *) bd.span; out->d_b_gap = bd.gap; out->d_b_state = bd.state;
    out->d_end_state = lo.end_state; out->d_scaffold = lo.scaffold; out->d_rank = lo.rank; out->d_orient = lo.orient; out->d_start = (const uint64_t *) lo.start;
    out->d_gap_after = lo.gap_after; out->d_join_links = lo.join_links; out->d_s_off = lo.s_off; out->d_s_members = lo.s_members; out->d_s_len = (const uint64_t *) lo.s_len;
    if (info) {
        alga_scaffold_info o{};
        o.pairs_split = hc[SC_SPLIT]; o.links = hc[SC_LINKS]; o.links_too_far = hc[SC_TOO_FAR]; o.bundles = n_bundles; o.bundles_supported = hc[SC_SUPPORTED];
        o.ends_ambiguous = hc[SC_AMBIGUOUS]; o.joins = hc[SC_JOINS]; o.joins_dropped_cycle = hc[SC_DROPPED]; o.scaffolds = S; o.scaffolds_multi = hc[SC_MULTI];
        o.longest = hc[SC_LONGEST];
        // the lengths for the N50s (no exception leaves the C ABI: a host allocation that fails is reported like a device one)
        try {
            std::vector<uint32_t> off(T + 1);
            std::vector<uint64_t> tl(T), sl(S);
            HIP_TRY(e, hipMemcpyAsync(off.data(), pl->d_col_off, (T + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            if (S) HIP_TRY(e, hipMemcpyAsync(sl.data(), lo.s_len, S * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(e, hipStreamSynchronize(s));
            for (uint64_t t = 0; t < T; t++) tl[t] = off[t + 1] - off[t];
            o.n50_targets = n50_of(std::move(tl)); o.n50_scaffolds = n50_of(std::move(sl));
        } catch (const std::bad_alloc &) {
            return alga_fail(e, ALGA_ERR_OUT_OF_MEMORY, "scaffold: no host memory for the lengths of the N50s");
        }
        if ((rc = evs.ms(e, 0, 1, &o.ms_links))) return rc;
        if ((rc = evs.ms(e, 1, 2, &o.ms_chain))) return rc;
        o.ms_total = alga_ms_since(t0);
        *info = o;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" void alga_scaffold_default_params(alga_scaffold_params *p) {
    if (!p) return;
    *p = alga_scaffold_params{};
    p->insert = 0; p->max_insert = 1000; p->min_links = 5; p->max_second_percent = 50; p->min_gap = 10; p->flags = 0;
}

extern "C" int alga_scaffold_placed_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const alga_placements *pl, const alga_scaffold_params *p,
                                           void *hip_stream, alga_scaffolds *out, alga_scaffold_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if (!nodes || !pl || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes, placements and out must not be NULL");
    if ((rc = alga_check_twin_nodes(e, nodes, false))) return rc;
    if (!alga_placement_is_current(e, pl)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last placement call on this engine");
    if ((int64_t) (nodes->n / 2) != pl->n_reads) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "scaffold: the node set does not have the placement's reads (n / 2 != n_reads)");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return scaffold_impl(e, nodes, d_pair_off, pl, p, call.s, out, info);
}

extern "C" int alga_write_scaffold_fasta_device(alga_engine *e, const alga_placements *pl, const alga_scaffolds *scaf, const alga_polished *pol, const char *path,
                                                alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!pl || !scaf || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "placements, scaffolds and path must not be NULL");
    if (!alga_placement_is_current(e, pl)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last placement call on this engine");
    if (!e->sc_valid || e->sc_pl_serial != e->pl_serial || scaf->n_targets < 0 || (uint64_t) scaf->n_targets != e->sc_targets || e->sc_targets != e->pl_targets ||
        scaf->n_scaffolds < 0 || (uint64_t) scaf->n_scaffolds != e->sc_scaffolds || scaf->d_s_off != (const uint32_t *) e->sc_soff.p ||
        scaf->d_s_members != (const int32_t *) e->sc_smembers.p || scaf->d_s_len != (const uint64_t *) e->sc_slen.p || scaf->d_start != (const uint64_t *) e->sc_start.p ||
        scaf->d_orient != (const uint8_t *) e->sc_orient.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_scaffold_placed_device call on this placement");
    if (pol && !alga_polished_is_current(e, pl, pol))
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_polish_placed_device call on this placement");
    if (e->sc_longest + 64 > 0xFFFFFFFFull) return alga_fail(e, ALGA_ERR_CAPACITY, "a scaffold record of more than 2^32 bytes");
    HIP_TRY(e, hipSetDevice(e->device));
    const ScFasta f{pol ? pol->d_words : (const uint32_t *) e->pl_cols.p, pl->d_col_off, scaf->d_s_off, scaf->d_s_members, (const unsigned long long *) scaf->d_s_len,
                    (const unsigned long long *) scaf->d_start, scaf->d_orient, (uint64_t) scaf->n_scaffolds,
                    e->opt_scaffold_max_blocks < 8192 ? (uint32_t) e->opt_scaffold_max_blocks : 16384u};   // the write grid's own cap unless a test lowers it
    return alga_text_records(e, f, launch_sc_fasta_sizes, launch_sc_fasta_write, path, info);
}
