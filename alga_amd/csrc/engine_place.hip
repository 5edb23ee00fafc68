// alga_amd/csrc/engine_place.hip -- C ABI of the read placement (include/alga_amd.h: alga_place_reads_device, alga_place_reads_on_final_device,
// alga_write_final_fasta_depth_device; kernels in place_kernels.hip).
//
// Host side: the checks run on workspaces and end in one read-back (the refusal flags, the number of columns and of indexed positions, the
// longest read); only then are the result buffers touched, so a refused call leaves an earlier result as it was.  Then: scan of the target
// lengths, the column array, the seed index over it (alga_seed_index), k_pl_place, the difference array and its
// scan, the per-target sums, the pairs; the counters and the histogram come back at the end.
#include <hip/hip_runtime.h>

#include <chrono>
#include <vector>

#include "engine_internal.h"
#include "correct_kernels.h"
#include "gfa_kernels.h"
#include "ingest_kernels.h"
#include "place_kernels.h"

using namespace alga;

namespace {

int check_params(alga_engine *e, const alga_place_params *p) {
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "placement parameters must not be NULL");
    if (p->k < 8 || p->k > 31) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "placement: k must be in [8, 31]");
    if (p->max_mismatches < 0 || p->max_mismatches > 254) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "placement: max_mismatches must be in [0, 254]");
    if (p->max_occ < 1 || p->max_occ > 65535) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "placement: max_occ must be in [1, 65535]");
    if (p->max_insert < 1 || p->max_insert > (1 << 20)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "placement: max_insert must be in [1, 2^20]");
    if (p->flags & ~ALGA_PLACE_DEPTH_MULTI) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "placement: unknown flag");
    return ALGA_OK;
}

int check_nodes(alga_engine *e, const alga_nodes *nodes) {
    if (!nodes) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes must not be NULL");
    return alga_check_twin_nodes(e, nodes, true);
}

int place_impl(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const uint32_t *d_words, const unsigned long long *d_begin, const int32_t *d_len,
               int32_t n_targets, const alga_place_params *p, hipStream_t s, uint64_t final_epoch, alga_placements *out, alga_place_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = (uint64_t) nodes->n, R = n / 2, T = (uint64_t) n_targets;
    int rc;
    AlgaEvents<4> evs;
    if ((rc = evs.create(e))) return rc;
    if ((rc = alga_ensure(e, e->pl_cnt, PL_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->pl_cnt.p, *hc = e->h_counters;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, PL_COUNTERS * sizeof(unsigned long long), s));

    // the checks: nothing of the result is written before their verdict
    if (R) {
        const CrReads c{const_cast<uint32_t *>(nodes->words), nodes->stride_words, nodes->len, R, p->k};
        launch_cr_twin(c, (uint32_t *) (cnt + PL_BAD_TWIN), s);
        if ((rc = alga_check_launch(e, "k_cr_twin"))) return rc;
        launch_pl_node_check(d_pair_off, nodes->len, n, cnt, s);
        if ((rc = alga_check_launch(e, "k_pl_node_check"))) return rc;
    }
    launch_pl_target_check(d_len, T, p->k, cnt, s);
    if ((rc = alga_check_launch(e, "k_pl_target_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, PL_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[PL_BAD_TWIN]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "placement: a row 2r is not the reverse complement of row 2r + 1, their lengths differ, or a length exceeds the stride");
    if (hc[PL_BAD_PAIR]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "placement: pair_off holds a value above 2, differs between a node and its twin, or names a mate that does not point back");
    if (hc[PL_BAD_LEN]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "placement: negative target length");
    const uint64_t columns = hc[PL_COLUMNS], n_index = hc[PL_INDEX_POS];
    const int64_t max_read_len = (int64_t) hc[PL_MAX_READ_LEN];
    if (columns > 0xFFFFFFFEull) return alga_fail(e, ALGA_ERR_CAPACITY, "placement: the targets hold more than 2^32 - 2 bases");

    // from here on the result is rewritten
    e->pl_valid = false; e->pl_serial++;
    const size_t col_words = (size_t) ((columns + 15) >> 4) + 2, n_hist = (size_t) p->max_insert + 1;
    const int blocks = seed_blocks(R, e->n_cu);
    const size_t ub_words = seed_scratch_words(blocks, max_read_len, p->k);
    for (DevBuf *b : {&e->pl_target, &e->pl_pos}) if ((rc = alga_ensure(e, *b, (R + 1) * sizeof(int32_t)))) return rc;
    for (DevBuf *b : {&e->pl_mm, &e->pl_hits, &e->pl_state}) if ((rc = alga_ensure(e, *b, R + 16))) return rc;
    if ((rc = alga_ensure(e, e->pl_coloff, (T + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->pl_cover, (columns + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->pl_diff, (columns + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->pl_tstat, (4 * T + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->pl_hist, n_hist * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->pl_cols, col_words * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->seed_ub, ub_words * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(std::max<uint64_t>(T + 1, columns + 1))))) return rc;
    uint32_t *col_off = (uint32_t *) e->pl_coloff.p, *cols = (uint32_t *) e->pl_cols.p, *scan = (uint32_t *) e->pl_cover.p, *diff = (uint32_t *) e->pl_diff.p;
    unsigned long long *tstat = (unsigned long long *) e->pl_tstat.p, *hist = (unsigned long long *) e->pl_hist.p;

    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    // col_off[0 .. T]: the scan leaves the total behind the last entry
    HIP_TRY(e, hipMemsetAsync(col_off, 0, (T + 2) * sizeof(uint32_t), s));
    if (T) launch_exclusive_scan((const uint32_t *) d_len, T, col_off, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(target lengths)"))) return rc;
    const PlTargets tg{col_off, d_len, (uint32_t) T, columns, cols};
    HIP_TRY(e, hipMemsetAsync(cols, 0, col_words * sizeof(uint32_t), s));
    launch_pl_gather(d_words, d_begin, tg, cols, s);
    if ((rc = alga_check_launch(e, "k_pl_gather"))) return rc;
    SeedIndex ix;
    if ((rc = alga_seed_index(e, tg, p->k, n_index, cnt + PL_DISTINCT, s, &ix))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    const SeedReads rd{nodes->words, nodes->stride_words, nodes->len, R};
    const PlOut po{(int32_t *) e->pl_target.p, (int32_t *) e->pl_pos.p, (uint8_t *) e->pl_mm.p, (uint8_t *) e->pl_hits.p, (uint8_t *) e->pl_state.p};
    launch_pl_place(rd, tg, ix, p->k, p->max_mismatches, p->max_occ, po, (unsigned long long *) e->seed_ub.p, (uint32_t) (ub_words / ((size_t) blocks * SEED_WAVES)), blocks, cnt, s);
    if ((rc = alga_check_launch(e, "k_pl_place"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));

    HIP_TRY(e, hipMemsetAsync(diff, 0, (columns + 4) * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(scan, 0, (columns + 4) * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(tstat, 0, (4 * T + 1) * sizeof(unsigned long long), s));
    HIP_TRY(e, hipMemsetAsync(hist, 0, n_hist * sizeof(unsigned long long), s));
    launch_pl_depth_add(rd, tg, po, (p->flags & ALGA_PLACE_DEPTH_MULTI) ? 1 : 0, diff, tstat, s);
    if ((rc = alga_check_launch(e, "k_pl_depth_add"))) return rc;
    // exclusive scan over columns + 1 differences: entry g + 1 is the cover of column g
    if (columns) launch_exclusive_scan(diff, columns + 1, scan, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(cover)"))) return rc;
    launch_pl_uncovered(tg, scan + 1, tstat, s);
    if ((rc = alga_check_launch(e, "k_pl_uncovered"))) return rc;
    launch_pl_pairs(rd, d_pair_off, po, p->max_insert, hist, cnt, s);
    if ((rc = alga_check_launch(e, "k_pl_pairs"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[3], s));
    std::vector<unsigned long long> h(n_hist);
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, PL_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(h.data(), hist, n_hist * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->pl_valid = true; e->pl_targets = T; e->pl_reads = R; e->pl_ncolumns = columns; e->pl_nhist = n_hist; e->pl_final_epoch = final_epoch;
    out->n_reads = (int64_t) R; out->n_targets = (int64_t) T; out->n_columns = columns; out->n_hist = (int64_t) n_hist;
    out->d_target = po.target; out->d_pos = po.pos; out->d_mm = po.mm; out->d_hits = po.hits; out->d_state = po.state;
    out->d_col_off = col_off; out->d_cover = scan + 1;
    out->d_t_reads = (const uint64_t *) tstat; out->d_t_bases = (const uint64_t *) (tstat + T); out->d_t_mismatches = (const uint64_t *) (tstat + 2 * T);
    out->d_t_uncovered = (const uint64_t *) (tstat + 3 * T); out->d_insert_hist = (const uint64_t *) hist;
    e->pl_out = *out;                                                 // what alga_placement_is_current compares a consumer's handle with
    if (info) {
        alga_place_info o{};
        o.reads = R; o.placed = hc[PL_PLACED]; o.unique = hc[PL_UNIQUE]; o.multi = o.placed - o.unique; o.unplaced = R - o.placed;
        o.hits_saturated = hc[PL_SATURATED]; o.seeds = hc[PL_SEEDS]; o.seeds_over_max_occ = hc[PL_SEEDS_OVER];
        o.index_positions = n_index; o.index_distinct = hc[PL_DISTINCT];
        o.pairs = hc[PL_PAIRS]; o.pairs_proper = hc[PL_PROPER]; o.pairs_improper = hc[PL_IMPROPER]; o.pairs_split = hc[PL_SPLIT]; o.pairs_not_unique = hc[PL_NOT_UNIQUE];
        o.insert_median = -1; o.insert_mean_x100 = -1;
        if (o.pairs_proper) {
            const unsigned long long half = (o.pairs_proper + 1) / 2;
            unsigned long long cum = 0;
            for (size_t i = 0; i < n_hist; i++) { cum += h[i]; if (cum >= half) { o.insert_median = (int64_t) i; break; } }
            o.insert_mean_x100 = (int64_t) ((100ull * hc[PL_INSERT_SUM]) / o.pairs_proper);
        }
        if ((rc = evs.ms(e, 0, 1, &o.ms_index))) return rc;
        if ((rc = evs.ms(e, 1, 2, &o.ms_place))) return rc;
        if ((rc = evs.ms(e, 2, 3, &o.ms_depth))) return rc;
        o.ms_total = alga_ms_since(t0);
        *info = o;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" void alga_place_default_params(alga_place_params *p) {
    if (!p) return;
    *p = alga_place_params{};
    p->k = 21; p->max_mismatches = 4; p->max_occ = 256; p->max_insert = 1000; p->flags = 0;
}

extern "C" int alga_place_reads_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const uint32_t *d_words, const uint64_t *d_begin,
                                       const int32_t *d_len, int32_t n_targets, const alga_place_params *p, void *hip_stream, alga_placements *out, alga_place_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if ((rc = check_nodes(e, nodes))) return rc;
    if (!out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "out must not be NULL");
    if (n_targets < 0 || (n_targets && (!d_words || !d_begin || !d_len))) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad target arrays");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return place_impl(e, nodes, d_pair_off, d_words, (const unsigned long long *) d_begin, d_len, n_targets, p, call.s, 0, out, info);
}

extern "C" int alga_place_reads_on_final_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const alga_unitigs *u, const alga_consensus *cons,
                                                const alga_final_contigs *fin, const alga_place_params *p, void *hip_stream, alga_placements *out, alga_place_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if ((rc = check_nodes(e, nodes))) return rc;
    if (!u || !cons || !fin || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unitigs, consensus, final contigs and out must not be NULL");
    const char *why = nullptr;
    if (!alga_final_is_current(e, u, cons, fin, &why)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, why);
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    hipStream_t s = call.s;
    const uint64_t T = (uint64_t) fin->n_accepted;
    if ((rc = alga_ensure(e, e->pl_fbegin, (T + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->pl_flen, (T + 1) * sizeof(int32_t)))) return rc;
    launch_pl_final_targets((const unsigned long long *) u->d_word_off, fin->d_verdict, fin->d_order, fin->d_begin, fin->d_len, T, (unsigned long long *) e->pl_fbegin.p,
                            (int32_t *) e->pl_flen.p, s);
    if ((rc = alga_check_launch(e, "k_pl_final_targets"))) return rc;
    return place_impl(e, nodes, d_pair_off, cons->d_words, (const unsigned long long *) e->pl_fbegin.p, (const int32_t *) e->pl_flen.p, (int32_t) T, p, s, e->fc_epoch, out, info);
}

extern "C" int alga_write_final_fasta_depth_device(alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, const alga_final_contigs *fin,
                                                   const alga_placements *pl, const char *path, alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!u || !cons || !fin || !pl || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unitigs, consensus, final contigs, placements and path must not be NULL");
    const char *why = nullptr;
    if (!alga_final_is_current(e, u, cons, fin, &why)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, why);
    if (!alga_placement_is_current(e, pl) || e->pl_final_epoch == 0 || e->pl_final_epoch != e->fc_epoch || e->pl_targets != (uint64_t) fin->n_accepted)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_place_reads_on_final_device call on this final result");
    HIP_TRY(e, hipSetDevice(e->device));
    const PlFasta f{cons->d_words, (const unsigned long long *) u->d_word_off, fin->d_verdict, fin->d_order, fin->d_begin, fin->d_len,
                    (const unsigned long long *) pl->d_t_reads, (const unsigned long long *) pl->d_t_bases, (uint64_t) fin->n_accepted};
    return alga_text_records(e, f, launch_pl_fasta_sizes, launch_pl_fasta_write, path, info);
}
