// alga_amd/csrc/engine_gapped.hip -- C ABI of the gapped placement (include/alga_amd.h: alga_place_gapped_device, alga_write_gapped_tsv_device;
// kernels in gapped_kernels.hip).
//
// Host side: the checks run on workspaces and end in one read-back (the refusal flags, the indexed positions, the participating reads); only
// then are the result buffers touched, so a refused call leaves an earlier result as it was.  Then: the defaults, the dense list of the
// participating reads (flag, scan, scatter), the column array (k_pl_gather over the placement's col_off, into this stage's own buffer), the seed
// index over it (alga_seed_index, the engine's one index workspace), k_gp_score, k_gp_trace, the scan of the run counts (one word read back: the
// size of d_cigar), the compaction, the difference array and its scan, the cover.  The placement result is read, never written.
#include <hip/hip_runtime.h>

#include <chrono>

#include "engine_internal.h"
#include "correct_kernels.h"
#include "gapped_kernels.h"
#include "gfa_kernels.h"
#include "place_kernels.h"

using namespace alga;

namespace {

int check_params(alga_engine *e, const alga_gapped_params *p) {
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "gapped placement parameters must not be NULL");
    if (p->k < 8 || p->k > 31) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "gapped placement: k must be in [8, 31]");
    if (p->max_edits < 1 || p->max_edits > GP_MAX_EDITS) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "gapped placement: max_edits must be in [1, 15]");
    if (p->max_occ < 1 || p->max_occ > 65535) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "gapped placement: max_occ must be in [1, 65535]");
    if (p->flags) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "gapped placement: unknown flag");
    return ALGA_OK;
}

int gapped_impl(alga_engine *e, const alga_nodes *nodes, const uint32_t *d_words, const unsigned long long *d_begin, const int32_t *d_len, const alga_placements *pl,
                const alga_gapped_params *p, hipStream_t s, alga_gapped *out, alga_gapped_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t R = (uint64_t) pl->n_reads, T = (uint64_t) pl->n_targets, columns = pl->n_columns;
    int rc;
    AlgaEvents<5> evs;
    if ((rc = evs.create(e))) return rc;
    if ((rc = alga_ensure(e, e->gp_cnt, GP_COUNTERS * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->gp_flag, (R + 2) * sizeof(uint32_t)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->gp_cnt.p, *hc = e->h_counters;
    uint32_t *flag = (uint32_t *) e->gp_flag.p;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, GP_COUNTERS * sizeof(unsigned long long), s));
    const SeedReads rd{nodes->words, nodes->stride_words, nodes->len, R};

    // the checks: nothing of the result is written before their verdict
    if (R) {
        const CrReads c{const_cast<uint32_t *>(nodes->words), nodes->stride_words, nodes->len, R, p->k};
        launch_cr_twin(c, (uint32_t *) (cnt + GP_BAD_TWIN), s);
        if ((rc = alga_check_launch(e, "k_cr_twin"))) return rc;
    }
    launch_gp_target_check(d_len, pl->d_col_off, T, columns, p->k, cnt, s);
    if ((rc = alga_check_launch(e, "k_gp_target_check"))) return rc;
    launch_gp_flag(rd, pl->d_state, p->k, flag, cnt, s);
    if ((rc = alga_check_launch(e, "k_gp_flag"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, GP_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[GP_BAD_TWIN]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "gapped placement: a row 2r is not the reverse complement of row 2r + 1, their lengths differ, or a length exceeds the stride");
    if (hc[GP_BAD_TARGETS]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "gapped placement: the targets are not the placement's (a length differs from its col_off)");
    const uint64_t n_index = hc[GP_INDEX_POS], n_list = hc[GP_TRIED], skipped_long = hc[GP_SKIPPED_LONG];

    // from here on the result is rewritten
    e->gp_valid = false; e->gp_serial++;
    const size_t col_words = (size_t) ((columns + 15) >> 4) + 2;
    const int blocks = seed_blocks(n_list, e->n_cu);
    for (DevBuf *b : {&e->gp_target, &e->gp_rpos, &e->gp_end}) if ((rc = alga_ensure(e, *b, (R + 1) * sizeof(int32_t)))) return rc;
    for (DevBuf *b : {&e->gp_edits, &e->gp_state}) if ((rc = alga_ensure(e, *b, R + 16))) return rc;
    for (DevBuf *b : {&e->gp_pos, &e->gp_nruns, &e->gp_cigoff}) if ((rc = alga_ensure(e, *b, (R + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->gp_list, (n_list + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->gp_best, (n_list + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->gp_runs, (n_list * GP_MAX_RUNS + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->gp_cols, col_words * sizeof(uint32_t)))) return rc;
    for (DevBuf *b : {&e->gp_diff, &e->gp_scan, &e->gp_cover}) if ((rc = alga_ensure(e, *b, (columns + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->gp_tstat, (3 * T + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(std::max<uint64_t>(R + 1, columns + 1))))) return rc;
    uint32_t *pos = (uint32_t *) e->gp_pos.p, *list = (uint32_t *) e->gp_list.p, *cols = (uint32_t *) e->gp_cols.p, *n_runs = (uint32_t *) e->gp_nruns.p;
    uint32_t *cig_off = (uint32_t *) e->gp_cigoff.p, *runs = (uint32_t *) e->gp_runs.p, *diff = (uint32_t *) e->gp_diff.p, *scan = (uint32_t *) e->gp_scan.p;
    uint32_t *cover = (uint32_t *) e->gp_cover.p;
    unsigned long long *best = (unsigned long long *) e->gp_best.p, *tstat = (unsigned long long *) e->gp_tstat.p;
    const GpOut go{(int32_t *) e->gp_target.p, (int32_t *) e->gp_rpos.p, (int32_t *) e->gp_end.p, (uint8_t *) e->gp_edits.p, (uint8_t *) e->gp_state.p};

    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    for (int32_t *a : {go.target, go.pos, go.end}) HIP_TRY(e, hipMemsetAsync(a, 0xFF, (R + 1) * sizeof(int32_t), s));
    for (uint8_t *a : {go.edits, go.state}) HIP_TRY(e, hipMemsetAsync(a, 0, R + 16, s));
    HIP_TRY(e, hipMemsetAsync(n_runs, 0, (R + 2) * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(cig_off, 0, (R + 2) * sizeof(uint32_t), s));
    if (R) launch_exclusive_scan(flag, R + 1, pos, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(participating reads)"))) return rc;
    launch_gp_scatter(flag, pos, R, list, s);
    if ((rc = alga_check_launch(e, "k_gp_scatter"))) return rc;
    const SeedSpace tg{pl->d_col_off, d_len, (uint32_t) T, columns, cols};
    SeedIndex ix{};
    if (n_list) {                                                    // an empty pass builds no index
        HIP_TRY(e, hipMemsetAsync(cols, 0, col_words * sizeof(uint32_t), s));
        launch_pl_gather(d_words, d_begin, tg, cols, s);
        if ((rc = alga_check_launch(e, "k_pl_gather"))) return rc;
        if ((rc = alga_seed_index(e, tg, p->k, n_index, nullptr, s, &ix))) return rc;
    }
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    launch_gp_score(rd, tg, ix, p->k, p->max_edits, p->max_occ, list, n_list, go, best, blocks, cnt, s);
    if ((rc = alga_check_launch(e, "k_gp_score"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));

    launch_gp_trace(rd, tg, p->k, p->max_edits, list, n_list, best, go.state, runs, n_runs, cnt, s);
    if ((rc = alga_check_launch(e, "k_gp_trace"))) return rc;
    if (R) launch_exclusive_scan(n_runs, R + 1, cig_off, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(runs)"))) return rc;
    uint32_t n_cigar = 0;
    HIP_TRY(e, hipMemcpyAsync(&n_cigar, cig_off + R, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if ((rc = alga_ensure(e, e->gp_cigar, ((size_t) n_cigar + 4) * sizeof(uint32_t)))) return rc;
    launch_gp_cigar(list, n_list, runs, cig_off, (uint32_t *) e->gp_cigar.p, s);
    if ((rc = alga_check_launch(e, "k_gp_cigar"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[3], s));

    HIP_TRY(e, hipMemsetAsync(diff, 0, (columns + 4) * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(scan, 0, (columns + 4) * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(tstat, 0, (3 * T + 1) * sizeof(unsigned long long), s));
    launch_gp_depth_add(tg, list, n_list, go, diff, tstat, s);
    if ((rc = alga_check_launch(e, "k_gp_depth_add"))) return rc;
    // exclusive scan over columns + 1 differences: entry g + 1 is the gapped cover of column g
    if (columns) launch_exclusive_scan(diff, columns + 1, scan, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(cover)"))) return rc;
    launch_gp_cover(pl->d_cover, scan, columns, cover, s);
    if ((rc = alga_check_launch(e, "k_gp_cover"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[4], s));
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, GP_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->gp_valid = true; e->gp_reads = R; e->gp_targets = T; e->gp_columns = columns; e->gp_ncigar = n_cigar; e->gp_pl_serial = e->pl_serial;
    out->n_reads = (int64_t) R; out->n_targets = (int64_t) T; out->n_columns = columns; out->n_cigar = n_cigar;
    out->d_target = go.target; out->d_pos = go.pos; out->d_end = go.end; out->d_edits = go.edits; out->d_state = go.state;
    out->d_cigar_off = cig_off; out->d_cigar = (const uint32_t *) e->gp_cigar.p; out->d_cover = cover;
    out->d_t_reads = (const uint64_t *) tstat; out->d_t_bases = (const uint64_t *) (tstat + T); out->d_t_edits = (const uint64_t *) (tstat + 2 * T);
    e->gp_out = *out;                                                 // what alga_gapped_is_current compares a consumer's handle with
    if (info) {
        alga_gapped_info o{};
        o.tried = n_list; o.skipped_long = skipped_long; o.placed = hc[GP_PLACED]; o.unique = hc[GP_UNIQUE]; o.with_indel = hc[GP_WITH_INDEL]; o.edits = hc[GP_EDITS];
        o.insertions = hc[GP_INSERTIONS]; o.deletions = hc[GP_DELETIONS]; o.candidates = hc[GP_CANDIDATES]; o.seeds = hc[GP_SEEDS]; o.seeds_over_max_occ = hc[GP_SEEDS_OVER];
        if ((rc = evs.ms(e, 0, 1, &o.ms_index))) return rc;
        if ((rc = evs.ms(e, 1, 2, &o.ms_place))) return rc;
        if ((rc = evs.ms(e, 2, 3, &o.ms_trace))) return rc;
        if ((rc = evs.ms(e, 3, 4, &o.ms_depth))) return rc;
        o.ms_total = alga_ms_since(t0);
        *info = o;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" void alga_gapped_default_params(alga_gapped_params *p) {
    if (!p) return;
    *p = alga_gapped_params{};
    p->k = 21; p->max_edits = 6; p->max_occ = 256; p->flags = 0;
}

extern "C" int alga_place_gapped_device(alga_engine *e, const alga_nodes *nodes, const uint32_t *d_words, const uint64_t *d_begin, const int32_t *d_len, int32_t n_targets,
                                        const alga_placements *pl, const alga_gapped_params *p, void *hip_stream, alga_gapped *out, alga_gapped_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if (!nodes || !pl || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes, placements and out must not be NULL");
    if ((rc = alga_check_twin_nodes(e, nodes, true))) return rc;
    if (n_targets < 0 || (n_targets && (!d_words || !d_begin || !d_len))) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad target arrays");
    if (!alga_placement_is_current(e, pl)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last placement call on this engine");
    if ((int64_t) (nodes->n / 2) != pl->n_reads) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "gapped placement: the node set does not have the placement's reads (n / 2 != n_reads)");
    if ((int64_t) n_targets != pl->n_targets) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "gapped placement: the targets are not the placement's (n_targets differs)");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return gapped_impl(e, nodes, d_words, (const unsigned long long *) d_begin, d_len, pl, p, call.s, out, info);
}

extern "C" int alga_write_gapped_tsv_device(alga_engine *e, const alga_gapped *gp, const char *path, alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!gp || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "gapped placements and path must not be NULL");
    if (!e->gp_valid || gp->n_reads < 0 || (uint64_t) gp->n_reads != e->gp_reads || gp->n_cigar != e->gp_ncigar || gp->d_target != (const int32_t *) e->gp_target.p ||
        gp->d_pos != (const int32_t *) e->gp_rpos.p || gp->d_end != (const int32_t *) e->gp_end.p || gp->d_edits != (const uint8_t *) e->gp_edits.p ||
        gp->d_state != (const uint8_t *) e->gp_state.p || gp->d_cigar_off != (const uint32_t *) e->gp_cigoff.p || gp->d_cigar != (const uint32_t *) e->gp_cigar.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_place_gapped_device call on this engine");
    HIP_TRY(e, hipSetDevice(e->device));
    const GpTsv f{gp->d_target, gp->d_pos, gp->d_end, gp->d_edits, gp->d_state, gp->d_cigar_off, gp->d_cigar, (uint64_t) gp->n_reads};
    AlgaTextJob job;
    job.items = f.n;
    job.sizes = [f](uint32_t *o, unsigned long long *counters, hipStream_t s) { launch_gp_tsv_sizes(f, o, counters, s); };
    job.format = [f](const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) { launch_gp_tsv_write(f, off, i0, i1, buf, s); };
    job.kind = "TSV";
    return alga_text_job_run(e, job, path, info);
}
