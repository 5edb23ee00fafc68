// alga_amd/csrc/engine_polish.hip -- C ABI of the polish (include/alga_amd.h: alga_polish_placed_device, alga_write_polished_fasta_device;
// kernels in polish_kernels.hip).
//
// Host side: the check runs on a workspace and ends in one read-back (the refusal flags, the voters, the longest); only then are the result
// buffers touched, so a refused call leaves an earlier result as it was.  Then: the copy of col_off, (first column, node) of every read sorted
// on 32 bits, the two vote kernels, a read-back of the counters (the change list is allocated at its size), the scan of the popcounts and
// the change list.  `cur` is read from the placement's column array (e->pl_cols), never from the caller.
#include <hip/hip_runtime.h>

#include <chrono>

#include "engine_internal.h"
#include "gfa_kernels.h"
#include "polish_kernels.h"

using namespace alga;

namespace {

int check_params(alga_engine *e, const alga_polish_params *p) {
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "polish parameters must not be NULL");
    if (p->min_cover < 1) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "polish: min_cover must be >= 1");
    if (p->min_percent < 1 || p->min_percent > 100) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "polish: min_percent must be in [1, 100]");
    if (p->flags & ~(ALGA_POLISH_MULTI | ALGA_POLISH_COUNTS)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "polish: unknown flag");
    return ALGA_OK;
}

int polish_impl(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_polish_params *p, hipStream_t s, alga_polished *out, alga_polish_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t R = (uint64_t) pl->n_reads, T = (uint64_t) pl->n_targets, columns = pl->n_columns;
    const bool want_counts = (p->flags & ALGA_POLISH_COUNTS) != 0;
    int rc;
    AlgaEvents<3> evs;
    if ((rc = evs.create(e))) return rc;
    if ((rc = alga_ensure(e, e->po_cnt, PO_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->po_cnt.p, *hc = e->h_counters;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, PO_COUNTERS * sizeof(unsigned long long), s));
    const PoReads rd{nodes->words, nodes->stride_words, nodes->len, R, pl->d_target, pl->d_pos, pl->d_state,
                     (uint8_t) ((p->flags & ALGA_POLISH_MULTI) ? ALGA_PLACE_PLACED : ALGA_PLACE_UNIQUE)};
    const PoTargets tg{pl->d_col_off, (uint32_t) T, columns, (const uint32_t *) e->pl_cols.p};

    // the check: nothing of the result is written before its verdict
    launch_po_check(rd, tg, cnt, s);
    if ((rc = alga_check_launch(e, "k_po_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, PO_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[PO_BAD] & PO_BAD_COLUMNS) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "polish: n_columns is not the placement's col_off[n_targets]");
    if (hc[PO_BAD] & PO_BAD_LEN) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "polish: a voting node has a length below 1 or above 16 * stride_words");
    if (hc[PO_BAD] & PO_BAD_PLACE) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "polish: a voting node does not fit its placement: not the node set that was placed");
    const uint64_t voters = hc[PO_VOTERS], votes = hc[PO_VOTES], longest = hc[PO_MAX_LEN];

    // from here on the result is rewritten
    e->po_valid = false;
    const size_t n_words = (size_t) ((columns + 15) >> 4), col_words = n_words + 2;
    for (int j = 0; j < 2; j++) {
        if ((rc = alga_ensure(e, e->po_keys[j], (R + 4) * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->po_vals[j], (R + 4) * sizeof(uint32_t)))) return rc;
    }
    for (DevBuf *b : {&e->po_marks, &e->po_pop, &e->po_scan}) if ((rc = alga_ensure(e, *b, (n_words + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->po_coloff, (T + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->po_words, col_words * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->po_tstat, (2 * T + 1) * sizeof(unsigned long long)))) return rc;
    if (want_counts && (rc = alga_ensure(e, e->po_counts, (64 * n_words + 4) * sizeof(uint32_t)))) return rc;       // 16 bytes per column, whole words
    const size_t temp = rsort_u32_pairs_temp_bytes(R);
    if ((rc = alga_ensure(e, e->sort_temp, temp))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(n_words + 1)))) return rc;
    uint32_t *col_off = (uint32_t *) e->po_coloff.p, *words = (uint32_t *) e->po_words.p, *marks = (uint32_t *) e->po_marks.p, *pop = (uint32_t *) e->po_pop.p;
    unsigned long long *tstat = (unsigned long long *) e->po_tstat.p;

    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    HIP_TRY(e, hipMemcpyAsync(col_off, pl->d_col_off, (T + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    if (voters) {
        launch_po_keys(rd, tg, (uint32_t *) e->po_keys[0].p, (uint32_t *) e->po_vals[0].p, s);
        if ((rc = alga_check_launch(e, "k_po_keys"))) return rc;
        HIP_TRY(e, rsort_u32_pairs(e->sort_temp.p, temp, (const uint32_t *) e->po_keys[0].p, (uint32_t *) e->po_keys[1].p, (const uint32_t *) e->po_vals[0].p,
                                   (uint32_t *) e->po_vals[1].p, R, 0, s));
    }
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    HIP_TRY(e, hipMemsetAsync(tstat, 0, (2 * T + 1) * sizeof(unsigned long long), s));
    HIP_TRY(e, hipMemsetAsync(words + n_words, 0, 2 * sizeof(uint32_t), s));                 // the padding; every word before it is written by its lane
    const PoVote pv{(const uint32_t *) e->po_keys[1].p, (const uint32_t *) e->po_vals[1].p, (uint32_t) voters, (uint32_t) longest, p->min_cover, p->min_percent,
                    words, marks, pop, want_counts ? (uint32_t *) e->po_counts.p : nullptr, tstat, tstat + T};
    launch_po_vote(rd, tg, pv, cnt, s);
    if ((rc = alga_check_launch(e, "k_po_vote"))) return rc;
    launch_po_vote_wide(rd, tg, pv, cnt, s);
    if ((rc = alga_check_launch(e, "k_po_vote_wide"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, PO_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t n_changed = hc[PO_CHANGED];
    if ((rc = alga_ensure(e, e->po_ccols, (n_changed + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->po_cbases, n_changed + 16))) return rc;
    if (n_changed) {
        launch_exclusive_scan(pop, n_words, (uint32_t *) e->po_scan.p, (uint64_t *) e->scan_scratch.p, s);
        if ((rc = alga_check_launch(e, "scan(changed columns)"))) return rc;
        launch_po_changes(tg, words, marks, (const uint32_t *) e->po_scan.p, (uint32_t *) e->po_ccols.p, (uint8_t *) e->po_cbases.p, s);
        if ((rc = alga_check_launch(e, "k_po_changes"))) return rc;
    }
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->po_valid = true; e->po_targets = T; e->po_columns = columns; e->po_final_epoch = e->pl_final_epoch; e->po_pl_serial = e->pl_serial;
    out->n_targets = (int64_t) T; out->n_columns = columns; out->n_changed = n_changed;
    out->d_col_off = col_off; out->d_words = words; out->d_changed_cols = (const uint32_t *) e->po_ccols.p; out->d_changed_bases = (const uint8_t *) e->po_cbases.p;
    out->d_t_changed = (const uint64_t *) tstat; out->d_t_ambiguous = (const uint64_t *) (tstat + T);
    out->d_counts = want_counts ? (const uint32_t *) e->po_counts.p : nullptr;
    e->po_out = *out;                                                 // what alga_polished_is_current compares a consumer's handle with
    if (info) {
        alga_polish_info o{};
        o.columns = columns; o.voters = voters; o.votes = votes; o.voted_columns = hc[PO_VOTED]; o.changed = n_changed; o.ambiguous = hc[PO_AMBIGUOUS];
        o.max_cover = hc[PO_MAX_COVER];
        if ((rc = evs.ms(e, 0, 1, &o.ms_sort))) return rc;
        if ((rc = evs.ms(e, 1, 2, &o.ms_vote))) return rc;
        o.ms_total = alga_ms_since(t0);
        *info = o;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" void alga_polish_default_params(alga_polish_params *p) {
    if (!p) return;
    *p = alga_polish_params{};
    p->min_cover = 3; p->min_percent = 60; p->flags = 0;
}

extern "C" int alga_polish_placed_device(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_polish_params *p, void *hip_stream,
                                         alga_polished *out, alga_polish_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if (!nodes || !pl || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes, placements and out must not be NULL");
    if ((rc = alga_check_twin_nodes(e, nodes, true))) return rc;
    if (!alga_placement_is_current(e, pl)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last placement call on this engine");
    if ((int64_t) (nodes->n / 2) != pl->n_reads) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "polish: the node set does not have the placement's reads (n / 2 != n_reads)");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return polish_impl(e, nodes, pl, p, call.s, out, info);
}

extern "C" int alga_write_polished_fasta_device(alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, const alga_final_contigs *fin, const alga_placements *pl,
                                                const alga_polished *pol, int32_t depth_header, const char *path, alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!u || !cons || !fin || !pl || !pol || !path || !*path)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unitigs, consensus, final contigs, placements, polished and path must not be NULL");
    const char *why = nullptr;
    if (!alga_final_is_current(e, u, cons, fin, &why)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, why);
    if (!alga_placement_is_current(e, pl) || e->pl_final_epoch == 0 || e->pl_final_epoch != e->fc_epoch || e->pl_targets != (uint64_t) fin->n_accepted)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_place_reads_on_final_device call on this final result");
    // the polish is the engine's, and matched on what makes the records safe to format: the final result's epoch, the targets and columns (a polish
    // of an earlier placement on the same final result has them: this writer, alone, does not ask for the placement's serial)
    if (!e->po_valid || !alga_same_handle(pol, e->po_out) || e->po_final_epoch != e->pl_final_epoch || e->po_targets != e->pl_targets || pol->n_columns != pl->n_columns)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_polish_placed_device call on this placement");
    HIP_TRY(e, hipSetDevice(e->device));
    const PoFasta f{pol->d_words, pol->d_col_off, fin->d_verdict, fin->d_order, (const unsigned long long *) pl->d_t_reads, (const unsigned long long *) pl->d_t_bases,
                    (uint64_t) fin->n_accepted, depth_header};
    return alga_text_records(e, f, launch_po_fasta_sizes, launch_po_fasta_write, path, info);
}
