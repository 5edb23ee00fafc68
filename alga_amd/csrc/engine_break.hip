// alga_amd/csrc/engine_break.hip -- C ABI of the break stage (include/alga_amd.h: alga_break_placed_device, alga_write_broken_fasta_device;
// kernels in break_kernels.hip).
//
// Host side: the check runs on a workspace and ends in one read-back (the refusal flags); only then are the result buffers touched, so a refused
// call leaves an earlier result as it was.  Then: the pair pass into the difference array, its scan (the span), the flags per column and the
// scan of the run starts, a read-back of the run count (the run arrays are allocated at their size), first / last / closed per run and the scan
// of the closed ones, a read-back of the cut count (the cut and piece arrays are allocated at their size), the cuts, the pieces and the copy
// of the bases.  The counters come back at the end; the lengths for the N50s only when `info` is given.  No step walks on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "engine_internal.h"
#include "gfa_kernels.h"
#include "break_kernels.h"

using namespace alga;

namespace {

int check_params(alga_engine *e, const alga_break_params *p) {
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "break parameters must not be NULL");
    if (p->min_span < 1) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "break: min_span must be >= 1");
    if (p->inset < 0 || p->inset > (1 << 20)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "break: inset must be in [0, 2^20]");
    if (p->margin < 0 || p->margin > (1 << 20)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "break: margin must be in [0, 2^20]");
    if (p->flags || p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "break: flags and reserved must be 0");
    return ALGA_OK;
}

int break_impl(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const alga_placements *pl, const alga_polished *pol, const alga_break_params *p,
               hipStream_t s, alga_broken *out, alga_break_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t R = (uint64_t) pl->n_reads, T = (uint64_t) pl->n_targets, C = pl->n_columns;
    int rc;
    AlgaEvents<3> evs;
    if ((rc = evs.create(e))) return rc;
    if ((rc = alga_ensure(e, e->br_cnt, BR_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->br_cnt.p, *hc = e->h_counters;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, BR_COUNTERS * sizeof(unsigned long long), s));
    const BrReads rd{nodes->len, nodes->stride_words, R, d_pair_off, pl->d_target, pl->d_pos, pl->d_state};
    const BrTargets tg{pl->d_col_off, (uint32_t) T, C};

    // the check: nothing of the result is written before its verdict
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    launch_br_check(rd, tg, cnt, s);
    if ((rc = alga_check_launch(e, "k_br_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, BR_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[BR_BAD] & BR_BAD_COLUMNS) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "break: n_columns is not the placement's col_off[n_targets]");
    if (hc[BR_BAD] & BR_BAD_PAIR) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "break: pair_off holds a value above 2, differs between a node and its twin, or names a mate that does not point back");
    if (hc[BR_BAD] & BR_BAD_LEN) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "break: a uniquely placed read has a length below 1 or above 16 * stride_words");
    if (hc[BR_BAD] & BR_BAD_PLACE) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "break: a uniquely placed read does not fit its placement: not the node set that was placed");

    // from here on the result is rewritten
    e->br_valid = false;
    const size_t col_words = (size_t) ((C + 15) >> 4) + 2;
    if ((rc = alga_ensure(e, e->br_diff, (C + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->br_span, (C + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->br_starts, (C + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->br_rpos, (C + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->br_marks, C + 16))) return rc;
    if ((rc = alga_ensure(e, e->br_tcuts, (T + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->br_words, col_words * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(C + 2)))) return rc;
    uint32_t *diff = (uint32_t *) e->br_diff.p, *scan = (uint32_t *) e->br_span.p, *starts = (uint32_t *) e->br_starts.p, *rpos = (uint32_t *) e->br_rpos.p;
    uint8_t *marks = (uint8_t *) e->br_marks.p;
    HIP_TRY(e, hipMemsetAsync(diff, 0, (C + 4) * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(scan, 0, (C + 4) * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(e->br_tcuts.p, 0, (T + 2) * sizeof(uint32_t), s));
    launch_br_pairs(rd, tg, (int32_t) (pl->n_hist - 1), p->inset, diff, cnt, s);
    if ((rc = alga_check_launch(e, "k_br_pairs"))) return rc;
    // exclusive scan over columns + 1 differences: entry g + 1 is the span of column g
    if (C) launch_exclusive_scan(diff, C + 1, scan, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(span)"))) return rc;
    const uint32_t *span = scan + 1;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    launch_br_flags(tg, span, (uint32_t) p->min_span, (uint32_t) p->margin, starts, marks, cnt, s);
    if ((rc = alga_check_launch(e, "k_br_flags"))) return rc;
    if (C) launch_exclusive_scan(starts, C + 1, rpos, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(run starts)"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, BR_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t n_runs = hc[BR_RUNS];

    uint64_t n_cuts = 0;
    for (DevBuf *b : {&e->br_rfirst, &e->br_rlast, &e->br_closed, &e->br_cpos}) if ((rc = alga_ensure(e, *b, (n_runs + 2) * sizeof(uint32_t)))) return rc;
    if (n_runs) {
        if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(n_runs + 2)))) return rc;
        for (DevBuf *b : {&e->br_rfirst, &e->br_rlast}) HIP_TRY(e, hipMemsetAsync(b->p, 0, (n_runs + 2) * sizeof(uint32_t), s));
        launch_br_runs(tg, rpos, marks, n_runs, (uint32_t *) e->br_rfirst.p, (uint32_t *) e->br_rlast.p, s);
        if ((rc = alga_check_launch(e, "k_br_runs"))) return rc;
        launch_br_closed((const uint32_t *) e->br_rfirst.p, (const uint32_t *) e->br_rlast.p, marks, n_runs, (uint32_t *) e->br_closed.p, cnt, s);
        if ((rc = alga_check_launch(e, "k_br_closed"))) return rc;
        launch_exclusive_scan((const uint32_t *) e->br_closed.p, n_runs + 1, (uint32_t *) e->br_cpos.p, (uint64_t *) e->scan_scratch.p, s);
        if ((rc = alga_check_launch(e, "scan(closed runs)"))) return rc;
        HIP_TRY(e, hipMemcpyAsync(hc, cnt, BR_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        n_cuts = hc[BR_CUTS];
    }

    // the cut and piece arrays at their size
    const uint64_t n_pieces = T + n_cuts;
    for (DevBuf *b : {&e->br_ccols, &e->br_cfirst, &e->br_clast}) if ((rc = alga_ensure(e, *b, (n_cuts + 2) * sizeof(uint32_t)))) return rc;
    for (DevBuf *b : {&e->br_poff, &e->br_len, &e->br_ptarget, &e->br_pstart}) if ((rc = alga_ensure(e, *b, (n_pieces + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->br_begin, (n_pieces + 2) * sizeof(unsigned long long)))) return rc;
    const BrCuts ct{n_cuts, (uint32_t *) e->br_ccols.p, (uint32_t *) e->br_cfirst.p, (uint32_t *) e->br_clast.p, (uint32_t *) e->br_tcuts.p};
    const BrPieces pc{(uint32_t *) e->br_poff.p, (unsigned long long *) e->br_begin.p, (int32_t *) e->br_len.p, (int32_t *) e->br_ptarget.p, (uint32_t *) e->br_pstart.p};
    launch_br_cuts(tg, (const uint32_t *) e->br_rfirst.p, (const uint32_t *) e->br_rlast.p, (const uint32_t *) e->br_closed.p, (const uint32_t *) e->br_cpos.p, n_runs, ct, s);
    if ((rc = alga_check_launch(e, "k_br_cuts"))) return rc;
    launch_br_pieces(tg, ct, pc, cnt, s);
    if ((rc = alga_check_launch(e, "k_br_pieces"))) return rc;
    launch_br_copy(pol ? pol->d_words : (const uint32_t *) e->pl_cols.p, C, (uint32_t *) e->br_words.p, s);
    if ((rc = alga_check_launch(e, "k_br_copy"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, BR_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->br_valid = true; e->br_targets = T; e->br_pieces = n_pieces; e->br_cuts = n_cuts; e->br_columns = C; e->br_longest = hc[BR_LONGEST];
    out->n_targets = (int64_t) T; out->n_pieces = (int64_t) n_pieces; out->n_cuts = (int64_t) n_cuts; out->n_columns = C;
    out->d_span = span; out->d_cut_cols = ct.cols; out->d_cut_first = ct.first; out->d_cut_last = ct.last; out->d_t_cuts = ct.t_cuts;
    out->d_piece_off = pc.piece_off; out->d_begin = (const uint64_t *) pc.begin; out->d_len = pc.len; out->d_piece_target = pc.piece_target;
    out->d_piece_start = pc.piece_start; out->d_words = (const uint32_t *) e->br_words.p;
    if (info) {
        alga_break_info o{};
        o.pairs_proper = hc[BR_PROPER]; o.pairs_spanning = hc[BR_SPANNING]; o.candidate_columns = hc[BR_CANDIDATES]; o.weak_columns = hc[BR_WEAK];
        o.runs = n_runs; o.runs_open = n_runs - n_cuts; o.cuts = n_cuts; o.targets_cut = hc[BR_TARGETS_CUT]; o.pieces = n_pieces;
        o.max_span = hc[BR_MAX_SPAN]; o.longest_piece = hc[BR_LONGEST];
        // the lengths for the N50s (no exception leaves the C ABI: a host allocation that fails is reported like a device one)
        try {
            std::vector<uint32_t> off(T + 1), poff(n_pieces + 1);
            std::vector<uint64_t> tl(T), plen(n_pieces);
            HIP_TRY(e, hipMemcpyAsync(off.data(), pl->d_col_off, (T + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(e, hipMemcpyAsync(poff.data(), pc.piece_off, (n_pieces + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(e, hipStreamSynchronize(s));
            for (uint64_t t = 0; t < T; t++) tl[t] = off[t + 1] - off[t];
            for (uint64_t j = 0; j < n_pieces; j++) plen[j] = poff[j + 1] - poff[j];
            o.n50_targets = n50_of(std::move(tl)); o.n50_pieces = n50_of(std::move(plen));
        } catch (const std::bad_alloc &) {
            return alga_fail(e, ALGA_ERR_OUT_OF_MEMORY, "break: no host memory for the lengths of the N50s");
        }
        if ((rc = evs.ms(e, 0, 1, &o.ms_span))) return rc;
        if ((rc = evs.ms(e, 1, 2, &o.ms_cut))) return rc;
        o.ms_total = alga_ms_since(t0);
        *info = o;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" void alga_break_default_params(alga_break_params *p) {
    if (!p) return;
    *p = alga_break_params{};
    p->min_span = 1; p->inset = 21; p->margin = 0; p->flags = 0;
}

extern "C" int alga_break_placed_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const alga_placements *pl, const alga_polished *pol,
                                        const alga_break_params *p, void *hip_stream, alga_broken *out, alga_break_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if (!nodes || !pl || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes, placements and out must not be NULL");
    if ((rc = alga_check_twin_nodes(e, nodes, false))) return rc;
    if (!alga_placement_is_current(e, pl)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last placement call on this engine");
    if ((int64_t) (nodes->n / 2) != pl->n_reads) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "break: the node set does not have the placement's reads (n / 2 != n_reads)");
    if (pol && !alga_polished_is_current(e, pl, pol))
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_polish_placed_device call on this placement");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return break_impl(e, nodes, d_pair_off, pl, pol, p, call.s, out, info);
}

extern "C" int alga_write_broken_fasta_device(alga_engine *e, const alga_broken *brk, const char *path, alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!brk || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "broken and path must not be NULL");
    if (!e->br_valid || brk->n_targets < 0 || (uint64_t) brk->n_targets != e->br_targets || brk->n_pieces < 0 || (uint64_t) brk->n_pieces != e->br_pieces ||
        brk->n_columns != e->br_columns || brk->d_words != (const uint32_t *) e->br_words.p || brk->d_piece_off != (const uint32_t *) e->br_poff.p ||
        brk->d_len != (const int32_t *) e->br_len.p || brk->d_piece_target != (const int32_t *) e->br_ptarget.p || brk->d_piece_start != (const uint32_t *) e->br_pstart.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_break_placed_device call on this engine");
    if (e->br_longest + 96 > 0xFFFFFFFFull) return alga_fail(e, ALGA_ERR_CAPACITY, "a piece record of more than 2^32 bytes");
    HIP_TRY(e, hipSetDevice(e->device));
    const BrFasta f{brk->d_words, brk->d_piece_off, brk->d_len, brk->d_piece_target, brk->d_piece_start, (uint64_t) brk->n_pieces};
    return alga_text_records(e, f, launch_br_fasta_sizes, launch_br_fasta_write, path, info);
}
