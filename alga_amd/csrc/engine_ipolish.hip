// alga_amd/csrc/engine_ipolish.hip -- C ABI of the polish with the gapped reads (include/alga_amd.h: alga_polish_indels_device,
// alga_write_ipolished_fasta_device, alga_write_ipolish_events_tsv_device; kernels in ipolish_kernels.hip, the H voters' gather in polish_kernels.hip).
//
// Host side: the checks (the twin property, the polish's check of the H voters, k_ip_check of the G voters) run on a workspace and end in one
// read-back (the refusal flags, the voters, the insertion votes); only then is anything else touched, and the result is written into the set
// that is not the current one and swapped in at the very end, so a refused or failed call leaves an earlier result as it was.  Then: the H voters
// through the polish's keys -> sort -> vote kernels with this stage's buffers (their counts are what is kept), the G voters' cells added onto
// them, the span (difference array, one scan), the insertion votes sorted by (slot, key) in two stable passes of the 64-bit radix sort (its keys
// end at 50 bits, (slot, key) has 62) and the winner per slot, the decision per old column, the scans of the widths and of the events (one
// read-back: the new columns and the events, the arrays are allocated at their size), the new words, the events, the targets, the counters.
#include <hip/hip_runtime.h>

#include <chrono>

#include "engine_internal.h"
#include "correct_kernels.h"
#include "gfa_kernels.h"
#include "ipolish_kernels.h"
#include "polish_kernels.h"

using namespace alga;

namespace {

int check_params(alga_engine *e, const alga_ipolish_params *p) {
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish parameters must not be NULL");
    if (p->min_cover < 1) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: min_cover must be >= 1");
    if (p->min_percent < 1 || p->min_percent > 100) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: min_percent must be in [1, 100]");
    if (p->max_ins < 1 || p->max_ins > ALGA_IPOLISH_MAX_INS) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: max_ins must be in [1, 13]");
    if (p->flags & ~ALGA_IPOLISH_COUNTS) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: unknown flag");
    for (int32_t r : p->reserved) if (r) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: reserved must be 0");
    return ALGA_OK;
}

int ipolish_impl(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_gapped *gp, const alga_ipolish_params *p, hipStream_t s, alga_ipolished *out,
                 alga_ipolish_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t R = (uint64_t) pl->n_reads, T = (uint64_t) pl->n_targets, columns = pl->n_columns;
    const bool want_counts = (p->flags & ALGA_IPOLISH_COUNTS) != 0;
    int rc;
    AlgaEvents<4> evs;
    if ((rc = evs.create(e))) return rc;
    constexpr int N_CNT = IP_COUNTERS + PO_COUNTERS;
    if ((rc = alga_ensure(e, e->ip_cnt, N_CNT * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->ip_cnt.p, *pcnt = cnt + IP_COUNTERS, *hc = e->h_counters, *hp = hc + IP_COUNTERS;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, N_CNT * sizeof(unsigned long long), s));
    const PoReads prd{nodes->words, nodes->stride_words, nodes->len, R, pl->d_target, pl->d_pos, pl->d_state, (uint8_t) ALGA_PLACE_UNIQUE};
    const PoTargets ptg{pl->d_col_off, (uint32_t) T, columns, (const uint32_t *) e->pl_cols.p};
    const IpReads ird{nodes->words, nodes->stride_words, nodes->len, R, gp->d_target, gp->d_pos, gp->d_end, gp->d_state, gp->d_cigar_off, gp->d_cigar, gp->n_cigar};
    const IpTargets itg{pl->d_col_off, (uint32_t) T, columns, (const uint32_t *) e->pl_cols.p, (uint32_t) e->opt_ipolish_max_blocks};

    // the checks: nothing of the result is written before their verdict
    if (R) {
        const CrReads c{const_cast<uint32_t *>(nodes->words), nodes->stride_words, nodes->len, R, 1};
        launch_cr_twin(c, (uint32_t *) (cnt + IP_BAD_TWIN), s);
        if ((rc = alga_check_launch(e, "k_cr_twin"))) return rc;
    }
    launch_po_check(prd, ptg, pcnt, s);
    if ((rc = alga_check_launch(e, "k_po_check"))) return rc;
    launch_ip_check(ird, itg, p->max_ins, cnt, s);
    if ((rc = alga_check_launch(e, "k_ip_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, N_CNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[IP_BAD_TWIN]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: a row 2r is not the reverse complement of row 2r + 1, their lengths differ, or a length exceeds the stride");
    if (hp[PO_BAD] & PO_BAD_COLUMNS) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: n_columns is not the placement's col_off[n_targets]");
    if (hp[PO_BAD] & PO_BAD_LEN) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: a voting node has a length below 1 or above 16 * stride_words");
    if (hp[PO_BAD] & PO_BAD_PLACE) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: a voting node does not fit its placement: not the node set that was placed");
    if (hc[IP_BAD] & IP_BAD_RUNS) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: a gapped voter's script has no run, more than 31 runs or an unknown op");
    if (hc[IP_BAD] & IP_BAD_PLACE) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: a gapped voter does not lie inside its target");
    if (hc[IP_BAD] & IP_BAD_READ_LEN) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: a gapped voter's script does not have the read's length: not the node set that was placed");
    if (hc[IP_BAD] & IP_BAD_COL_LEN) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: a gapped voter's script does not have end - pos columns");
    const uint64_t voters_h = hp[PO_VOTERS], votes_h = hp[PO_VOTES], longest = hp[PO_MAX_LEN], voters_g = hc[IP_VOTERS_G], n_ins = hc[IP_INS_VOTES];
    alga_ipolish_info o{};
    o.columns = columns; o.voters_hamming = voters_h; o.voters_gapped = voters_g; o.votes = votes_h + hc[IP_VOTES_G]; o.del_votes = hc[IP_DEL_VOTES]; o.ins_votes = n_ins;
    o.ins_too_long = hc[IP_INS_LONG]; o.ins_edge = hc[IP_INS_EDGE]; o.shifted_runs = hc[IP_SHIFTED_RUNS]; o.shifted_bases = hc[IP_SHIFTED_BASES];

    // the workspaces, and the set that is not the current one
    const size_t n_words = (size_t) ((columns + 15) >> 4);
    for (int j = 0; j < 2; j++) {
        if ((rc = alga_ensure(e, e->ip_keys[j], (R + 4) * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->ip_vals[j], (R + 4) * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->ip_ikey[j], (n_ins + 2) * sizeof(unsigned long long)))) return rc;
        if ((rc = alga_ensure(e, e->ip_islot[j], (n_ins + 2) * sizeof(unsigned long long)))) return rc;
    }
    for (DevBuf *b : {&e->ip_marks, &e->ip_pop, &e->ip_pwords}) if ((rc = alga_ensure(e, *b, (n_words + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ip_ptstat, (2 * T + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->ip_counts4, (64 * n_words + 4) * sizeof(uint32_t)))) return rc;                     // 16 bytes per column, whole words
    for (DevBuf *b : {&e->ip_del, &e->ip_diff, &e->ip_scan, &e->ip_winkey, &e->ip_winvotes, &e->ip_insall, &e->ip_width, &e->ip_evn, &e->ip_evoff})
        if ((rc = alga_ensure(e, *b, (columns + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ip_code, columns + 16))) return rc;
    const size_t temp32 = rsort_u32_pairs_temp_bytes(R), temp64 = rsort_u64_pairs_temp_bytes(n_ins);
    if ((rc = alga_ensure(e, e->sort_temp, std::max(temp32, temp64)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(columns + 2)))) return rc;
    const int nxt = alga_other_set(e->ip_valid, e->ip_cur);
    alga_engine::IpolishSet &rs = e->ip_set[nxt];
    if ((rc = alga_ensure(e, rs.len, (T + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, rs.coloff, (T + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, rs.oldoff, (T + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, rs.begin, (T + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, rs.tstat, (4 * T + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, rs.newcol, (columns + 4) * sizeof(uint32_t)))) return rc;
    if (want_counts) {
        if ((rc = alga_ensure(e, rs.counts, (5 * columns + 4) * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, rs.span, (columns + 4) * sizeof(uint32_t)))) return rc;
    }
    uint32_t *counts4 = (uint32_t *) e->ip_counts4.p, *del = (uint32_t *) e->ip_del.p, *diff = (uint32_t *) e->ip_diff.p, *scan = (uint32_t *) e->ip_scan.p;
    uint32_t *win_key = (uint32_t *) e->ip_winkey.p, *win_votes = (uint32_t *) e->ip_winvotes.p, *ins_all = (uint32_t *) e->ip_insall.p;
    uint32_t *width = (uint32_t *) e->ip_width.p, *evn = (uint32_t *) e->ip_evn.p, *ev_off = (uint32_t *) e->ip_evoff.p, *new_col = (uint32_t *) rs.newcol.p;
    uint8_t *code = (uint8_t *) e->ip_code.p;
    unsigned long long *tstat = (unsigned long long *) rs.tstat.p, *ptstat = (unsigned long long *) e->ip_ptstat.p;
    unsigned long long *ikey[2] = {(unsigned long long *) e->ip_ikey[0].p, (unsigned long long *) e->ip_ikey[1].p};
    unsigned long long *islot[2] = {(unsigned long long *) e->ip_islot[0].p, (unsigned long long *) e->ip_islot[1].p};

    // the votes: the H voters by the polish's gather, the G voters' cells on top, the span
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    if (voters_h) {
        launch_po_keys(prd, ptg, (uint32_t *) e->ip_keys[0].p, (uint32_t *) e->ip_vals[0].p, s);
        if ((rc = alga_check_launch(e, "k_po_keys"))) return rc;
        HIP_TRY(e, rsort_u32_pairs(e->sort_temp.p, temp32, (const uint32_t *) e->ip_keys[0].p, (uint32_t *) e->ip_keys[1].p, (const uint32_t *) e->ip_vals[0].p,
                                   (uint32_t *) e->ip_vals[1].p, R, 0, s));
    }
    HIP_TRY(e, hipMemsetAsync(ptstat, 0, (2 * T + 1) * sizeof(unsigned long long), s));
    const PoVote pv{(const uint32_t *) e->ip_keys[1].p, (const uint32_t *) e->ip_vals[1].p, (uint32_t) voters_h, (uint32_t) longest, p->min_cover, p->min_percent,
                    (uint32_t *) e->ip_pwords.p, (uint32_t *) e->ip_marks.p, (uint32_t *) e->ip_pop.p, counts4, ptstat, ptstat + T};
    // the polish's vote kernels store the four counts of every column they decide; that they decide every column is their business, not a
    // contract of this stage: the counts start at zero
    HIP_TRY(e, hipMemsetAsync(counts4, 0, (64 * n_words + 4) * sizeof(uint32_t), s));
    launch_po_vote(prd, ptg, pv, pcnt, s);
    if ((rc = alga_check_launch(e, "k_po_vote"))) return rc;
    launch_po_vote_wide(prd, ptg, pv, pcnt, s);
    if ((rc = alga_check_launch(e, "k_po_vote_wide"))) return rc;
    for (uint32_t *a : {del, diff, scan, win_key, win_votes, ins_all}) HIP_TRY(e, hipMemsetAsync(a, 0, (columns + 4) * sizeof(uint32_t), s));
    if (voters_g) {
        launch_ip_vote_gapped(ird, itg, p->max_ins, counts4, del, ikey[0], islot[0], ins_all, cnt, s);
        if ((rc = alga_check_launch(e, "k_ip_vote_gapped"))) return rc;
    }
    if (voters_h + voters_g) {
        launch_ip_span(ird, itg, pl->d_target, pl->d_pos, pl->d_state, diff, s);
        if ((rc = alga_check_launch(e, "k_ip_span"))) return rc;
        // exclusive scan over columns + 1 differences: entry c + 1 is span[c]
        launch_exclusive_scan(diff, columns + 1, scan, (uint64_t *) e->scan_scratch.p, s);
        if ((rc = alga_check_launch(e, "scan(span)"))) return rc;
    }
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    // the insertion votes: by key, then (stable) by slot; the winner of every slot
    if (n_ins) {
        HIP_TRY(e, rsort_u64_pairs(e->sort_temp.p, temp64, ikey[0], ikey[1], islot[0], islot[1], n_ins, 30, s));
        HIP_TRY(e, rsort_u64_pairs(e->sort_temp.p, temp64, islot[1], islot[0], ikey[1], ikey[0], n_ins, 32, s));
        launch_ip_ins_pick(islot[0], ikey[0], n_ins, win_key, win_votes, ins_all, itg.max_blocks, s);
        if ((rc = alga_check_launch(e, "k_ip_ins_pick"))) return rc;
    }
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));

    // the decision, the widths and the events, their scans
    HIP_TRY(e, hipMemsetAsync(tstat, 0, (4 * T + 1) * sizeof(unsigned long long), s));
    HIP_TRY(e, hipMemcpyAsync(rs.oldoff.p, pl->d_col_off, (T + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    const IpDecide dec{counts4, del, scan, win_key, win_votes, ins_all, p->min_cover, p->min_percent, width, evn, code, want_counts ? (uint32_t *) rs.counts.p : nullptr,
                       want_counts ? (uint32_t *) rs.span.p : nullptr, tstat, tstat + T, tstat + 2 * T, tstat + 3 * T};
    launch_ip_decide(itg, dec, cnt, s);
    if ((rc = alga_check_launch(e, "k_ip_decide"))) return rc;
    uint64_t totals[2] = {0, 0};                                      // the new columns, the events: the scans' 64-bit totals
    uint64_t *scr = (uint64_t *) e->scan_scratch.p;
    launch_exclusive_scan(width, columns + 1, new_col, scr, s);
    if ((rc = alga_check_launch(e, "scan(widths)"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(&totals[0], scr + scan_total_index(columns + 1), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    launch_exclusive_scan(evn, columns + 1, ev_off, scr, s);
    if ((rc = alga_check_launch(e, "scan(events)"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(&totals[1], scr + scan_total_index(columns + 1), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t NC = totals[0], n_events = totals[1];
    if (NC > 0xFFFFFFFEull) return alga_fail(e, ALGA_ERR_CAPACITY, "indel polish: the new targets hold more than 2^32 - 2 bases");
    if (n_events > 0xFFFFFFFEull) return alga_fail(e, ALGA_ERR_CAPACITY, "indel polish: more than 2^32 - 2 events");
    const size_t new_words = (size_t) ((NC + 15) >> 4) + 2;
    if ((rc = alga_ensure(e, rs.words, new_words * sizeof(uint32_t)))) return rc;
    for (DevBuf *b : {&rs.evcol, &rs.evbases, &rs.evvotes, &rs.evcover}) if ((rc = alga_ensure(e, *b, (n_events + 4) * sizeof(uint32_t)))) return rc;
    for (DevBuf *b : {&rs.evkind, &rs.evlen}) if ((rc = alga_ensure(e, *b, n_events + 16))) return rc;

    const IpBuild bld{new_col, ev_off, code, counts4, del, scan, win_key, win_votes, NC};
    launch_ip_words(itg, bld, (uint32_t *) rs.words.p, s);
    if ((rc = alga_check_launch(e, "k_ip_words"))) return rc;
    if (n_events) {
        const IpEvents ev{(uint32_t *) rs.evcol.p, (uint8_t *) rs.evkind.p, (uint8_t *) rs.evlen.p, (uint32_t *) rs.evbases.p, (uint32_t *) rs.evvotes.p, (uint32_t *) rs.evcover.p};
        launch_ip_events(itg, bld, ev, s);
        if ((rc = alga_check_launch(e, "k_ip_events"))) return rc;
    }
    launch_ip_targets(itg, new_col, (uint32_t *) rs.coloff.p, (int32_t *) rs.len.p, (unsigned long long *) rs.begin.p, cnt, s);
    if ((rc = alga_check_launch(e, "k_ip_targets"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[3], s));
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, IP_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[IP_LONGEST] > 0x7FFFFFFFull) return alga_fail(e, ALGA_ERR_CAPACITY, "indel polish: a new target is longer than 2^31 - 1");

    e->ip_cur = nxt; e->ip_valid = true; e->ip_targets = T; e->ip_columns = NC; e->ip_columns_before = columns; e->ip_events = n_events; e->ip_longest = hc[IP_LONGEST];
    out->n_targets = (int64_t) T; out->n_columns_before = columns; out->n_columns = NC; out->n_events = n_events;
    out->d_len = (const int32_t *) rs.len.p; out->d_col_off = (const uint32_t *) rs.coloff.p; out->d_begin = (const uint64_t *) rs.begin.p;
    out->d_words = (const uint32_t *) rs.words.p; out->d_new_col = new_col;
    out->d_ev_col = (const uint32_t *) rs.evcol.p; out->d_ev_kind = (const uint8_t *) rs.evkind.p; out->d_ev_len = (const uint8_t *) rs.evlen.p;
    out->d_ev_bases = (const uint32_t *) rs.evbases.p; out->d_ev_votes = (const uint32_t *) rs.evvotes.p; out->d_ev_cover = (const uint32_t *) rs.evcover.p;
    out->d_t_subs = (const uint64_t *) tstat; out->d_t_dels = (const uint64_t *) (tstat + T); out->d_t_ins_bases = (const uint64_t *) (tstat + 2 * T);
    out->d_t_ambiguous = (const uint64_t *) (tstat + 3 * T);
    out->d_counts = want_counts ? (const uint32_t *) rs.counts.p : nullptr; out->d_span = want_counts ? (const uint32_t *) rs.span.p : nullptr;
    if (info) {
        o.voted_columns = hc[IP_VOTED]; o.substituted = hc[IP_SUBST]; o.deleted = hc[IP_DELETED]; o.inserted_slots = hc[IP_INS_SLOTS]; o.inserted_bases = hc[IP_INS_BASES];
        o.ambiguous_columns = hc[IP_AMB_COLS]; o.ambiguous_slots = hc[IP_AMB_SLOTS]; o.columns_after = NC; o.max_cover = hc[IP_MAX_COVER];
        if ((rc = evs.ms(e, 0, 1, &o.ms_votes))) return rc;
        if ((rc = evs.ms(e, 1, 2, &o.ms_inserts))) return rc;
        if ((rc = evs.ms(e, 2, 3, &o.ms_build))) return rc;
        o.ms_total = alga_ms_since(t0);
        *info = o;
    }
    return ALGA_OK;
}

// `ipol` names the buffers and sizes of the result the engine holds
int ipolished_is_current(alga_engine *e, const alga_ipolished *ipol) {
    const alga_engine::IpolishSet &rs = e->ip_set[e->ip_cur];
    if (!e->ip_valid || ipol->n_targets < 0 || (uint64_t) ipol->n_targets != e->ip_targets || ipol->n_columns != e->ip_columns ||
        ipol->n_columns_before != e->ip_columns_before || ipol->n_events != e->ip_events || ipol->d_len != (const int32_t *) rs.len.p ||
        ipol->d_col_off != (const uint32_t *) rs.coloff.p || ipol->d_words != (const uint32_t *) rs.words.p || ipol->d_ev_col != (const uint32_t *) rs.evcol.p ||
        ipol->d_ev_kind != (const uint8_t *) rs.evkind.p || ipol->d_ev_len != (const uint8_t *) rs.evlen.p || ipol->d_ev_bases != (const uint32_t *) rs.evbases.p ||
        ipol->d_ev_votes != (const uint32_t *) rs.evvotes.p || ipol->d_ev_cover != (const uint32_t *) rs.evcover.p || ipol->d_begin != (const uint64_t *) rs.begin.p ||
        ipol->d_new_col != (const uint32_t *) rs.newcol.p || ipol->d_t_subs != (const uint64_t *) rs.tstat.p ||
        ipol->d_t_dels != (const uint64_t *) rs.tstat.p + e->ip_targets || ipol->d_t_ins_bases != (const uint64_t *) rs.tstat.p + 2 * e->ip_targets ||
        ipol->d_t_ambiguous != (const uint64_t *) rs.tstat.p + 3 * e->ip_targets)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_polish_indels_device call on this engine");
    return ALGA_OK;
}

}  // namespace

extern "C" void alga_ipolish_default_params(alga_ipolish_params *p) {
    if (!p) return;
    *p = alga_ipolish_params{};
    p->min_cover = 3; p->min_percent = 60; p->max_ins = 6; p->flags = 0;
}

extern "C" int alga_polish_indels_device(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_gapped *gp, const alga_ipolish_params *p,
                                         void *hip_stream, alga_ipolished *out, alga_ipolish_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if (!nodes || !pl || !gp || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes, placements, gapped placements and out must not be NULL");
    if ((rc = alga_check_twin_nodes(e, nodes, true))) return rc;
    if (!alga_placement_is_current(e, pl)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last placement call on this engine");
    if (!alga_gapped_is_current(e, gp)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_place_gapped_device call on this placement");
    if ((int64_t) (nodes->n / 2) != pl->n_reads) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "indel polish: the node set does not have the placement's reads (n / 2 != n_reads)");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return ipolish_impl(e, nodes, pl, gp, p, call.s, out, info);
}

extern "C" int alga_write_ipolished_fasta_device(alga_engine *e, const alga_ipolished *ipol, const char *path, alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!ipol || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "the indel polish result and path must not be NULL");
    int rc;
    if ((rc = ipolished_is_current(e, ipol))) return rc;
    if (e->ip_longest + 128 > 0xFFFFFFFFull) return alga_fail(e, ALGA_ERR_CAPACITY, "a contig record of more than 2^32 bytes");
    HIP_TRY(e, hipSetDevice(e->device));
    const IpFasta f{ipol->d_words, ipol->d_col_off, ipol->d_len, (const unsigned long long *) ipol->d_t_subs, (const unsigned long long *) ipol->d_t_ins_bases,
                    (const unsigned long long *) ipol->d_t_dels, (uint64_t) ipol->n_targets};
    return alga_text_records(e, f, launch_ip_fasta_sizes, launch_ip_fasta_write, path, info);
}

extern "C" int alga_write_ipolish_events_tsv_device(alga_engine *e, const alga_ipolished *ipol, const char *path, alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!ipol || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "the indel polish result and path must not be NULL");
    int rc;
    if ((rc = ipolished_is_current(e, ipol))) return rc;
    HIP_TRY(e, hipSetDevice(e->device));
    const IpTsv f{(const uint32_t *) e->ip_set[e->ip_cur].oldoff.p,    // the result's own copy of the col_off that was polished: `pos`
                  (uint32_t) e->ip_targets, ipol->d_ev_col, ipol->d_ev_kind, ipol->d_ev_len, ipol->d_ev_bases, ipol->d_ev_votes,
                  ipol->d_ev_cover, ipol->n_events};
    AlgaTextJob job;
    job.items = f.n;
    job.sizes = [f](uint32_t *o, unsigned long long *counters, hipStream_t s) { launch_ip_tsv_sizes(f, o, counters, s); };
    job.format = [f](const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) { launch_ip_tsv_write(f, off, i0, i1, buf, s); };
    job.kind = "TSV";
    return alga_text_job_run(e, job, path, info);
}
