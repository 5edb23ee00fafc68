// alga_amd/csrc/engine_final.hip -- C ABI of the final contig set (include/alga_amd.h: alga_contig_trim_device, alga_final_contigs_device,
// alga_write_final_fasta_device; kernels in final_kernels.hip).
//
// Host side of the filter: the rank sort, the verdicts that need no order, then one loop over the rounds with one count read back per round; the
// ids by a scan of the accepted flags in rank order.  Of the trim: the device's verdict on the lengths (one read-back, with the row stride), the
// capped rows and their reverse complements, one build, k_trim_left.  The FASTA goes through the chunk pipeline of engine_gfa.hip.
#include <hip/hip_runtime.h>

#include <chrono>

#include "engine_internal.h"
#include "final_kernels.h"
#include "gfa_kernels.h"
#include "simplify_kernels.h"

using namespace alga;

namespace {

// max_capped_len: the longest capped length if the caller knows it (the final call's number kernel), -1: ask the device (and check the lengths)
int trim_impl(alga_engine *e, const uint32_t *d_words, const unsigned long long *d_begin, const int32_t *d_len, int32_t n, int32_t threshold,
              int64_t max_capped_len, hipStream_t s, int32_t *d_trim_left, uint64_t *edges_out) {
    int rc;
    const size_t M = (size_t) n;
    if (max_capped_len < 0) {
        if ((rc = alga_ensure(e, e->fc_cnt, FC_COUNTERS * sizeof(unsigned long long)))) return rc;
        unsigned long long *cnt = (unsigned long long *) e->fc_cnt.p;
        HIP_TRY(e, hipMemsetAsync(cnt, 0, FC_COUNTERS * sizeof(unsigned long long), s));
        launch_fc_len_check(d_len, M, cnt, s);
        if ((rc = alga_check_launch(e, "k_fc_len_check"))) return rc;
        HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, FC_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        if (e->h_counters[FC_FLAGS] & FC_BAD_LEN) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "negative sequence length");
        max_capped_len = (int64_t) e->h_counters[FC_MAX_LEN];
    }
    const int32_t stride = (int32_t) std::max<int64_t>(1, (max_capped_len + 15) / 16);        // <= 63 words
    const size_t row_bytes = (size_t) stride * sizeof(uint32_t);
    // the input is valid: from here on the engine's build state is rewritten.  Nodes as src/main.cpp:636-645 numbers them: the sequences
    // 0 .. M-1, then their reverse complements M .. 2M-1
    alga_forget_node_set(e);
    if ((rc = alga_ensure(e, e->fc_rows, 2 * M * row_bytes))) return rc;
    if ((rc = alga_ensure(e, e->fc_rlen, 2 * M * sizeof(int32_t)))) return rc;
    launch_fc_gather(d_words, d_begin, d_len, M, stride, (uint32_t *) e->fc_rows.p, (int32_t *) e->fc_rlen.p, s);
    if ((rc = alga_check_launch(e, "k_fc_gather"))) return rc;
    launch_revcomp_rows((uint32_t *) e->fc_rows.p, stride, (int32_t *) e->fc_rlen.p, n, s);
    if ((rc = alga_check_launch(e, "k_revcomp_rows"))) return rc;
    alga_nodes nd{(const uint32_t *) e->fc_rows.p, stride, (const int32_t *) e->fc_rlen.p, 2 * n, nullptr, nullptr};
    alga_prefsuf_params p;
    alga_prefsuf_default_params(&p);
    p.min_overlap = threshold;                             // src/main.cpp:651-653
    p.rsoe_min_overlap = threshold;
    const alga_edge *d_edges = nullptr;
    uint64_t m = 0;
    if ((rc = alga_prefsuf_build_device(e, &nd, &p, (void *) s, &d_edges, &m))) return rc;
    alga_forget_node_set(e);                               // (the rows are rewritten by the next call at the same address)
    HIP_TRY(e, hipMemsetAsync(d_trim_left, 0, M * sizeof(int32_t), s));
    launch_trim_left((const alga_edge_dev *) d_edges, m, (const int32_t *) e->fc_rlen.p, n, d_trim_left, s);
    if ((rc = alga_check_launch(e, "k_trim_left"))) return rc;
    if (edges_out) *edges_out = m;
    return ALGA_OK;
}

bool current_results(const alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, const char **why) {
    if (!e->ut_valid || u->d_len != (const int32_t *) e->ut_ulen.p || (uint64_t) u->n_pairs != e->ut_n_pairs || u->d_words != (const uint32_t *) e->ut_words.p ||
        u->d_path_node != (const int32_t *) e->ut_path_node.p || u->d_path_off != (const uint64_t *) e->ut_path_off.p ||
        u->d_word_off != (const uint64_t *) e->ut_word_off.p) {
        *why = "not the result of the last alga_unitigs_device call on this engine";
        return false;
    }
    if (!e->cs_valid || cons->n_pairs != u->n_pairs || cons->d_words != (const uint32_t *) e->cs_words.p || cons->d_len != (const int32_t *) e->cs_len.p ||
        cons->d_trim_left != (const int32_t *) e->cs_trim.p) {
        *why = "not the result of the last alga_unitig_consensus_device call on this engine";
        return false;
    }
    return true;
}

int final_impl(alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, int32_t min_length, int32_t percent, int32_t trim_threshold, hipStream_t s,
               alga_final_contigs *out, alga_final_info *info) {
    const uint32_t P = (uint32_t) u->n_pairs;
    const size_t reads = (size_t) e->ut_n_nodes / 2;
    int rc;
    AlgaEvents<3> evs;
    if ((rc = evs.create(e))) return rc;
    e->fc_valid = false;
    if ((rc = alga_ensure(e, e->fc_cnt, FC_COUNTERS * sizeof(unsigned long long)))) return rc;
    for (DevBuf *b : {&e->fc_keys[0], &e->fc_keys[1], &e->fc_vals, &e->fc_list[0], &e->fc_list[1], &e->fc_ids, &e->fc_flag})
        if ((rc = alga_ensure(e, *b, (size_t) (P + 8) * sizeof(uint32_t)))) return rc;                 // (the sort reads its keys 16 bytes at a time)
    for (DevBuf *b : {&e->fc_rank, &e->fc_id, &e->fc_new, &e->fc_trim, &e->fc_begin, &e->fc_len, &e->fc_order, &e->fc_wlen, &e->fc_tid})
        if ((rc = alga_ensure(e, *b, (size_t) (P + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->fc_verdict, (size_t) P + 1))) return rc;
    if ((rc = alga_ensure(e, e->fc_wbegin, (size_t) (P + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->fc_first, (reads + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->fc_min, (reads + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->sort_temp, rsort_u32_pairs_temp_bytes(P)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes((uint64_t) P + 1)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->fc_cnt.p;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, FC_COUNTERS * sizeof(unsigned long long), s));
    HIP_TRY(e, hipMemsetAsync(e->fc_first.p, 0xFF, (reads + 1) * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(e->fc_min.p, 0, (reads + 1) * sizeof(unsigned long long), s));
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    // the rank order: a stable sort of (2^31 - 1 - length, pair)
    launch_fc_rank_keys(cons->d_len, P, (uint32_t *) e->fc_keys[0].p, s);
    if ((rc = alga_check_launch(e, "k_fc_rank_keys"))) return rc;
    HIP_TRY(e, rsort_u32_pairs(e->sort_temp.p, e->sort_temp.cap, (const uint32_t *) e->fc_keys[0].p, (uint32_t *) e->fc_keys[1].p, nullptr, (uint32_t *) e->fc_vals.p, P,
                               0, s));
    FcCfg c{u->d_path_node, (const unsigned long long *) u->d_path_off, (const unsigned long long *) u->d_word_off, cons->d_len, cons->d_trim_left, P, min_length,
            percent, (const uint32_t *) e->fc_vals.p, (uint8_t *) e->fc_verdict.p, (int32_t *) e->fc_rank.p, (int32_t *) e->fc_id.p, (int32_t *) e->fc_new.p,
            (int32_t *) e->fc_trim.p, (int32_t *) e->fc_begin.p, (int32_t *) e->fc_len.p, (int32_t *) e->fc_order.p, (uint32_t *) e->fc_first.p,
            (unsigned long long *) e->fc_min.p, e->ut_is_extended ? (const unsigned long long *) e->ex_seam_off.p : nullptr,
            e->ut_is_extended ? (const int32_t *) e->ex_seam_entry.p : nullptr};
    launch_fc_init(c, (uint32_t *) e->fc_list[0].p, cnt, s);
    if ((rc = alga_check_launch(e, "k_fc_init"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(&e->h_counters[0], cnt + FC_UNDECIDED, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    uint64_t undecided = e->h_counters[0], rounds = 0;
    int cur = 0;
    while (undecided) {                                    // the undecided pair of the smallest rank is decidable: every round decides one at least
        rounds++;
        HIP_TRY(e, hipMemsetAsync(cnt + FC_UNDECIDED, 0, sizeof(unsigned long long), s));
        launch_fc_round(c, (const uint32_t *) e->fc_list[cur].p, (uint32_t) undecided, (uint32_t) rounds, (uint32_t *) e->fc_list[cur ^ 1].p, cnt + FC_UNDECIDED, s);
        if ((rc = alga_check_launch(e, "k_fc_round_decide"))) return rc;
        HIP_TRY(e, hipMemcpyAsync(&e->h_counters[0], cnt + FC_UNDECIDED, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        if (e->h_counters[0] >= undecided) return alga_fail(e, ALGA_ERR_HIP, "the contig filter made no progress in a round");
        undecided = e->h_counters[0];
        cur ^= 1;
    }
    // ids, new reads, the windows of the accepted pairs in id order
    launch_fc_accept_flags(c, (uint32_t *) e->fc_flag.p, s);
    launch_exclusive_scan((const uint32_t *) e->fc_flag.p, (uint64_t) P + 1, (uint32_t *) e->fc_ids.p, (uint64_t *) e->scan_scratch.p, s);
    launch_fc_number(c, (const uint32_t *) e->fc_ids.p, (unsigned long long *) e->fc_wbegin.p, (int32_t *) e->fc_wlen.p, cnt, s);
    if ((rc = alga_check_launch(e, "k_fc_number"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, FC_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t n_short = e->h_counters[FC_SHORT], n_rej = e->h_counters[FC_REJECTED], n_acc = e->h_counters[FC_ACCEPTED];
    const int64_t max_capped = (int64_t) e->h_counters[FC_MAX_LEN];
    uint64_t away = 0, trim_edges = 0;
    if (trim_threshold > 0 && n_acc) {
        if ((rc = trim_impl(e, cons->d_words, (const unsigned long long *) e->fc_wbegin.p, (const int32_t *) e->fc_wlen.p, (int32_t) n_acc, trim_threshold, max_capped, s,
                            (int32_t *) e->fc_tid.p, &trim_edges))) return rc;
        launch_fc_apply_trim(c, (const int32_t *) e->fc_tid.p, (uint32_t) n_acc, cnt, s);
        if ((rc = alga_check_launch(e, "k_fc_apply_trim"))) return rc;
        HIP_TRY(e, hipMemcpyAsync(&e->h_counters[0], cnt + FC_TRIMMED_AWAY, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (trim_threshold > 0 && n_acc) away = e->h_counters[0];

    e->fc_valid = true; e->fc_n_accepted = n_acc; e->fc_epoch++;
    out->n_pairs = u->n_pairs; out->n_accepted = (int32_t) n_acc; out->n_written = (int32_t) (n_acc - away); out->reserved = 0;
    out->d_verdict = (const uint8_t *) e->fc_verdict.p; out->d_rank = c.rank; out->d_id = c.id; out->d_new_reads = c.new_reads; out->d_trim_left = c.trim_left;
    out->d_begin = c.begin; out->d_len = c.len; out->d_order = c.order;
    if (info) {
        info->pairs = P; info->n_short = n_short; info->rejected = n_rej; info->accepted = n_acc - away; info->trimmed_away = away;
        info->filter_rounds = rounds; info->trim_edges = trim_edges;
        if ((rc = evs.ms(e, 0, 1, &info->ms_filter))) return rc;
        if ((rc = evs.ms(e, 1, 2, &info->ms_trim))) return rc;
    }
    return ALGA_OK;
}

}  // namespace

bool alga_final_is_current(const alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, const alga_final_contigs *fin, const char **why) {
    if (!current_results(e, u, cons, why)) return false;
    if (!e->fc_valid || fin->n_pairs != u->n_pairs || (uint64_t) fin->n_accepted != e->fc_n_accepted || fin->d_verdict != (const uint8_t *) e->fc_verdict.p ||
        fin->d_order != (const int32_t *) e->fc_order.p || fin->d_begin != (const int32_t *) e->fc_begin.p || fin->d_len != (const int32_t *) e->fc_len.p) {
        *why = "not the result of the last alga_final_contigs_device call on this engine";
        return false;
    }
    return true;
}

extern "C" int alga_contig_trim_device(alga_engine *e, const uint32_t *d_words, const uint64_t *d_begin, const int32_t *d_len, int32_t n, int32_t threshold,
                                       void *hip_stream, int32_t *d_trim_left, uint64_t *edges_out) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (edges_out) *edges_out = 0;
    if (n < 0 || (n && (!d_words || !d_begin || !d_len || !d_trim_left))) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad sequence arrays");
    if (threshold < 1 || threshold > 501) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "threshold must be in [1, 501]");
    if (n == 0) return ALGA_OK;
    if (n > 0x3FFFFFFF) return alga_fail(e, ALGA_ERR_CAPACITY, "too many sequences");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    const int rc = trim_impl(e, d_words, (const unsigned long long *) d_begin, d_len, n, threshold, -1, s, d_trim_left, edges_out);
    (void) hipStreamSynchronize(s);
    return rc;
}

extern "C" int alga_final_contigs_device(alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, int32_t min_length, int32_t new_reads_percent,
                                         int32_t trim_threshold, int32_t flags, void *hip_stream, alga_final_contigs *out, alga_final_info *info) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    const auto t0 = std::chrono::steady_clock::now();
    if (info) *info = alga_final_info{};
    if (!u || !cons || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unitigs, consensus and out must not be NULL");
    if (flags) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unknown final-contigs flag");
    if (min_length < 0) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "min_length must not be negative");
    if (new_reads_percent < 0 || new_reads_percent > 100) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "new_reads_percent must be in [0, 100]");
    if (trim_threshold < 0 || trim_threshold > 501) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "trim_threshold must be 0 or in [1, 501]");
    const char *why = nullptr;
    if (!current_results(e, u, cons, &why)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, why);
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    const int rc = final_impl(e, u, cons, min_length, new_reads_percent, trim_threshold, s, out, info);
    if (rc != ALGA_OK) { (void) hipStreamSynchronize(s); return rc; }
    if (info) info->ms_total = alga_ms_since(t0);
    return ALGA_OK;
}

extern "C" int alga_write_final_fasta_device(alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, const alga_final_contigs *fin, const char *path,
                                             alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!u || !cons || !fin || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unitigs, consensus, final contigs and path must not be NULL");
    const char *why = nullptr;
    if (!alga_final_is_current(e, u, cons, fin, &why)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, why);
    HIP_TRY(e, hipSetDevice(e->device));
    const FcFasta f{cons->d_words, (const unsigned long long *) u->d_word_off, fin->d_verdict, fin->d_order, fin->d_begin, fin->d_len, (uint64_t) fin->n_accepted};
    return alga_text_records(e, f, launch_fc_fasta_sizes, launch_fc_fasta_write, path, info);
}
