// alga_amd/csrc/engine_extend.hip -- C ABI of the extension of contigs by paired connections (include/alga_amd.h: alga_extend_contigs_device,
// alga_extend_seams_get; kernels in extend_kernels.hip).
//
// Host side: the order of the stages and the counts that size the next one.  The list ranking with its ruling set and the cycle cut are the
// unitig call's (engine_unitig.hip: alga_ut_rank), run twice over the oriented contig ids -- once with the weights (the bases before a contig on
// its path), once with the entry counts (the path entries before it); the sequences are k_ut_sequence, the edges go through the engine's edge sort.
// The new result is built in buffers of its own while the contig result is read, and the two sets of buffers change places at the very end: a
// refusal or an error leaves the contig result as it was.
#include <hip/hip_runtime.h>

#include <chrono>
#include <utility>

#include "engine_internal.h"
#include "extend_kernels.h"
#include "gfa_kernels.h"
#include "simplify_kernels.h"
#include "unitig_kernels.h"

using namespace alga;

namespace {

int read_u32(alga_engine *e, const void *d_src, hipStream_t s, uint64_t *out) {
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, d_src, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    *out = *(const uint32_t *) e->h_counters;
    return ALGA_OK;
}

bool current_contigs(const alga_engine *e, const alga_unitigs *u) {
    return e->ut_valid && u->d_len == (const int32_t *) e->ut_ulen.p && (uint64_t) u->n_pairs == e->ut_n_pairs && u->n_edges == e->ut_n_edges &&
           u->d_words == (const uint32_t *) e->ut_words.p && u->d_path_node == (const int32_t *) e->ut_path_node.p &&
           u->d_path_pos == (const int32_t *) e->ut_path_pos.p && u->d_path_off == (const uint64_t *) e->ut_path_off.p &&
           u->d_word_off == (const uint64_t *) e->ut_word_off.p && u->d_edges == (const alga_edge *) e->ut_edges.p;
}

int extend_impl(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const alga_unitigs *u, int32_t min_chain_weight, int32_t min_connections,
                int32_t max_insert, hipStream_t s, alga_unitigs *out, alga_extend_info *info) {
    const int32_t n = nodes->n;
    const uint64_t P = (uint64_t) u->n_pairs, n2 = 2 * P, mu_in = u->n_edges;
    const size_t N2 = (size_t) n2;
    int rc;
    AlgaEvents<6> evs;
    if ((rc = evs.create(e))) return rc;
    const size_t n_ucnt = UT_COUNTERS + ALGA_UT_MAX_ROUNDS;
    if ((rc = alga_ensure(e, e->ut_cnt, n_ucnt * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->ex_cnt, EX_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *ucnt = (unsigned long long *) e->ut_cnt.p, *cnt = (unsigned long long *) e->ex_cnt.p;
    HIP_TRY(e, hipMemsetAsync(ucnt, 0, n_ucnt * sizeof(unsigned long long), s));
    HIP_TRY(e, hipMemsetAsync(cnt, 0, EX_COUNTERS * sizeof(unsigned long long), s));
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    // ---- step 0: the device's verdict on pair_off
    launch_ex_check(d_pair_off, n, cnt, s);
    if ((rc = alga_check_launch(e, "k_ex_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters + 1, u->d_path_off + P, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t entries_in = e->h_counters[1];
    if (const unsigned long long bad = e->h_counters[EX_FLAGS]) {
        const char *why = (bad & EX_BAD_VALUE) ? "pair_off above 2" : (bad & EX_BAD_TWIN) ? "pair_off[v] != pair_off[v ^ 1]"
                                                                                          : "the mate of a paired read is out of range or does not point back";
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, why);
    }
    // the input is valid; the contig result and its consensus stay as they are until the new result is complete
    for (DevBuf *b : {&e->ex_w, &e->ex_kcnt, &e->ex_dlink, &e->ex_sole, &e->ex_xhead, &e->ex_xbase, &e->ex_xrank, &e->ex_uid, &e->ut_nxt, &e->ut_prv,
                      &e->ut_tail})
        if ((rc = alga_ensure(e, *b, (N2 + 1) * sizeof(int32_t)))) return rc;
    for (DevBuf *b : {&e->ex_rowptr, &e->ex_outcnt, &e->ut_win, &e->ut_pair, &e->ct_deg, &e->ct_epos})
        if ((rc = alga_ensure(e, *b, (N2 + 2) * sizeof(uint32_t)))) return rc;
    for (int k = 0; k < 2; k++) if ((rc = alga_ensure(e, e->ut_rank[k], (N2 + 1) * sizeof(UtRank)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(n2 + 1)))) return rc;
    uint32_t *rowptr = (uint32_t *) e->ex_rowptr.p, *outcnt = (uint32_t *) e->ex_outcnt.p;
    int32_t *w = (int32_t *) e->ex_w.p, *kcnt = (int32_t *) e->ex_kcnt.p, *dlink = (int32_t *) e->ex_dlink.p, *sole = (int32_t *) e->ex_sole.p;
    int32_t *xhead = (int32_t *) e->ex_xhead.p, *xbase = (int32_t *) e->ex_xbase.p, *xrank = (int32_t *) e->ex_xrank.p, *uid = (int32_t *) e->ex_uid.p;
    int32_t *nxt = (int32_t *) e->ut_nxt.p, *prv = (int32_t *) e->ut_prv.p, *tail = (int32_t *) e->ut_tail.p;
    launch_edge_rowptr((const alga_edge_dev *) u->d_edges, mu_in, (int32_t) n2, rowptr, s);
    if ((rc = alga_check_launch(e, "k_edge_rowptr"))) return rc;
    const ExIn in{nodes->len, d_pair_off, n, u->d_path_node, u->d_path_pos, (const unsigned long long *) u->d_path_off, u->d_len, (uint32_t) P,
                  (const alga_edge_dev *) u->d_edges, rowptr};

    // ---- steps 1-4: weights, the counts, L*
    launch_ex_weights(in, w, kcnt, s);
    launch_ex_count(in, w, min_chain_weight, min_connections, max_insert, dlink, cnt, s);
    if ((rc = alga_check_launch(e, "k_ex_count"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    // ---- step 5: joinable links, paths by list ranking (bases, then entries), cycles
    launch_ex_outlinks(in, dlink, outcnt, sole, cnt, s);
    launch_ex_next(outcnt, sole, (uint32_t) n2, nxt, cnt, s);
    launch_ut_prev(nxt, (int32_t) n2, prv, s);
    if ((rc = alga_check_launch(e, "k_ex_next"))) return rc;
    const int32_t *len2 = (const int32_t *) e->ut_ulen2.p;           // (positive for every oriented contig: all of them are ranked)
    int cur = 0, rounds = 0;
    if ((rc = alga_ut_rank(e, len2, (int32_t) n2, nxt, w, prv, ucnt, nullptr, cur, rounds, s))) return rc;
    launch_ex_save((const UtRank *) e->ut_rank[cur].p, (uint32_t) n2, xhead, xbase, xrank, s);
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, ucnt + UT_CYCLES, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t cycles = e->h_counters[0];
    HIP_TRY(e, hipMemsetAsync(ucnt, 0, n_ucnt * sizeof(unsigned long long), s));
    int rounds2 = 0;
    if ((rc = alga_ut_rank(e, len2, (int32_t) n2, nxt, kcnt, prv, ucnt, nullptr, cur, rounds2, s))) return rc;
    const UtRank *r2 = (const UtRank *) e->ut_rank[cur].p;
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));

    // ---- numbering, sizes, layout, seam list
    uint32_t *win = (uint32_t *) e->ut_win.p, *pair_of = (uint32_t *) e->ut_pair.p;
    launch_ut_tails(r2, len2, nxt, (int32_t) n2, tail, s);
    launch_ex_winners(prv, tail, (uint32_t) n2, win, s);
    if ((rc = alga_check_launch(e, "k_ex_winners"))) return rc;
    launch_exclusive_scan(win, n2, pair_of, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(winners)"))) return rc;
    uint64_t Pn = 0;
    if ((rc = read_u32(e, pair_of + n2, s, &Pn))) return rc;
    for (DevBuf *b : {&e->ex_pcnt, &e->ex_uwords, &e->ex_scnt})
        if ((rc = alga_ensure(e, *b, (size_t) (Pn + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ex_ulen, (size_t) (Pn + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ex_ulen2, (size_t) (2 * Pn + 2) * sizeof(int32_t)))) return rc;
    for (DevBuf *b : {&e->ex_path_off, &e->ex_word_off, &e->ex_seam_off})
        if ((rc = alga_ensure(e, *b, (size_t) (Pn + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->ut_tiles, (gfa_scan_tiles(Pn) + 2) * sizeof(unsigned long long)))) return rc;
    unsigned long long *path_off = (unsigned long long *) e->ex_path_off.p, *word_off = (unsigned long long *) e->ex_word_off.p,
                       *seam_off = (unsigned long long *) e->ex_seam_off.p;
    launch_ex_pair_sizes(in, prv, tail, win, pair_of, xbase, xrank, r2, kcnt, (uint32_t *) e->ex_pcnt.p, (int32_t *) e->ex_ulen.p, (int32_t *) e->ex_ulen2.p,
                         (uint32_t *) e->ex_uwords.p, (uint32_t *) e->ex_scnt.p, cnt, s);
    if ((rc = alga_check_launch(e, "k_ex_pair_sizes"))) return rc;
    launch_gfa_scan64((const uint32_t *) e->ex_pcnt.p, Pn, path_off, (unsigned long long *) e->ut_tiles.p, s);
    launch_gfa_scan64((const uint32_t *) e->ex_uwords.p, Pn, word_off, (unsigned long long *) e->ut_tiles.p, s);
    launch_gfa_scan64((const uint32_t *) e->ex_scnt.p, Pn, seam_off, (unsigned long long *) e->ut_tiles.p, s);
    if ((rc = alga_check_launch(e, "scan(pair sizes)"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, EX_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters + EX_COUNTERS, word_off + Pn, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters + EX_COUNTERS + 1, path_off + Pn, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters + EX_COUNTERS + 2, seam_off + Pn, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    unsigned long long c[EX_COUNTERS];
    for (int k = 0; k < EX_COUNTERS; k++) c[k] = e->h_counters[k];
    const uint64_t total_words = e->h_counters[EX_COUNTERS], total_entries = e->h_counters[EX_COUNTERS + 1], total_seams = e->h_counters[EX_COUNTERS + 2];
    if (c[EX_OVERFLOW]) return alga_fail(e, ALGA_ERR_CAPACITY, "an extended contig is longer than 2^31 - 1 bases");
    if ((rc = alga_ensure(e, e->ex_path_node, (size_t) (total_entries + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ex_path_pos, (size_t) (total_entries + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ex_seam_entry, (size_t) (total_seams + 1) * sizeof(int32_t)))) return rc;
    launch_ex_ids(in, xhead, xrank, r2, nxt, tail, win, pair_of, kcnt, seam_off, (int32_t *) e->ex_seam_entry.p, uid, s);
    launch_ex_layout(in, entries_in, xhead, xbase, xrank, r2, win, uid, path_off, (int32_t *) e->ex_path_node.p, (int32_t *) e->ex_path_pos.p, s);
    if ((rc = alga_check_launch(e, "k_ex_layout"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[3], s));

    // ---- sequences
    if ((rc = alga_ensure(e, e->ex_words, (size_t) (total_words + 4) * sizeof(uint32_t)))) return rc;
    launch_ut_sequence(nodes->words, nodes->stride_words, (const int32_t *) e->ex_path_node.p, (const int32_t *) e->ex_path_pos.p, path_off, word_off,
                       (const int32_t *) e->ex_ulen.p, (uint32_t) Pn, total_words, (uint32_t *) e->ex_words.p, s);
    if ((rc = alga_check_launch(e, "k_ut_sequence"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[4], s));

    // ---- the graph of the extended contigs
    uint32_t *deg = (uint32_t *) e->ct_deg.p, *epos = (uint32_t *) e->ct_epos.p;
    launch_ex_join_count(in, nxt, prv, deg, s);
    launch_exclusive_scan(deg, n2, epos, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(extended contig edges)"))) return rc;
    uint64_t mu = 0;
    if ((rc = read_u32(e, epos + n2, s, &mu))) return rc;
    for (int k = 0; k < 2; k++) {
        if ((rc = alga_ensure(e, e->ct_ekeys[k], (size_t) (mu + 1) * sizeof(unsigned long long)))) return rc;
        if ((rc = alga_ensure(e, e->ct_evals[k], (size_t) (mu + 1) * sizeof(uint32_t)))) return rc;
    }
    if ((rc = alga_ensure(e, e->ex_edges, (size_t) (mu + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->sort_temp, sort_edges_temp_bytes(mu)))) return rc;
    launch_ex_join_fill(in, nxt, prv, uid, xbase, w, epos, (unsigned long long *) e->ct_ekeys[0].p, (uint32_t *) e->ct_evals[0].p, s);
    if ((rc = alga_check_launch(e, "k_ex_join_fill"))) return rc;
    int pair_bits = 1;
    while (pair_bits < 31 && (1ll << pair_bits) < (long long) (2 * Pn)) pair_bits++;
    HIP_TRY(e, sort_edges(e->sort_temp.p, sort_edges_temp_bytes(mu), (const unsigned long long *) e->ct_ekeys[0].p, (unsigned long long *) e->ct_ekeys[1].p,
                          (const uint32_t *) e->ct_evals[0].p, (uint32_t *) e->ct_evals[1].p, mu, pair_bits, s));
    launch_keys_to_edges((const unsigned long long *) e->ct_ekeys[1].p, (const uint32_t *) e->ct_evals[1].p, mu, (alga_edge_dev *) e->ex_edges.p, s);
    if ((rc = alga_check_launch(e, "k_keys_to_edges"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[5], s));
    HIP_TRY(e, hipStreamSynchronize(s));

    // ---- the new result takes the place of the contig result
    std::swap(e->ut_ulen, e->ex_ulen); std::swap(e->ut_ulen2, e->ex_ulen2); std::swap(e->ut_words, e->ex_words); std::swap(e->ut_word_off, e->ex_word_off);
    std::swap(e->ut_path_off, e->ex_path_off); std::swap(e->ut_path_node, e->ex_path_node); std::swap(e->ut_path_pos, e->ex_path_pos);
    std::swap(e->ut_edges, e->ex_edges);
    e->cs_valid = false; e->fc_valid = false;
    e->ut_valid = true; e->ut_is_contig = true; e->ut_is_extended = true; e->ut_n_pairs = Pn; e->ut_n_edges = mu; e->ut_total_bases = c[EX_TOTAL_BASES];
    out->n_pairs = (int32_t) Pn;
    out->d_words = (const uint32_t *) e->ut_words.p; out->d_word_off = (const uint64_t *) e->ut_word_off.p; out->d_len = (const int32_t *) e->ut_ulen.p;
    out->d_path_node = (const int32_t *) e->ut_path_node.p; out->d_path_pos = (const int32_t *) e->ut_path_pos.p;
    out->d_path_off = (const uint64_t *) e->ut_path_off.p; out->d_edges = (const alga_edge *) e->ut_edges.p; out->n_edges = mu;
    if (info) {
        info->candidates = c[EX_CANDIDATES]; info->direct_links = c[EX_DIRECT]; info->links = c[EX_LINKS]; info->joinable = c[EX_JOINABLE] - 2 * cycles;
        info->ambiguous = c[EX_AMBIGUOUS]; info->cycles_cut = cycles; info->pairs_in = P; info->pairs_out = Pn;
        info->head_max = c[EX_HEAD_MAX]; info->head_passes = (c[EX_HEAD_MAX] + EX_FILL - 1) / EX_FILL;
        info->longest_nodes = c[EX_LONGEST_NODES]; info->longest_bases = c[EX_LONGEST_BASES]; info->total_bases = c[EX_TOTAL_BASES];
        info->rank_rounds = rounds + rounds2;
        double *part[5] = {&info->ms_count, &info->ms_paths, &info->ms_layout, &info->ms_seq, &info->ms_edges};
        for (int k = 0; k < 5; k++) if ((rc = evs.ms(e, k, k + 1, part[k]))) return rc;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" int alga_extend_contigs_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const alga_unitigs *u, int32_t min_chain_weight,
                                          int32_t min_connections, int32_t max_insert, int32_t flags, void *hip_stream, alga_unitigs *out,
                                          alga_extend_info *info) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    const auto t0 = std::chrono::steady_clock::now();
    if (info) *info = alga_extend_info{};
    if (!nodes || !u || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes, u and out must not be NULL");
    if (flags) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unknown extension flag");
    if (min_chain_weight < 0 || max_insert < 0) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "min_chain_weight and max_insert must not be negative");
    if (min_connections < 1) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "min_connections must be at least 1");
    if (!current_contigs(e, u)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the engine's current result");
    if (!e->ut_is_contig || e->ut_is_extended)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "the current result does not come from alga_contigs_device");
    if (nodes->n != e->ut_n_nodes) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the node set of the contig call (another node count)");
    if (nodes->n && (!nodes->len || !nodes->words || nodes->stride_words <= 0)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad node set");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    const int rc = extend_impl(e, nodes, d_pair_off, u, min_chain_weight, min_connections, max_insert, s, out, info);
    if (rc != ALGA_OK) { (void) hipStreamSynchronize(s); return rc; }
    if (info) info->ms_total = alga_ms_since(t0);
    return ALGA_OK;
}

extern "C" int alga_extend_seams_get(alga_engine *e, const alga_unitigs *u, alga_extend_seams *out) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!u || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "u and out must not be NULL");
    if (!current_contigs(e, u) || !e->ut_is_extended)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the engine's current result, or not the result of alga_extend_contigs_device");
    out->d_seam_off = (const uint64_t *) e->ex_seam_off.p; out->d_seam_entry = (const int32_t *) e->ex_seam_entry.p;
    out->n_seams = 0;
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipMemcpy(&out->n_seams, out->d_seam_off + u->n_pairs, sizeof(uint64_t), hipMemcpyDeviceToHost));
    return ALGA_OK;
}
