// alga_amd/csrc/engine_contig.hip -- C ABI of the contigs (include/alga_amd.h: alga_contigs_device; kernels in contig_kernels.hip).
//
// Host side: the order of the stages and the counts that size the next one.  E*, the ranking and the sequences are the unitig call's own
// (engine_unitig.hip, k_ut_sequence); the cut of the contracted graph H is the triangle cut's kernel on buffers of this call, so the cut's,
// the clip's and the parallel-path step's engine-owned results all stay valid.  A round reads back: the number of open chains (the group
// sort's size), the number of groups (H's size), and one block with the round's counts and the size of the next B; the ranking inside it
// reads one count per jump round as it does for the unitigs.
#include <hip/hip_runtime.h>

#include <chrono>

#include "engine_internal.h"
#include "contig_kernels.h"
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

int contigs_impl(alga_engine *e, const alga_nodes *nodes, const alga_edge_dev *d_in, uint64_t m, int32_t max_offset, hipStream_t s, alga_unitigs *out,
                 alga_contig_info *info) {
    const int32_t n = nodes->n;
    const size_t N = (size_t) n;
    int rc;
    AlgaEvents<6> evs;
    if ((rc = evs.create(e))) return rc;
    const size_t n_ucnt = UT_COUNTERS + ALGA_UT_MAX_ROUNDS;
    if ((rc = alga_ensure(e, e->ut_cnt, n_ucnt * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->ct_cnt, CT_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *ucnt = (unsigned long long *) e->ut_cnt.p, *cnt = (unsigned long long *) e->ct_cnt.p;
    HIP_TRY(e, hipMemsetAsync(ucnt, 0, n_ucnt * sizeof(unsigned long long), s));
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    if ((rc = alga_ut_check(e, nodes, d_in, m, ucnt, s))) return rc;
    // the input is valid: from here on the previous result's buffers are rewritten
    e->ut_valid = false; e->cs_valid = false; e->fc_valid = false; e->ut_is_contig = false; e->ut_is_extended = false;

    // ---- E*: the input is consumed here, before anything else of this call runs
    uint64_t ms = 0;
    if ((rc = alga_ut_estar(e, nodes, d_in, m, ucnt, s, &ms))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));
    for (int k = 0; k < 2; k++) {
        if ((rc = alga_ensure(e, e->ut_rank[k], (N + 1) * sizeof(UtRank)))) return rc;
        if ((rc = alga_ensure(e, e->ct_B[k], (size_t) (ms + 1) * sizeof(alga_edge_dev)))) return rc;
        if ((rc = alga_ensure(e, e->ct_keys[k], (size_t) (ms + 1) * sizeof(unsigned long long)))) return rc;
        if ((rc = alga_ensure(e, e->ct_vals[k], (size_t) (ms + 1) * sizeof(uint32_t)))) return rc;
    }
    if ((rc = alga_ensure(e, e->ut_nxt, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_noff, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_prv, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_tail, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_win, (N + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_pair, (N + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_rowptr, (N + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_pflag, (N + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_runkey, (N + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_headchain, (N + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_chain, (size_t) (ms + 1) * sizeof(CtChain)))) return rc;
    if ((rc = alga_ensure(e, e->ct_drop, (size_t) ms + 16))) return rc;
    if ((rc = alga_ensure(e, e->ct_flag, (size_t) (ms + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_pos, (size_t) (ms + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_hw, (size_t) (ms + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_hk, (size_t) (ms + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_H, (size_t) (ms + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->ct_hsorted, (size_t) (ms + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->ct_hlist, (size_t) (ms + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->ct_hrow, (N + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_hcnt, (N + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_win, (size_t) (ms + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_pair, (size_t) (ms + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_oid, (size_t) (ms + 2) * sizeof(uint32_t)))) return rc;
    int32_t *nxt = (int32_t *) e->ut_nxt.p, *noff = (int32_t *) e->ut_noff.p, *prv = (int32_t *) e->ut_prv.p, *tail = (int32_t *) e->ut_tail.p;
    uint32_t *pflag = (uint32_t *) e->ct_pflag.p, *runkey = (uint32_t *) e->ct_runkey.p, *headchain = (uint32_t *) e->ct_headchain.p;
    uint32_t *flag = (uint32_t *) e->ct_flag.p, *pos = (uint32_t *) e->ct_pos.p, *hw = (uint32_t *) e->ct_hw.p, *hk = (uint32_t *) e->ct_hk.p;
    unsigned long long *keys0 = (unsigned long long *) e->ct_keys[0].p, *keys1 = (unsigned long long *) e->ct_keys[1].p;
    uint32_t *vals0 = (uint32_t *) e->ct_vals[0].p, *vals1 = (uint32_t *) e->ct_vals[1].p;
    CtChain *chain = (CtChain *) e->ct_chain.p;
    uint8_t *drop = (uint8_t *) e->ct_drop.p;
    alga_edge_dev *H = (alga_edge_dev *) e->ct_H.p;
    uint32_t *hrow = (uint32_t *) e->ct_hrow.p, *hcnt = (uint32_t *) e->ct_hcnt.p;
    int node_bits = 1;
    while (node_bits < 31 && (1ll << node_bits) < (long long) n) node_bits++;

    // ---- the rounds
    const alga_edge_dev *B = (const alga_edge_dev *) e->ut_estar.p;
    const uint32_t *rowptr = (const uint32_t *) e->ut_rowptr.p;
    uint64_t mb = ms, touched_first = 0, rounds = 0;
    int rank_rounds_total = 0, cur = 0;
    unsigned long long c[CT_COUNTERS] = {}, cycles = 0;
    for (;; rounds++) {
        if (rounds) HIP_TRY(e, hipMemsetAsync(ucnt, 0, n_ucnt * sizeof(unsigned long long), s));
        HIP_TRY(e, hipMemsetAsync(cnt, 0, CT_COUNTERS * sizeof(unsigned long long), s));
        HIP_TRY(e, hipMemsetAsync(drop, 0, (size_t) mb + 16, s));
        HIP_TRY(e, hipMemsetAsync(runkey, 0xFF, (N + 1) * sizeof(uint32_t), s));
        launch_ct_pflags(B, rowptr, n, pflag, s);
        launch_ct_next(B, rowptr, pflag, n, nxt, noff, s);
        launch_ut_prev(nxt, n, prv, s);
        if ((rc = alga_check_launch(e, "k_ct_next"))) return rc;
        int rr = 0;
        if ((rc = alga_ut_rank(e, nodes->len, n, nxt, noff, prv, ucnt, pflag, cur, rr, s))) return rc;
        rank_rounds_total += rr;
        const UtRank *r = (const UtRank *) e->ut_rank[cur].p;
        launch_ct_run_info(r, pflag, nxt, rowptr, n, tail, runkey, cnt, s);
        launch_ct_chains(B, rowptr, mb, pflag, r, tail, runkey, chain, headchain, flag, cnt, s);
        if ((rc = alga_check_launch(e, "k_ct_chains"))) return rc;
        launch_exclusive_scan(flag, mb, pos, (uint64_t *) e->scan_scratch.p, s);
        if ((rc = alga_check_launch(e, "scan(open chains)"))) return rc;
        uint64_t no = 0, nh = 0;
        if ((rc = read_u32(e, pos + mb, s, &no))) return rc;
        if (no) {
            launch_ct_open_keys(B, flag, pos, chain, mb, keys0, vals0, s);
            if ((rc = alga_check_launch(e, "k_ct_open_keys"))) return rc;
            HIP_TRY(e, sort_edges(e->sort_temp.p, sort_edges_temp_bytes(2 * m), keys0, keys1, vals0, vals1, no, node_bits, s));
            launch_ct_groups(keys1, vals1, no, chain, max_offset, flag, hw, hk, drop, cnt, s);
            if ((rc = alga_check_launch(e, "k_ct_groups"))) return rc;
            launch_exclusive_scan(flag, no, pos, (uint64_t *) e->scan_scratch.p, s);
            if ((rc = alga_check_launch(e, "scan(groups)"))) return rc;
            if ((rc = read_u32(e, pos + no, s, &nh))) return rc;
            // H, one edge per group in (a, c) order, and the triangle cut on it
            launch_ut_compact_edges(keys1, flag, pos, hw, no, H, s);
            launch_edge_rowptr(H, nh, n, hrow, s);
            launch_cut_triangles(H, hrow, n, max_offset, (alga_edge_dev *) e->ct_hsorted.p, (alga_edge_dev *) e->ct_hlist.p, hcnt, cnt + CT_CUT_REMOVED, s);
            if ((rc = alga_check_launch(e, "k_cut_triangles(H)"))) return rc;
            launch_ct_cut_back(keys1, vals1, no, flag, hw, hk, chain, hrow, (const alga_edge_dev *) e->ct_hlist.p, hcnt, drop, cnt, s);
            if ((rc = alga_check_launch(e, "k_ct_cut_back"))) return rc;
        }
        uint32_t *keep = (uint32_t *) e->ct_win.p, *kpos = (uint32_t *) e->ct_pair.p;      // (free until the numbering)
        launch_ct_edge_keep(B, rowptr, mb, pflag, r, headchain, drop, keep, s);
        launch_exclusive_scan(keep, mb, kpos, (uint64_t *) e->scan_scratch.p, s);
        if ((rc = alga_check_launch(e, "scan(kept edges)"))) return rc;
        // the round's block of counts
        HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, CT_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipMemcpyAsync(e->h_counters + CT_COUNTERS, ucnt + UT_CYCLES, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipMemcpyAsync(e->h_counters + CT_COUNTERS + 1, kpos + mb, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        for (int k = 0; k < CT_COUNTERS; k++) c[k] = e->h_counters[k];
        cycles = e->h_counters[CT_COUNTERS];
        const uint64_t kept = *(const uint32_t *) (e->h_counters + CT_COUNTERS + 1);
        if (c[CT_OVERFLOW]) return alga_fail(e, ALGA_ERR_CAPACITY, "a chain weighs more than 2^31 - 1");
        if (rounds == 0) touched_first = c[CT_TOUCHED];
        if (info && rounds < ALGA_CONTIG_MAX_ROUNDS) {
            info->chains[rounds] = c[CT_CHAINS]; info->parallel_drops[rounds] = c[CT_PARALLEL]; info->groups_cut[rounds] = c[CT_GROUPS_CUT];
            info->base_edges_dropped[rounds] = mb - kept;
        }
        if (c[CT_GROUPS_CUT] != c[CT_CUT_REMOVED]) return alga_fail(e, ALGA_ERR_HIP, "contigs: the cut of H and its mapping back disagree");
        if (kept == mb) { rounds++; break; }
        alga_edge_dev *Bn = (alga_edge_dev *) e->ct_B[rounds & 1].p;
        launch_ct_compact(B, keep, kpos, mb, Bn, s);
        launch_edge_rowptr(Bn, kept, n, (uint32_t *) e->ct_rowptr.p, s);
        if ((rc = alga_check_launch(e, "k_ct_compact"))) return rc;
        B = Bn; rowptr = (const uint32_t *) e->ct_rowptr.p; mb = kept;
    }
    const UtRank *r = (const UtRank *) e->ut_rank[cur].p;
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));

    // ---- numbering, sizes, layout (the chain records are those of the final B: its round dropped nothing)
    uint32_t *win = (uint32_t *) e->ct_win.p, *pair_of = (uint32_t *) e->ct_pair.p, *oid = (uint32_t *) e->ct_oid.p;
    launch_ct_winners(B, mb, pflag, chain, win, s);
    launch_exclusive_scan(win, mb, pair_of, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(winners)"))) return rc;
    uint64_t P = 0;
    if ((rc = read_u32(e, pair_of + mb, s, &P))) return rc;
    if (P >= (1ull << 30)) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^30 contig pairs");
    if ((rc = alga_ensure(e, e->ut_pcnt, (size_t) (P + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_uwords, (size_t) (P + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_ulen, (size_t) (P + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_ulen2, (size_t) (2 * P + 2) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_path_off, (size_t) (P + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->ut_word_off, (size_t) (P + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->ut_tiles, (gfa_scan_tiles(P) + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->ct_cid, (size_t) (2 * P + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_deg, (size_t) (2 * P + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ct_epos, (size_t) (2 * P + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(std::max<uint64_t>(std::max<uint64_t>(2 * m, N), 2 * P))))) return rc;
    unsigned long long *path_off = (unsigned long long *) e->ut_path_off.p, *word_off = (unsigned long long *) e->ut_word_off.p;
    uint32_t *cid = (uint32_t *) e->ct_cid.p;
    launch_ct_pair_sizes(B, chain, nodes->len, win, pair_of, mb, (uint32_t *) e->ut_pcnt.p, (int32_t *) e->ut_ulen.p, (int32_t *) e->ut_ulen2.p,
                         (uint32_t *) e->ut_uwords.p, oid, cid, cnt, s);
    if ((rc = alga_check_launch(e, "k_ct_pair_sizes"))) return rc;
    launch_gfa_scan64((const uint32_t *) e->ut_pcnt.p, P, path_off, (unsigned long long *) e->ut_tiles.p, s);
    launch_gfa_scan64((const uint32_t *) e->ut_uwords.p, P, word_off, (unsigned long long *) e->ut_tiles.p, s);
    if ((rc = alga_check_launch(e, "scan(pair sizes)"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, CT_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters + CT_COUNTERS, word_off + P, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters + CT_COUNTERS + 1, path_off + P, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    for (int k = 0; k < CT_COUNTERS; k++) c[k] = e->h_counters[k];
    const uint64_t total_words = e->h_counters[CT_COUNTERS], total_entries = e->h_counters[CT_COUNTERS + 1];
    if (c[CT_OVERFLOW]) return alga_fail(e, ALGA_ERR_CAPACITY, "a contig is longer than 2^31 - 1 bases");
    if ((rc = alga_ensure(e, e->ut_path_node, (size_t) (total_entries + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_path_pos, (size_t) (total_entries + 1) * sizeof(int32_t)))) return rc;
    launch_ct_layout_ends(B, mb, chain, win, pair_of, path_off, (int32_t *) e->ut_path_node.p, (int32_t *) e->ut_path_pos.p, s);
    launch_ct_layout_inner(B, n, pflag, r, headchain, win, pair_of, path_off, (int32_t *) e->ut_path_node.p, (int32_t *) e->ut_path_pos.p, s);
    if ((rc = alga_check_launch(e, "k_ct_layout"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[3], s));

    // ---- sequences
    if ((rc = alga_ensure(e, e->ut_words, (size_t) (total_words + 4) * sizeof(uint32_t)))) return rc;
    launch_ut_sequence(nodes->words, nodes->stride_words, (const int32_t *) e->ut_path_node.p, (const int32_t *) e->ut_path_pos.p, path_off, word_off,
                       (const int32_t *) e->ut_ulen.p, (uint32_t) P, total_words, (uint32_t *) e->ut_words.p, s);
    if ((rc = alga_check_launch(e, "k_ut_sequence"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[4], s));

    // ---- the contig graph: the join at the junction nodes
    uint32_t *deg = (uint32_t *) e->ct_deg.p, *epos = (uint32_t *) e->ct_epos.p;
    launch_ct_join_count(cid, chain, rowptr, 2 * P, deg, s);
    launch_exclusive_scan(deg, 2 * P, epos, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(contig edges)"))) return rc;
    uint64_t mu = 0;
    if ((rc = read_u32(e, epos + 2 * P, s, &mu))) return rc;
    if (mu >= (1ull << 31) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^31 contig edges");
    for (int k = 0; k < 2; k++) {
        if ((rc = alga_ensure(e, e->ct_ekeys[k], (size_t) (mu + 1) * sizeof(unsigned long long)))) return rc;
        if ((rc = alga_ensure(e, e->ct_evals[k], (size_t) (mu + 1) * sizeof(uint32_t)))) return rc;
    }
    if ((rc = alga_ensure(e, e->ut_edges, (size_t) (mu + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->sort_temp, sort_edges_temp_bytes(mu)))) return rc;
    launch_ct_join_fill(cid, chain, rowptr, oid, epos, 2 * P, (unsigned long long *) e->ct_ekeys[0].p, (uint32_t *) e->ct_evals[0].p, s);
    if ((rc = alga_check_launch(e, "k_ct_join_fill"))) return rc;
    int pair_bits = 1;
    while (pair_bits < 31 && (1ll << pair_bits) < (long long) (2 * P)) pair_bits++;
    HIP_TRY(e, sort_edges(e->sort_temp.p, sort_edges_temp_bytes(mu), (const unsigned long long *) e->ct_ekeys[0].p, (unsigned long long *) e->ct_ekeys[1].p,
                          (const uint32_t *) e->ct_evals[0].p, (uint32_t *) e->ct_evals[1].p, mu, pair_bits, s));
    launch_keys_to_edges((const unsigned long long *) e->ct_ekeys[1].p, (const uint32_t *) e->ct_evals[1].p, mu, (alga_edge_dev *) e->ut_edges.p, s);
    if ((rc = alga_check_launch(e, "k_keys_to_edges"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[5], s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->ut_valid = true; e->ut_is_contig = true; e->ut_n_pairs = P; e->ut_n_edges = mu; e->ut_n_nodes = n; e->ut_total_bases = c[CT_TOTAL_BASES];
    out->n_pairs = (int32_t) P;
    out->d_words = (const uint32_t *) e->ut_words.p; out->d_word_off = (const uint64_t *) word_off; out->d_len = (const int32_t *) e->ut_ulen.p;
    out->d_path_node = (const int32_t *) e->ut_path_node.p; out->d_path_pos = (const int32_t *) e->ut_path_pos.p; out->d_path_off = (const uint64_t *) path_off;
    out->d_edges = (const alga_edge *) e->ut_edges.p; out->n_edges = mu;
    if (info) {
        info->edges_in = m; info->edges_sym = ms; info->rounds = rounds; info->final_edges = mb;
        info->path_nodes = c[CT_PATH_NODES]; info->junction_nodes = c[CT_TOUCHED] - c[CT_PATH_NODES]; info->cycles_cut = cycles;
        info->closed_chains = c[CT_CLOSED]; info->reads_dropped = touched_first - c[CT_TOUCHED];
        info->longest_nodes = c[CT_LONGEST_NODES]; info->longest_bases = c[CT_LONGEST_BASES]; info->total_bases = c[CT_TOTAL_BASES];
        info->rank_rounds = rank_rounds_total;
        double *part[5] = {&info->ms_sym, &info->ms_rounds, &info->ms_layout, &info->ms_seq, &info->ms_edges};
        for (int k = 0; k < 5; k++) if ((rc = evs.ms(e, k, k + 1, part[k]))) return rc;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" int alga_contigs_device(alga_engine *e, const alga_nodes *nodes, const alga_edge *d_edges, uint64_t n_edges, int32_t max_offset, int32_t flags,
                                   void *hip_stream, alga_unitigs *out, alga_contig_info *info) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    const auto t0 = std::chrono::steady_clock::now();
    if (info) *info = alga_contig_info{};
    if (!nodes || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes and out must not be NULL");
    if (flags) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unknown contig flag");
    if (max_offset < 0) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "max_offset must not be negative");
    if (nodes->n < 0 || (nodes->n & 1)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "the node count must be even (twin layout)");
    if ((nodes->n && (!nodes->len || !nodes->words || nodes->stride_words <= 0)) || (n_edges && !d_edges))
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad node set or edge list");
    if (n_edges && !nodes->n) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "edge endpoint outside [0, n)");
    if (n_edges >= (1ull << 31) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^31 edges");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    const int rc = contigs_impl(e, nodes, (const alga_edge_dev *) d_edges, n_edges, max_offset, s, out, info);
    if (rc != ALGA_OK) { (void) hipStreamSynchronize(s); return rc; }
    if (info) info->ms_total = alga_ms_since(t0);
    return ALGA_OK;
}
