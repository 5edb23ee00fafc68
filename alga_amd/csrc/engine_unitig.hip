// alga_amd/csrc/engine_unitig.hip -- C ABI of the unitig graph (include/alga_amd.h: alga_unitigs_device; kernels in unitig_kernels.hip).
//
// Host side: the order of the stages and the few counts the host has to know to size the next one -- the device's verdict on the input, the
// size of E*, one counter per pointer-jumping round (the ranking stops when the number of unresolved nodes no longer falls: a fixed
// schedule of ceil(log2 n) rounds would run 27 rounds at 90 M nodes where the longest path needs 21; a read-back costs ~10 us against
// up to 16 ms for a round), the number of pairs, the total words, the number of unitig edges.
#include <hip/hip_runtime.h>

#include <chrono>

#include "engine_internal.h"
#include "gfa_kernels.h"
#include "simplify_kernels.h"
#include "contig_kernels.h"
#include "unitig_kernels.h"

using namespace alga;

namespace {

int read_u64(alga_engine *e, const void *d_src, int n_words, hipStream_t s) {
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, d_src, (size_t) n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return ALGA_OK;
}
int read_u32(alga_engine *e, const void *d_src, hipStream_t s, uint64_t *out) {
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, d_src, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    *out = *(const uint32_t *) e->h_counters;
    return ALGA_OK;
}

// pointer jumping until the number of unresolved nodes is 0 or no longer falls; cur = the array that holds the last round's records
int rank_rounds(alga_engine *e, DevBuf *buf, int32_t n, unsigned long long *cnt, int &cur, int &rounds, uint64_t &open, hipStream_t s) {
    uint64_t before = ~0ull;
    int rc;
    open = 0;
    for (int k = 0; k < 34; k++) {
        if (rounds >= ALGA_UT_MAX_ROUNDS) return alga_fail(e, ALGA_ERR_HIP, "unitigs: the list ranking did not settle");
        unsigned long long *slot = cnt + UT_COUNTERS + rounds;
        launch_ut_rank_jump((const UtRank *) buf[cur].p, (UtRank *) buf[cur ^ 1].p, n, slot, s);
        if ((rc = alga_check_launch(e, "k_ut_rank_jump"))) return rc;
        cur ^= 1; rounds++;
        if ((rc = read_u64(e, slot, 1, s))) return rc;
        open = e->h_counters[0];
        if (open == 0 || open == before) return ALGA_OK;
        before = open;
    }
    return ALGA_OK;
}

}  // namespace

// step 1 (shared with engine_contig.hip): the device's verdict on the input; nothing but cnt[] is written
int alga_ut_check(alga_engine *e, const alga_nodes *nodes, const alga_edge_dev *d_in, uint64_t m, unsigned long long *cnt, hipStream_t s) {
    int rc;
    launch_ut_check(nodes->len, nodes->n, d_in, m, cnt, s);
    if ((rc = alga_check_launch(e, "k_ut_check"))) return rc;
    if ((rc = read_u64(e, cnt, 1, s))) return rc;
    if (const unsigned long long bad = e->h_counters[UT_FLAGS]) {
        const char *why = (bad & UT_BAD_LEN) ? "node length negative or above 2^30" : (bad & UT_BAD_TWIN_LEN) ? "len[2k] != len[2k + 1]"
                        : (bad & UT_BAD_ID) ? "edge endpoint outside [0, n)" : (bad & UT_BAD_DEAD) ? "edge endpoint is a removed node (len 0)"
                        : "edge is not a dovetail: 0 <= offset < len[src] and offset + len[dst] >= len[src]";
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, why);
    }
    return ALGA_OK;
}

// step 2 (shared): E* in ut_estar, its row pointers in ut_rowptr; the sort buffers, flags and scan positions are sized for 2 m records
int alga_ut_estar(alga_engine *e, const alga_nodes *nodes, const alga_edge_dev *d_in, uint64_t m, unsigned long long *cnt, hipStream_t s, uint64_t *ms_out) {
    const int32_t n = nodes->n;
    const uint64_t m2 = 2 * m;
    const size_t N = (size_t) n;
    int rc;
    for (int k = 0; k < 2; k++) {
        if ((rc = alga_ensure(e, e->ut_keys[k], (size_t) (m2 + 1) * sizeof(unsigned long long)))) return rc;
        if ((rc = alga_ensure(e, e->ut_vals[k], (size_t) (m2 + 1) * sizeof(uint32_t)))) return rc;
    }
    if ((rc = alga_ensure(e, e->ut_flag, (size_t) (m2 + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_pos, (size_t) (m2 + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_best, (size_t) (m2 + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_estar, (size_t) (m2 + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->ut_rowptr, (N + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->sort_temp, sort_edges_temp_bytes(m2)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(std::max<uint64_t>(m2, N))))) return rc;
    unsigned long long *keys0 = (unsigned long long *) e->ut_keys[0].p, *keys1 = (unsigned long long *) e->ut_keys[1].p;
    uint32_t *vals0 = (uint32_t *) e->ut_vals[0].p, *vals1 = (uint32_t *) e->ut_vals[1].p;
    uint32_t *flag = (uint32_t *) e->ut_flag.p, *pos = (uint32_t *) e->ut_pos.p;
    int node_bits = 1;
    while (node_bits < 31 && (1ll << node_bits) < (long long) n) node_bits++;
    launch_ut_twins(nodes->len, d_in, m, keys0, vals0, s);
    if ((rc = alga_check_launch(e, "k_ut_twins"))) return rc;
    HIP_TRY(e, sort_edges(e->sort_temp.p, sort_edges_temp_bytes(m2), keys0, keys1, vals0, vals1, m2, node_bits, s));
    launch_ut_group_heads(keys1, vals1, m2, flag, (uint32_t *) e->ut_best.p, cnt, s);
    if ((rc = alga_check_launch(e, "k_ut_group_heads"))) return rc;
    launch_exclusive_scan(flag, m2, pos, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(group heads)"))) return rc;
    uint64_t ms = 0;
    if ((rc = read_u32(e, pos + m2, s, &ms))) return rc;
    launch_ut_compact_edges(keys1, flag, pos, (const uint32_t *) e->ut_best.p, m2, (alga_edge_dev *) e->ut_estar.p, s);
    if ((rc = alga_check_launch(e, "k_ut_compact_edges"))) return rc;
    launch_edge_rowptr((const alga_edge_dev *) e->ut_estar.p, ms, n, (uint32_t *) e->ut_rowptr.p, s);
    if ((rc = alga_check_launch(e, "k_edge_rowptr"))) return rc;
    *ms_out = ms;
    return ALGA_OK;
}

// the list ranking along nxt[] / prv[] (shared), in both forms, with the cycle-minimum jump for what stays unresolved.  p_flag == nullptr: the
// unitig cut (step 4); else the contig form: m and m^1 leave P (k_ct_open_cycles).  Records: e->ut_rank[cur]; ut_win / ut_pair are scratch.
int alga_ut_rank(alga_engine *e, const int32_t *len, int32_t n, int32_t *nxt, const int32_t *noff, int32_t *prv, unsigned long long *cnt, uint32_t *p_flag,
                 int &cur, int &rounds, hipStream_t s) {
    const size_t N = (size_t) n;
    int rc;
    cur = 0;
    uint64_t open = 0;
    launch_ut_rank_init(len, prv, noff, n, 0, (UtRank *) e->ut_rank[0].p, s);
    if ((rc = alga_check_launch(e, "k_ut_rank_init"))) return rc;
    const bool ruling = e->opt_unitig_ruling < 0 ? n >= (1 << 16) : e->opt_unitig_ruling != 0;
    if (ruling && n > 0) {
        // the rulers (heads and one id in 64) are ranked among themselves; every node between two ranked rulers then gets its final record,
        // and the rounds below find nothing left to do unless there are cycles
        uint32_t *rflag = (uint32_t *) e->ut_win.p, *ridx = (uint32_t *) e->ut_pair.p;         // (free until the numbering)
        if ((rc = alga_ensure(e, e->ut_link, (N + 1) * sizeof(int2)))) return rc;
        launch_ut_ruler_flags(len, prv, n, rflag, s);
        launch_ut_links(nxt, noff, n, (int2 *) e->ut_link.p, s);
        launch_exclusive_scan(rflag, (uint64_t) n, ridx, (uint64_t *) e->scan_scratch.p, s);
        if ((rc = alga_check_launch(e, "scan(rulers)"))) return rc;
        uint64_t R = 0;
        if ((rc = read_u32(e, ridx + n, s, &R))) return rc;
        if ((rc = alga_ensure(e, e->ut_rnode, (size_t) (R + 1) * sizeof(int32_t)))) return rc;
        for (int k = 0; k < 2; k++) if ((rc = alga_ensure(e, e->ut_rrec[k], (size_t) (R + 1) * sizeof(UtRank)))) return rc;
        launch_ut_ruler_list(rflag, ridx, prv, n, (int32_t *) e->ut_rnode.p, (UtRank *) e->ut_rrec[0].p, s);
        launch_ut_ruler_walk1((const int2 *) e->ut_link.p, (const int32_t *) e->ut_rnode.p, ridx, (uint32_t) R, (UtRank *) e->ut_rrec[0].p, s);
        if ((rc = alga_check_launch(e, "k_ut_ruler_walk1"))) return rc;
        int rcur = 0;
        if (R && (rc = rank_rounds(e, e->ut_rrec, (int32_t) R, cnt, rcur, rounds, open, s))) return rc;
        launch_ut_ruler_walk2((const int2 *) e->ut_link.p, (const int32_t *) e->ut_rnode.p, (const UtRank *) e->ut_rrec[rcur].p, (uint32_t) R, (UtRank *) e->ut_rank[0].p, s);
        if ((rc = alga_check_launch(e, "k_ut_ruler_walk2"))) return rc;
    }
    if (n > 0 && (rc = rank_rounds(e, e->ut_rank, n, cnt, cur, rounds, open, s))) return rc;
    if (open) {                                                     // what is left lies on cycles of compactable edges
        for (int k = 0; k < 2; k++) if ((rc = alga_ensure(e, e->ut_min[k], (N + 1) * sizeof(UtMin)))) return rc;
        const UtRank *r = (const UtRank *) e->ut_rank[cur].p;
        int mc = 0, jumps = 1;
        while (jumps < 34 && (1ull << (jumps - 1)) < open) jumps++;  // 2^jumps >= 2 * open: every node has seen its whole cycle
        launch_ut_min_init(r, prv, n, (UtMin *) e->ut_min[0].p, s);
        for (int k = 0; k < jumps; k++) { launch_ut_min_jump(r, (const UtMin *) e->ut_min[mc].p, (UtMin *) e->ut_min[mc ^ 1].p, n, s); mc ^= 1; }
        if (p_flag) launch_ct_open_cycles(r, (const UtMin *) e->ut_min[mc].p, n, nxt, prv, p_flag, cnt, s);
        else launch_ut_cut(r, (const UtMin *) e->ut_min[mc].p, n, nxt, prv, cnt, s);
        launch_ut_rank_init(len, prv, noff, n, 1, (UtRank *) e->ut_rank[cur].p, s);
        if ((rc = alga_check_launch(e, "unitig cycle cuts"))) return rc;
        if ((rc = rank_rounds(e, e->ut_rank, n, cnt, cur, rounds, open, s))) return rc;
        if (open) return alga_fail(e, ALGA_ERR_HIP, "unitigs: nodes left unranked after the cycle cuts");
    }
    return ALGA_OK;
}

namespace {

int unitigs_impl(alga_engine *e, const alga_nodes *nodes, const alga_edge_dev *d_in, uint64_t m, int32_t flags, hipStream_t s, alga_unitigs *out,
                 alga_unitig_info *info) {
    const int32_t n = nodes->n;
    const uint64_t m2 = 2 * m;
    int rc;
    AlgaEvents<6> evs;
    if ((rc = evs.create(e))) return rc;
    const size_t n_cnt = UT_COUNTERS + ALGA_UT_MAX_ROUNDS;
    if ((rc = alga_ensure(e, e->ut_cnt, n_cnt * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->ut_cnt.p;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, n_cnt * sizeof(unsigned long long), s));
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    if ((rc = alga_ut_check(e, nodes, d_in, m, cnt, s))) return rc;
    // the input is valid: from here on the previous result's buffers are rewritten
    e->ut_valid = false; e->cs_valid = false; e->fc_valid = false; e->ut_is_contig = false; e->ut_is_extended = false;
    const size_t N = (size_t) n;
    for (int k = 0; k < 2; k++) if ((rc = alga_ensure(e, e->ut_rank[k], (N + 1) * sizeof(UtRank)))) return rc;
    if ((rc = alga_ensure(e, e->ut_nxt, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_noff, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_prv, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_tail, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_win, (N + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_pair, (N + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_uid, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_path_node, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_path_pos, (N + 1) * sizeof(int32_t)))) return rc;
    // ---- E*: twins, sort, the smallest offset per (src, dst), row pointers
    uint64_t ms = 0;
    if ((rc = alga_ut_estar(e, nodes, d_in, m, cnt, s, &ms))) return rc;
    unsigned long long *keys0 = (unsigned long long *) e->ut_keys[0].p, *keys1 = (unsigned long long *) e->ut_keys[1].p;
    uint32_t *vals0 = (uint32_t *) e->ut_vals[0].p, *vals1 = (uint32_t *) e->ut_vals[1].p;
    uint32_t *flag = (uint32_t *) e->ut_flag.p, *pos = (uint32_t *) e->ut_pos.p, *rowptr = (uint32_t *) e->ut_rowptr.p;
    alga_edge_dev *estar = (alga_edge_dev *) e->ut_estar.p;
    int32_t *nxt = (int32_t *) e->ut_nxt.p, *noff = (int32_t *) e->ut_noff.p, *prv = (int32_t *) e->ut_prv.p, *tail = (int32_t *) e->ut_tail.p;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    // ---- next / prev, list ranking, cycles
    launch_ut_next(estar, rowptr, n, nxt, noff, s);
    launch_ut_prev(nxt, n, prv, s);
    int cur = 0, rounds = 0;
    if ((rc = alga_ut_rank(e, nodes->len, n, nxt, noff, prv, cnt, nullptr, cur, rounds, s))) return rc;
    const UtRank *r = (const UtRank *) e->ut_rank[cur].p;
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));

    // ---- numbering, sizes, layout
    uint32_t *win = (uint32_t *) e->ut_win.p, *pair_of = (uint32_t *) e->ut_pair.p;
    launch_ut_tails(r, nodes->len, nxt, n, tail, s);
    launch_ut_winners(r, nodes->len, prv, tail, rowptr, n, (flags & ALGA_UNITIG_SKIP_ISOLATED) ? 1 : 0, win, cnt, s);
    if ((rc = alga_check_launch(e, "k_ut_winners"))) return rc;
    launch_exclusive_scan(win, (uint64_t) n, pair_of, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(winners)"))) return rc;
    uint64_t P = 0;
    if ((rc = read_u32(e, pair_of + n, s, &P))) return rc;
    if (P >= (1ull << 30)) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^30 unitig pairs");
    if ((rc = alga_ensure(e, e->ut_pcnt, (size_t) (P + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_uwords, (size_t) (P + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_ulen, (size_t) (P + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_ulen2, (size_t) (2 * P + 2) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->ut_path_off, (size_t) (P + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->ut_word_off, (size_t) (P + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->ut_tiles, (gfa_scan_tiles(P) + 2) * sizeof(unsigned long long)))) return rc;
    unsigned long long *path_off = (unsigned long long *) e->ut_path_off.p, *word_off = (unsigned long long *) e->ut_word_off.p;
    launch_ut_pair_sizes(r, nodes->len, tail, win, pair_of, n, (uint32_t *) e->ut_pcnt.p, (int32_t *) e->ut_ulen.p, (int32_t *) e->ut_ulen2.p, (uint32_t *) e->ut_uwords.p, cnt, s);
    if ((rc = alga_check_launch(e, "k_ut_pair_sizes"))) return rc;
    launch_gfa_scan64((const uint32_t *) e->ut_pcnt.p, P, path_off, (unsigned long long *) e->ut_tiles.p, s);
    launch_gfa_scan64((const uint32_t *) e->ut_uwords.p, P, word_off, (unsigned long long *) e->ut_tiles.p, s);
    if ((rc = alga_check_launch(e, "scan(pair sizes)"))) return rc;
    uint64_t total_words = 0;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters + UT_COUNTERS, word_off + P, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if ((rc = read_u64(e, cnt, UT_COUNTERS, s))) return rc;
    total_words = e->h_counters[UT_COUNTERS];
    unsigned long long c[UT_COUNTERS];
    for (int k = 0; k < UT_COUNTERS; k++) c[k] = e->h_counters[k];
    if (c[UT_OVERFLOW]) return alga_fail(e, ALGA_ERR_CAPACITY, "a unitig is longer than 2^31 - 1 bases");
    launch_ut_layout(r, nodes->len, tail, win, pair_of, path_off, n, (int32_t *) e->ut_path_node.p, (int32_t *) e->ut_path_pos.p, (int32_t *) e->ut_uid.p, s);
    if ((rc = alga_check_launch(e, "k_ut_layout"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[3], s));

    // ---- sequences
    if ((rc = alga_ensure(e, e->ut_words, (size_t) (total_words + 4) * sizeof(uint32_t)))) return rc;
    launch_ut_sequence(nodes->words, nodes->stride_words, (const int32_t *) e->ut_path_node.p, (const int32_t *) e->ut_path_pos.p, path_off, word_off,
                       (const int32_t *) e->ut_ulen.p, (uint32_t) P, total_words, (uint32_t *) e->ut_words.p, s);
    if ((rc = alga_check_launch(e, "k_ut_sequence"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[4], s));

    // ---- unitig edges
    launch_ut_edge_flags(estar, ms, nxt, flag, s);
    launch_exclusive_scan(flag, ms, pos, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(unitig edges)"))) return rc;
    uint64_t mu = 0;
    if ((rc = read_u32(e, pos + ms, s, &mu))) return rc;
    if ((rc = alga_ensure(e, e->ut_edges, (size_t) (mu + 1) * sizeof(alga_edge_dev)))) return rc;
    launch_ut_edges(estar, ms, flag, pos, (const int32_t *) e->ut_uid.p, r, keys0, vals0, s);
    if ((rc = alga_check_launch(e, "k_ut_edges"))) return rc;
    int pair_bits = 1;
    while (pair_bits < 31 && (1ll << pair_bits) < (long long) (2 * P)) pair_bits++;
    HIP_TRY(e, sort_edges(e->sort_temp.p, sort_edges_temp_bytes(m2), keys0, keys1, vals0, vals1, mu, pair_bits, s));
    launch_keys_to_edges(keys1, vals1, mu, (alga_edge_dev *) e->ut_edges.p, s);
    if ((rc = alga_check_launch(e, "k_keys_to_edges"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[5], s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->ut_valid = true; e->ut_n_pairs = P; e->ut_n_edges = mu; e->ut_n_nodes = n; e->ut_total_bases = c[UT_TOTAL_BASES];
    out->n_pairs = (int32_t) P;
    out->d_words = (const uint32_t *) e->ut_words.p; out->d_word_off = (const uint64_t *) word_off; out->d_len = (const int32_t *) e->ut_ulen.p;
    out->d_path_node = (const int32_t *) e->ut_path_node.p; out->d_path_pos = (const int32_t *) e->ut_path_pos.p; out->d_path_off = (const uint64_t *) path_off;
    out->d_edges = (const alga_edge *) e->ut_edges.p; out->n_edges = mu;
    if (info) {
        info->edges_in = m; info->edges_sym = ms; info->twins_added = c[UT_TWINS_ADDED]; info->compactable = ms - mu; info->cycles_cut = c[UT_CYCLES];
        info->isolated_skipped = c[UT_ISOLATED]; info->longest_nodes = c[UT_LONGEST_NODES]; info->longest_bases = c[UT_LONGEST_BASES];
        info->total_bases = c[UT_TOTAL_BASES]; info->total_nodes = c[UT_TOTAL_NODES]; info->rank_rounds = rounds;
        double *part[5] = {&info->ms_sym, &info->ms_rank, &info->ms_layout, &info->ms_seq, &info->ms_edges};
        for (int k = 0; k < 5; k++) if ((rc = evs.ms(e, k, k + 1, part[k]))) return rc;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" int alga_unitigs_device(alga_engine *e, const alga_nodes *nodes, const alga_edge *d_edges, uint64_t n_edges, int32_t flags, void *hip_stream,
                                   alga_unitigs *out, alga_unitig_info *info) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    const auto t0 = std::chrono::steady_clock::now();
    if (info) *info = alga_unitig_info{};
    if (!nodes || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes and out must not be NULL");
    if (flags & ~ALGA_UNITIG_SKIP_ISOLATED) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unknown unitig flag");
    if (nodes->n < 0 || (nodes->n & 1)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "the node count must be even (twin layout)");
    if ((nodes->n && (!nodes->len || !nodes->words || nodes->stride_words <= 0)) || (n_edges && !d_edges))
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad node set or edge list");
    if (n_edges && !nodes->n) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "edge endpoint outside [0, n)");
    if (n_edges >= (1ull << 31) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^31 edges");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    const int rc = unitigs_impl(e, nodes, (const alga_edge_dev *) d_edges, n_edges, flags, s, out, info);
    if (rc != ALGA_OK) { (void) hipStreamSynchronize(s); return rc; }
    if (info) info->ms_total = alga_ms_since(t0);
    return ALGA_OK;
}
