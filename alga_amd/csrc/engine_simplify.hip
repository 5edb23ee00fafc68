// alga_amd/csrc/engine_simplify.hip -- C ABI of the simplifier steps: the triangle cut (simplify_kernels.hip), the removal of short parallel
// paths (mst_kernels.hip), the dangling-branch removal (tip_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>

#include "engine_internal.h"
#include "mst_kernels.h"
#include "simplify_kernels.h"
#include "tip_kernels.h"
#include "unitig_kernels.h"

using namespace alga;

namespace {

int cut_impl(alga_engine *e, int32_t n, const alga_edge_dev *d_in, uint64_t m, int32_t mopp, hipStream_t s, const alga_edge **d_out, uint64_t *m_out,
             uint64_t *removed) {
    int rc;
    if ((rc = alga_ensure(e, e->counters, (CNT_TOTAL + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->sp_rowptr, ((size_t) n + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->sp_sorted, (size_t) (m + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->sp_list, (size_t) (m + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->sp_cnt, ((size_t) n + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->sp_orow, ((size_t) n + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->sp_out, (size_t) (m + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes((uint64_t) n)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->counters.p;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), s));
    launch_edge_rowptr(d_in, m, n, (uint32_t *) e->sp_rowptr.p, s);
    if ((rc = alga_check_launch(e, "k_edge_rowptr"))) return rc;
    launch_cut_triangles(d_in, (const uint32_t *) e->sp_rowptr.p, n, mopp, (alga_edge_dev *) e->sp_sorted.p, (alga_edge_dev *) e->sp_list.p,
                         (uint32_t *) e->sp_cnt.p, cnt, s);
    if ((rc = alga_check_launch(e, "k_cut_triangles"))) return rc;
    launch_exclusive_scan((const uint32_t *) e->sp_cnt.p, (uint64_t) n, (uint32_t *) e->sp_orow.p, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(out_cnt)"))) return rc;
    launch_compact_rows((const alga_edge_dev *) e->sp_list.p, (const uint32_t *) e->sp_rowptr.p, (const uint32_t *) e->sp_cnt.p,
                        (const uint32_t *) e->sp_orow.p, n, (alga_edge_dev *) e->sp_out.p, s);
    if ((rc = alga_check_launch(e, "k_compact_rows"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    *removed = e->h_counters[0];
    *m_out = m - *removed;
    *d_out = (const alga_edge *) e->sp_out.p;
    return ALGA_OK;
}

// Host side of the dangling-branch removal: the graph once, then per iteration a down and an up pass and ONE read-back (the two counts of
// the iteration, which decide whether there is another one).
int tips_impl(alga_engine *e, int32_t n, const alga_edge_dev *d_in, uint64_t m, int32_t max_offset, hipStream_t s, const alga_edge **d_out, uint64_t *m_out,
              alga_tips_info *info) {
    int rc;
    AlgaEvents<3> evs;
    if ((rc = evs.create(e))) return rc;
    const size_t N = (size_t) n;
    if ((rc = alga_ensure(e, e->tp_cnt, (TIP_COUNTERS + UT_COUNTERS) * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->tp_cnt.p;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, (TIP_COUNTERS + UT_COUNTERS) * sizeof(unsigned long long), s));
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    launch_tip_check(d_in, m, n, cnt, s);
    if ((rc = alga_check_launch(e, "k_tip_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (const unsigned long long bad = e->h_counters[0])
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, (bad & TIP_BAD_ID) ? "edge endpoint outside [0, n)" : "negative edge offset");
    // the input is valid: from here on the previous result's buffer is rewritten
    for (int k = 0; k < 2; k++) {
        if ((rc = alga_ensure(e, e->tp_keys[k], (size_t) (m + 1) * sizeof(unsigned long long)))) return rc;
        if ((rc = alga_ensure(e, e->tp_vals[k], (size_t) (m + 1) * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->tp_rowptr[k], (N + 2) * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->tp_rec[k], (N + 1) * sizeof(TipRec)))) return rc;
    }
    if ((rc = alga_ensure(e, e->tp_flag, (size_t) (m + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->tp_pos, (size_t) (m + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->tp_best, (size_t) (m + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->tp_est, (size_t) (m + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->tp_rev, (size_t) (m + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->tp_rfid, (size_t) (m + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->tp_alive, (size_t) (m + 1)))) return rc;
    if ((rc = alga_ensure(e, e->tp_kill, (size_t) (m + 1)))) return rc;
    if ((rc = alga_ensure(e, e->tp_branch, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->tp_overflow, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->tp_out, (size_t) (m + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->sort_temp, sort_edges_temp_bytes(m)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(m)))) return rc;
    // the overflow route: 64 MB of workspaces of 5 words per node, at least one, at most 1024
    const int32_t n_ws = (int32_t) std::min<size_t>(std::max<size_t>((64u << 20) / (20 * (N + 1)), 1), 1024);
    if ((rc = alga_ensure(e, e->tp_ws, (size_t) n_ws * 5 * (N + 1) * sizeof(int32_t)))) return rc;
    unsigned long long *keys0 = (unsigned long long *) e->tp_keys[0].p, *keys1 = (unsigned long long *) e->tp_keys[1].p;
    uint32_t *vals0 = (uint32_t *) e->tp_vals[0].p, *vals1 = (uint32_t *) e->tp_vals[1].p;
    uint32_t *flag = (uint32_t *) e->tp_flag.p, *pos = (uint32_t *) e->tp_pos.p;
    alga_edge_dev *est = (alga_edge_dev *) e->tp_est.p, *rev = (alga_edge_dev *) e->tp_rev.p;
    uint8_t *alive = (uint8_t *) e->tp_alive.p, *kill = (uint8_t *) e->tp_kill.p;

    // ---- Graph::retainOnlySmallestOffset: the smallest offset per (src, dst), sorted; both CSR directions
    int node_bits = 1;
    while (node_bits < 31 && (1ll << node_bits) < (long long) n) node_bits++;
    launch_tip_keys(d_in, m, keys0, vals0, s);
    if ((rc = alga_check_launch(e, "k_tip_keys"))) return rc;
    HIP_TRY(e, sort_edges(e->sort_temp.p, sort_edges_temp_bytes(m), keys0, keys1, vals0, vals1, m, node_bits, s));
    launch_ut_group_heads(keys1, vals1, m, flag, (uint32_t *) e->tp_best.p, cnt + TIP_COUNTERS, s);
    if ((rc = alga_check_launch(e, "k_ut_group_heads"))) return rc;
    launch_exclusive_scan(flag, m, pos, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(group heads)"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, pos + m, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t ms = *(const uint32_t *) e->h_counters;
    launch_ut_compact_edges(keys1, flag, pos, (const uint32_t *) e->tp_best.p, m, est, s);
    if ((rc = alga_check_launch(e, "k_ut_compact_edges"))) return rc;
    launch_edge_rowptr(est, ms, n, (uint32_t *) e->tp_rowptr[0].p, s);
    launch_tip_rev_keys(est, ms, keys0, vals0, s);
    if ((rc = alga_check_launch(e, "k_tip_rev_keys"))) return rc;
    HIP_TRY(e, sort_edges(e->sort_temp.p, sort_edges_temp_bytes(m), keys0, keys1, vals0, vals1, ms, node_bits, s));
    launch_tip_rev_edges(keys1, vals1, est, ms, rev, (uint32_t *) e->tp_rfid.p, s);
    launch_edge_rowptr(rev, ms, n, (uint32_t *) e->tp_rowptr[1].p, s);
    if ((rc = alga_check_launch(e, "k_edge_rowptr"))) return rc;
    HIP_TRY(e, hipMemsetAsync(alive, 1, (size_t) ms + 1, s));
    HIP_TRY(e, hipMemsetAsync(kill, 0, (size_t) ms + 1, s));
    HIP_TRY(e, hipMemsetAsync(e->tp_ws.p, 0xFF, (size_t) n_ws * 5 * (N + 1) * sizeof(int32_t), s));
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    // ---- the loop of simplifyGraphOld
    const TipDir dirs[2] = {{est, (const uint32_t *) e->tp_rowptr[0].p, nullptr}, {rev, (const uint32_t *) e->tp_rowptr[1].p, (const uint32_t *) e->tp_rfid.p}};
    TipRec *rec[2] = {(TipRec *) e->tp_rec[0].p, (TipRec *) e->tp_rec[1].p};
    uint64_t removed_total = 0;
    int iterations = 0;
    for (int i = 0;; i++) {
        HIP_TRY(e, hipMemsetAsync(cnt + TIP_DOWN, 0, 2 * sizeof(unsigned long long), s));
        for (int dir = 0; dir < 2 && n > 0 && ms > 0; dir++) {
            HIP_TRY(e, hipMemsetAsync(cnt + TIP_N_BRANCH, 0, 2 * sizeof(unsigned long long), s));
            launch_tip_degrees(dirs[0], dirs[1], alive, n, dir, rec[0], rec[1], (int32_t *) e->tp_branch.p, cnt, s);
            if ((rc = alga_check_launch(e, "k_tip_degrees"))) return rc;
            const TipGraph g{dirs[dir].E, dirs[dir].rowptr, dirs[dir].fid, alive, rec[dir], rec[dir ^ 1]};
            launch_tip_find(g, (const int32_t *) e->tp_branch.p, n, max_offset, kill, (int32_t *) e->tp_overflow.p, cnt, s);
            if ((rc = alga_check_launch(e, "k_tip_find"))) return rc;
            launch_tip_find_overflow(g, (const int32_t *) e->tp_overflow.p, max_offset, kill, (int32_t *) e->tp_ws.p, n, n_ws, cnt, s);
            if ((rc = alga_check_launch(e, "k_tip_find_overflow"))) return rc;
            launch_tip_apply(alive, kill, ms, cnt + TIP_DOWN + dir, s);
            if ((rc = alga_check_launch(e, "k_tip_apply"))) return rc;
        }
        HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt + TIP_DOWN, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        const uint64_t down = e->h_counters[0], up = e->h_counters[1];
        if (info) {
            if (2 * i < ALGA_TIPS_MAX_PASSES) { info->removed[2 * i] = down; info->removed[2 * i + 1] = up; }
        }
        removed_total += down + up;
        iterations = i + 1;
        if (down + up == 0 || (i >= 15 && down + up <= 30)) break;      // src/GraphSimplifiers/GraphSimplifier.cpp:210-213
    }
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));

    // ---- the survivors, in (src, dst) order
    launch_tip_flags(alive, ms, flag, s);
    launch_exclusive_scan(flag, ms, pos, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(alive)"))) return rc;
    launch_tip_emit(est, flag, pos, ms, (alga_edge_dev *) e->tp_out.p, s);
    if ((rc = alga_check_launch(e, "k_tip_emit"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, TIP_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    *d_out = (const alga_edge *) e->tp_out.p;
    *m_out = ms - removed_total;
    if (info) {
        info->edges_in = m; info->edges_unique = ms; info->edges_out = ms - removed_total; info->iterations = iterations; info->passes = 2 * iterations;
        info->removed_total = removed_total; info->branching_nodes = e->h_counters[TIP_BRANCH_TOTAL]; info->overflow_nodes = e->h_counters[TIP_OVERFLOW_TOTAL];
        if ((rc = evs.ms(e, 0, 1, &info->ms_prepare))) return rc;
        if ((rc = evs.ms(e, 1, 2, &info->ms_passes))) return rc;
    }
    return ALGA_OK;
}

// Host side of the removal of short parallel paths: the mutable rows once, then per round claim, select, ONE read-back (the winners and
// the begs still pending, which decide whether there is a run and another round) and the run.
int mst_impl(alga_engine *e, int32_t n, const alga_edge_dev *d_in, uint64_t m, int32_t max_offset, hipStream_t s, const alga_edge **d_out, uint64_t *m_out,
             alga_mst_info *info) {
    int rc;
    AlgaEvents<3> evs;
    if ((rc = evs.create(e))) return rc;
    const size_t N = (size_t) n;
    if ((rc = alga_ensure(e, e->mp_cnt, MST_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->mp_cnt.p;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, MST_COUNTERS * sizeof(unsigned long long), s));
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    launch_mst_check(d_in, m, n, cnt, s);
    if ((rc = alga_check_launch(e, "k_mst_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (const unsigned long long bad = e->h_counters[0])
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, (bad & MST_BAD_ID) ? "edge endpoint outside [0, n)" : (bad & MST_BAD_OFFSET) ? "negative edge offset"
                                                                                                                                   : "edges must be grouped by src, in ascending order");
    // the input is valid: from here on the previous result's buffer is rewritten
    if ((rc = alga_ensure(e, e->mp_rowptr, (N + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->mp_rows, (size_t) (m + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->mp_len, (N + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->mp_owner, (N + 1) * sizeof(unsigned long long)))) return rc;
    for (int k = 0; k < 2; k++) if ((rc = alga_ensure(e, e->mp_pend[k], (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->mp_win, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->mp_overflow, (N + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->mp_orow, (N + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->mp_out, (size_t) (m + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes((uint64_t) n)))) return rc;
    if ((rc = alga_ensure(e, e->mp_overflow2, (N + 1) * sizeof(int32_t)))) return rc;
    // the overflow route: 1024 states of opt_mst_mid_nodes nodes and twice as many edges (180 MB), or fewer and smaller ones if that already holds
    // the whole graph; then, if it does not, states sized for the whole graph: 1 GB of them, at least one, at most 256.  They are allocated up
    // front (the cost is stated in the header): whether a beg needs one is known only inside a round, and the host reads one block of counts per round
    MstTiers tiers{};
    tiers.mid.cap_nodes = (uint32_t) std::min<uint64_t>((uint64_t) e->opt_mst_mid_nodes, (uint64_t) N + 1);
    tiers.mid.cap_edges = (uint32_t) std::min<uint64_t>(2 * (uint64_t) e->opt_mst_mid_nodes, m + 1);
    tiers.mid.hbits = mst_hbits_for(tiers.mid.cap_nodes);
    tiers.mid.n_ws = (int32_t) std::min<uint64_t>(1024, std::max<uint64_t>(N, 1));
    const bool need_big = (uint64_t) N + 1 > tiers.mid.cap_nodes || m + 1 > tiers.mid.cap_edges;
    if (need_big) {
        tiers.big.cap_nodes = (uint32_t) N + 1; tiers.big.cap_edges = (uint32_t) m + 1; tiers.big.hbits = mst_hbits_for((uint64_t) N + 1);
        tiers.big.n_ws = (int32_t) std::min<size_t>(std::max<size_t>(((size_t) 1 << 30) / (4 * mst_tier_words(tiers.big)), 1), 256);
    }
    const size_t mid_bytes = (size_t) tiers.mid.n_ws * mst_tier_words(tiers.mid) * sizeof(uint32_t);
    const size_t big_bytes = need_big ? (size_t) tiers.big.n_ws * mst_tier_words(tiers.big) * sizeof(uint32_t) : 0;
    if ((rc = alga_ensure(e, e->mp_ws, mid_bytes))) return rc;
    if (need_big && (rc = alga_ensure(e, e->mp_ws_big, big_bytes))) return rc;
    tiers.mid.ws = (uint32_t *) e->mp_ws.p;
    tiers.big.ws = need_big ? (uint32_t *) e->mp_ws_big.p : nullptr;
    alga_edge_dev *rows = (alga_edge_dev *) e->mp_rows.p;
    uint32_t *rowptr = (uint32_t *) e->mp_rowptr.p, *len = (uint32_t *) e->mp_len.p;
    int32_t *pend[2] = {(int32_t *) e->mp_pend[0].p, (int32_t *) e->mp_pend[1].p};

    if (m) HIP_TRY(e, hipMemcpyAsync(rows, d_in, (size_t) m * sizeof(alga_edge_dev), hipMemcpyDeviceToDevice, s));
    launch_edge_rowptr(d_in, m, n, rowptr, s);
    if ((rc = alga_check_launch(e, "k_edge_rowptr"))) return rc;
    launch_mst_init(rowptr, n, len, (unsigned long long *) e->mp_owner.p, pend[0], cnt, s);
    if ((rc = alga_check_launch(e, "k_mst_init"))) return rc;
    // the maps of the overflow states must be empty: every walk leaves them so (mst_clear), so a tier is filled only when its buffer or its geometry
    // is not the one of the last fill -- once per engine for the graphs of one size class, not per call.  Until this call has reached its end
    // the states count as unknown.
    const MstTier *tier_of[2] = {&tiers.mid, &tiers.big};
    const size_t tier_bytes[2] = {mid_bytes, big_bytes};
    for (int k = 0; k < (need_big ? 2 : 1); k++) {
        const MstTier &t = *tier_of[k];
        const alga_engine::MstFilled &f = e->mp_filled[k];
        if (f.p != t.ws || f.bytes != tier_bytes[k] || f.hbits != t.hbits || f.cap_nodes != t.cap_nodes || f.cap_edges != t.cap_edges || f.n_ws != t.n_ws)
            HIP_TRY(e, hipMemsetAsync(t.ws, 0xFF, tier_bytes[k], s));
        e->mp_filled[k].p = nullptr;
    }
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt + MST_N_PEND0, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));
    HIP_TRY(e, hipStreamSynchronize(s));
    uint64_t n_pend = e->h_counters[0];
    const uint64_t branching = n_pend;

    // ---- the rounds
    uint64_t rounds = 0, begs_run = 0;
    for (int cur = 0; n_pend > 0; cur ^= 1) {
        if (rounds >= 0xFFFFFFFEull) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 rounds");
        HIP_TRY(e, hipMemsetAsync(cnt + MST_N_WIN, 0, MST_ROUND_COUNTERS * sizeof(unsigned long long), s));   // winners and the overflow counts
        HIP_TRY(e, hipMemsetAsync(cnt + MST_N_PEND0 + (cur ^ 1), 0, sizeof(unsigned long long), s));
        const MstRound r{MstGraph{rows, rowptr, len}, (unsigned long long *) e->mp_owner.p, (unsigned long long) (0xFFFFFFFFull - rounds) << 32, max_offset,
                         (int32_t *) e->mp_win.p, pend[cur ^ 1], (int32_t *) e->mp_overflow.p, (int32_t *) e->mp_overflow2.p, cnt, cur ^ 1};
        launch_mst_claim(r, pend[cur], cur, n_pend, tiers, s);
        if ((rc = alga_check_launch(e, "k_mst_claim"))) return rc;
        launch_mst_select(r, pend[cur], cur, n_pend, tiers, s);
        if ((rc = alga_check_launch(e, "k_mst_select"))) return rc;
        HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, MST_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        const uint64_t n_win = e->h_counters[MST_N_WIN];
        n_pend = e->h_counters[MST_N_PEND0 + (cur ^ 1)];
        if (n_win == 0) break;                                       // nothing pending branches any more (the smallest that does always wins)
        launch_mst_run(r, n_win, tiers, s);
        if ((rc = alga_check_launch(e, "k_mst_run"))) return rc;
        if (info && rounds < ALGA_MST_MAX_ROUNDS) info->winners[rounds] = n_win;
        rounds++;
        begs_run += n_win;
    }
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));

    // ---- the rows, closed up
    launch_exclusive_scan(len, (uint64_t) n, (uint32_t *) e->mp_orow.p, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(len)"))) return rc;
    if (n > 0) launch_compact_rows(rows, rowptr, len, (const uint32_t *) e->mp_orow.p, n, (alga_edge_dev *) e->mp_out.p, s);
    if ((rc = alga_check_launch(e, "k_compact_rows"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, MST_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters + MST_COUNTERS, (const uint32_t *) e->mp_orow.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    *d_out = (const alga_edge *) e->mp_out.p;
    *m_out = n > 0 ? (uint64_t) *(const uint32_t *) (e->h_counters + MST_COUNTERS) : 0;
    for (int k = 0; k < (need_big ? 2 : 1); k++) e->mp_filled[k] = alga_engine::MstFilled{tier_of[k]->ws, tier_bytes[k], tier_of[k]->hbits, tier_of[k]->cap_nodes, tier_of[k]->cap_edges, tier_of[k]->n_ws};
    if (info) {
        info->edges_in = m; info->edges_out = *m_out; info->branching_nodes = branching; info->begs_run = begs_run; info->rounds = rounds;
        info->overflow_begs = e->h_counters[MST_OVERFLOW_TOTAL]; info->ball_max = e->h_counters[MST_BALL_MAX];
        if ((rc = evs.ms(e, 0, 1, &info->ms_prepare))) return rc;
        if ((rc = evs.ms(e, 1, 2, &info->ms_rounds))) return rc;
    }
    return ALGA_OK;
}

} // namespace

extern "C" {

int alga_remove_short_parallel_paths_device(alga_engine *e, int32_t n_nodes, const alga_edge *d_edges, uint64_t n_edges, int32_t max_offset, void *hip_stream,
                                            const alga_edge **d_edges_out, uint64_t *n_edges_out, alga_mst_info *info) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    const auto t0 = std::chrono::steady_clock::now();
    if (info) *info = alga_mst_info{};
    if (!d_edges_out || !n_edges_out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *d_edges_out = nullptr; *n_edges_out = 0;
    if (n_nodes < 0 || (n_edges && !d_edges)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad graph");
    if (n_edges && !n_nodes) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "edge endpoint outside [0, n)");
    if (n_edges >= (1ull << 31) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^31 edges");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    const int rc = mst_impl(e, n_nodes, (const alga_edge_dev *) d_edges, n_edges, max_offset, s, d_edges_out, n_edges_out, info);
    if (rc != ALGA_OK) { (void) hipStreamSynchronize(s); if (info) *info = alga_mst_info{}; *d_edges_out = nullptr; *n_edges_out = 0; return rc; }
    if (info) info->ms_total = alga_ms_since(t0);
    return ALGA_OK;
}

int alga_remove_dangling_branches_device(alga_engine *e, int32_t n_nodes, const alga_edge *d_edges, uint64_t n_edges, int32_t max_offset, void *hip_stream,
                                         const alga_edge **d_edges_out, uint64_t *n_edges_out, alga_tips_info *info) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    const auto t0 = std::chrono::steady_clock::now();
    if (info) *info = alga_tips_info{};
    if (!d_edges_out || !n_edges_out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *d_edges_out = nullptr; *n_edges_out = 0;
    if (n_nodes < 0 || (n_edges && !d_edges)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad graph");
    if (n_edges && !n_nodes) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "edge endpoint outside [0, n)");
    if (n_edges >= (1ull << 31) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^31 edges");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    const int rc = tips_impl(e, n_nodes, (const alga_edge_dev *) d_edges, n_edges, max_offset, s, d_edges_out, n_edges_out, info);
    if (rc != ALGA_OK) { (void) hipStreamSynchronize(s); if (info) *info = alga_tips_info{}; return rc; }
    if (info) info->ms_total = alga_ms_since(t0);
    return ALGA_OK;
}

int alga_cut_triangles_device(alga_engine *e, int32_t n_nodes, const alga_edge *d_edges, uint64_t n_edges, int32_t max_offset_parallel_paths,
                              void *hip_stream, const alga_edge **d_edges_out, uint64_t *n_edges_out, uint64_t *n_removed) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!d_edges_out || !n_edges_out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *d_edges_out = nullptr; *n_edges_out = 0;
    if (n_nodes < 0 || (n_edges && !d_edges)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad graph");
    if (n_edges >= (1ull << 32) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 edges");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    uint64_t removed = 0;
    int rc = cut_impl(e, n_nodes, (const alga_edge_dev *) d_edges, n_edges, max_offset_parallel_paths, s, d_edges_out, n_edges_out, &removed);
    if (rc == ALGA_OK && n_removed) *n_removed = removed;
    return rc;
}

int alga_cut_triangles_host(alga_engine *e, int32_t n_nodes, const alga_edge *edges, uint64_t n_edges, int32_t max_offset_parallel_paths,
                            alga_edge **edges_out, uint64_t *n_edges_out) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!edges_out || !n_edges_out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *edges_out = nullptr; *n_edges_out = 0;
    if (n_nodes < 0 || (n_edges && !edges)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad graph");
    for (uint64_t k = 0; k < n_edges; k++) {
        if (edges[k].src < 0 || edges[k].src >= n_nodes || edges[k].dst < 0 || edges[k].dst >= n_nodes) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "edge endpoint out of range");
        if (k && (edges[k - 1].src > edges[k].src || (edges[k - 1].src == edges[k].src && edges[k - 1].dst > edges[k].dst)))
            return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "edges must be sorted by (src, dst)");
    }
    HIP_TRY(e, hipSetDevice(e->device));
    int rc;
    if ((rc = alga_ensure(e, e->sp_in, (size_t) (n_edges + 1) * sizeof(alga_edge)))) return rc;
    if ((rc = alga_staged_h2d(e, e->sp_in.p, edges, (size_t) n_edges * sizeof(alga_edge)))) return rc;
    const alga_edge *d_out = nullptr;
    uint64_t m = 0, removed = 0;
    if ((rc = cut_impl(e, n_nodes, (const alga_edge_dev *) e->sp_in.p, n_edges, max_offset_parallel_paths, e->own_stream, &d_out, &m, &removed))) return rc;
    alga_edge *h = (alga_edge *) alga_host_list_take(e, (size_t) (m ? m : 1) * sizeof(alga_edge));
    if (!h) return alga_fail(e, ALGA_ERR_OUT_OF_MEMORY, "host edge buffer");
    if (m && (rc = alga_staged_d2h(e, h, d_out, (size_t) m * sizeof(alga_edge)))) { alga_host_list_give(e, h); return rc; }
    *edges_out = h; *n_edges_out = m;
    return ALGA_OK;
}

int alga_contig_trim_host(alga_engine *e, const uint32_t *words, int32_t stride_words, const int32_t *len, int32_t n_contigs, int32_t threshold,
                          int32_t *trim_left) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (n_contigs < 0 || (n_contigs && (!words || !len || !trim_left || stride_words <= 0))) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad contig arrays");
    if (threshold < 1 || threshold > 501) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "threshold must be in [1, 501]");
    if (n_contigs == 0) return ALGA_OK;
    if (n_contigs > 0x3FFFFFFF) return alga_fail(e, ALGA_ERR_CAPACITY, "too many contigs");
    const size_t M = (size_t) n_contigs;
    int32_t max_len = 0;
    for (size_t i = 0; i < M; i++) { if (len[i] < 0) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "negative contig length"); max_len = std::max(max_len, len[i]); }
    if ((int64_t) blocks_of(max_len) > (int64_t) stride_words) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stride_words is smaller than the longest contig needs");
    const size_t row_bytes = (size_t) stride_words * sizeof(uint32_t);
    if (2 * M * row_bytes > (64ull << 30)) return alga_fail(e, ALGA_ERR_CAPACITY, "contig rows at one fixed stride would take more than 64 GB: trim on the host");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = e->own_stream;
    int rc;
    // nodes as src/main.cpp:636-645 numbers them: contigs 0 .. M-1, then their reverse complements M .. 2M-1
    alga_forget_node_set(e);
    if ((rc = alga_ensure(e, e->up_words, 2 * M * row_bytes))) return rc;
    if ((rc = alga_ensure(e, e->up_len, 2 * M * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->sp_cnt, (M + 2) * sizeof(int32_t)))) return rc;
    HIP_TRY(e, hipStreamSynchronize(s));
    if ((rc = alga_staged_h2d(e, e->up_words.p, words, M * row_bytes))) return rc;
    if ((rc = alga_staged_h2d(e, e->up_len.p, len, M * sizeof(int32_t)))) return rc;
    launch_revcomp_rows((uint32_t *) e->up_words.p, stride_words, (int32_t *) e->up_len.p, n_contigs, s);
    if ((rc = alga_check_launch(e, "k_revcomp_rows"))) return rc;
    alga_nodes nd{(const uint32_t *) e->up_words.p, stride_words, (const int32_t *) e->up_len.p, 2 * n_contigs, nullptr, nullptr};
    alga_prefsuf_params p;
    alga_prefsuf_default_params(&p);
    p.min_overlap = threshold;                             // src/main.cpp:651-653
    p.rsoe_min_overlap = threshold;
    const alga_edge *d_edges = nullptr;
    uint64_t m = 0;
    if ((rc = alga_prefsuf_build_device(e, &nd, &p, (void *) s, &d_edges, &m))) return rc;
    // the reference does not call retainOnlySmallestOffset after this creator run; the largest overlap into a contig is the
    // smallest offset of its (source, contig) pair, which that call keeps: trimLeft is the same either way
    HIP_TRY(e, hipMemsetAsync(e->sp_cnt.p, 0, (M + 2) * sizeof(int32_t), s));
    launch_trim_left((const alga_edge_dev *) d_edges, m, (const int32_t *) e->up_len.p, n_contigs, (int32_t *) e->sp_cnt.p, s);
    if ((rc = alga_check_launch(e, "k_trim_left"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(trim_left, e->sp_cnt.p, M * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return ALGA_OK;
}

} // extern "C"
