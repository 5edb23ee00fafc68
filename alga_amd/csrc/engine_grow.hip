// alga_amd/csrc/engine_grow.hip -- C ABI of the grow stage (include/alga_amd.h: alga_grow_placed_device, alga_write_grown_fasta_device;
// kernels in grow_kernels.hip).
//
// Host side: the check runs on a workspace and ends in one read-back (the refusal flags, the longest node).  Then, still on workspaces: the
// candidate flags, their scan and the list; W_e of every end and the scan; a read-back of the candidate count, the end columns and the indexed
// positions (they size the sort and the directory); the end sequences, the seed index over them (alga_seed_index).  The
// result is written into the set of buffers that does NOT hold the current result: k_gr_place, the votes, the decision, the new lengths; a
// read-back of the counters (the new column count sizes the result's bases, and is the last refusal); the scan and the build.  The sets are
// swapped at the end, so a call that is refused or fails anywhere leaves an earlier result as it was.  The lengths for the N50s come back only
// when `info` is given.  No step walks on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "engine_internal.h"
#include "correct_kernels.h"
#include "gfa_kernels.h"
#include "ingest_kernels.h"
#include "grow_kernels.h"

using namespace alga;

namespace {

int check_params(alga_engine *e, const alga_grow_params *p) {
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow parameters must not be NULL");
    if (p->k < 8 || p->k > 31) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow: k must be in [8, 31]");
    if (p->max_mismatches < 0 || p->max_mismatches > 254) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow: max_mismatches must be in [0, 254]");
    if (p->max_occ < 1 || p->max_occ > 65535) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow: max_occ must be in [1, 65535]");
    if (p->min_anchor < p->k || p->min_anchor > (1 << 20)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow: min_anchor must be in [k, 2^20]");
    if (p->min_cover < 1) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow: min_cover must be >= 1");
    if (p->min_percent < 51 || p->min_percent > 100) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow: min_percent must be in [51, 100]");
    if (p->max_grow < 1 || p->max_grow > 4096) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow: max_grow must be in [1, 4096]");
    if (p->flags || p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow: flags and reserved must be 0");
    return ALGA_OK;
}

int grow_impl(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_polished *pol, const alga_grow_params *p, hipStream_t s, alga_grown *out,
              alga_grow_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t R = (uint64_t) pl->n_reads, T = (uint64_t) pl->n_targets, C = pl->n_columns, G = (uint64_t) p->max_grow, E = 2 * T;
    if (E * G > (1ull << 30)) return alga_fail(e, ALGA_ERR_CAPACITY, "grow: 2 * n_targets * max_grow exceeds 2^30");
    int rc;
    AlgaEvents<4> evs;
    if ((rc = evs.create(e))) return rc;
    if ((rc = alga_ensure(e, e->gr_cnt, GR_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->gr_cnt.p, *hc = e->h_counters;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, GR_COUNTERS * sizeof(unsigned long long), s));
    const SeedReads rd{nodes->words, nodes->stride_words, nodes->len, R};
    const GrTargets tg{pl->d_col_off, (uint32_t) T, C, pol ? pol->d_words : (const uint32_t *) e->pl_cols.p, (uint32_t) e->opt_grow_max_blocks};

    // the check: nothing of the result is written before its verdict
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    if (R) {
        const CrReads c{const_cast<uint32_t *>(nodes->words), nodes->stride_words, nodes->len, R, p->k};
        launch_cr_twin(c, (uint32_t *) (cnt + GR_BAD_TWIN), s);
        if ((rc = alga_check_launch(e, "k_cr_twin"))) return rc;
    }
    launch_gr_check(rd, tg, cnt, s);
    if ((rc = alga_check_launch(e, "k_gr_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, GR_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[GR_BAD] & GR_BAD_COLUMNS) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow: n_columns is not the placement's col_off[n_targets]");
    if (hc[GR_BAD_TWIN] || (hc[GR_BAD] & GR_BAD_LEN))
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow: a row 2r is not the reverse complement of row 2r + 1, their lengths differ, or a length exceeds 16 * stride_words");
    const int64_t max_len = (int64_t) hc[GR_MAX_LEN];

    // workspaces: the candidates, the ends
    if ((rc = alga_ensure(e, e->gr_flag, (R + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->gr_pos, (R + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->gr_elen, (E + 2) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->gr_eoff, (E + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(std::max<uint64_t>(std::max(R, E), T) + 2)))) return rc;
    uint32_t *flag = (uint32_t *) e->gr_flag.p, *pos = (uint32_t *) e->gr_pos.p, *eoff = (uint32_t *) e->gr_eoff.p;
    int32_t *elen = (int32_t *) e->gr_elen.p;
    launch_gr_candidates(rd, pl->d_state, p->min_anchor, flag, tg.max_blocks, s);
    if ((rc = alga_check_launch(e, "k_gr_candidates"))) return rc;
    launch_exclusive_scan(flag, R + 1, pos, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(candidates)"))) return rc;
    launch_gr_end_lens(tg, (int32_t) std::min<int64_t>(max_len, 0x7FFFFFFF), p->k, elen, cnt, s);
    if ((rc = alga_check_launch(e, "k_gr_end_lens"))) return rc;
    launch_exclusive_scan((const uint32_t *) elen, E + 1, eoff, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(end lengths)"))) return rc;
    uint32_t *h_cand = (uint32_t *) (hc + GR_COUNTERS);
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, GR_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(h_cand, pos + R, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t n_cand = *h_cand, EC = hc[GR_END_COLUMNS], n_index = hc[GR_INDEX_POS];
    if (EC > 0xFFFFFFFEull) return alga_fail(e, ALGA_ERR_CAPACITY, "grow: the end sequences hold more than 2^32 - 2 bases");

    // the list, the end sequences, the index
    const size_t ec_words = (size_t) ((EC + 15) >> 4) + 2;
    const int blocks = std::min(seed_blocks(n_cand, e->n_cu), e->opt_grow_max_blocks);   // the scratch and its words per wave follow from the capped count
    const size_t ub_words = seed_scratch_words(blocks, max_len, p->k);
    if ((rc = alga_ensure(e, e->gr_cand, (n_cand + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->gr_ecols, ec_words * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->seed_ub, ub_words * sizeof(unsigned long long)))) return rc;
    uint32_t *cand = (uint32_t *) e->gr_cand.p, *ecols = (uint32_t *) e->gr_ecols.p;
    launch_gr_compact(flag, pos, R, cand, tg.max_blocks, s);
    if ((rc = alga_check_launch(e, "k_gr_compact"))) return rc;
    const GrEnds en{eoff, elen, (uint32_t) E, EC, ecols};
    HIP_TRY(e, hipMemsetAsync(ecols, 0, ec_words * sizeof(uint32_t), s));
    launch_gr_ends(tg, en, ecols, s);
    if ((rc = alga_check_launch(e, "k_gr_ends"))) return rc;
    SeedIndex ix;
    if ((rc = alga_seed_index(e, en, p->k, n_index, nullptr, s, &ix))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    // the result, into the set that is not the current one
    const int nxt = alga_other_set(e->gr_valid, e->gr_cur);
    alga_engine::GrowSet &rs = e->gr_set[nxt];
    const size_t count_bytes = (size_t) (E * G) * 4 * sizeof(uint32_t);
    for (DevBuf *b : {&rs.end, &rs.over}) if ((rc = alga_ensure(e, *b, (R + 1) * sizeof(int32_t)))) return rc;
    for (DevBuf *b : {&rs.mm, &rs.hits, &rs.state}) if ((rc = alga_ensure(e, *b, R + 16))) return rc;
    if ((rc = alga_ensure(e, rs.count, count_bytes + 16))) return rc;
    if ((rc = alga_ensure(e, rs.estop, E + 16))) return rc;
    if ((rc = alga_ensure(e, rs.evoters, (E + 2) * sizeof(uint32_t)))) return rc;
    for (DevBuf *b : {&rs.left, &rs.right, &rs.len, &rs.coloff}) if ((rc = alga_ensure(e, *b, (T + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, rs.begin, (T + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->gr_x, (E + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->gr_g, (size_t) (E * G) + 16))) return rc;
    const GrOut go{(int32_t *) rs.end.p, (int32_t *) rs.over.p, (uint8_t *) rs.mm.p, (uint8_t *) rs.hits.p, (uint8_t *) rs.state.p};
    uint32_t *count = (uint32_t *) rs.count.p, *voters = (uint32_t *) rs.evoters.p, *x = (uint32_t *) e->gr_x.p, *new_off = (uint32_t *) rs.coloff.p;
    HIP_TRY(e, hipMemsetAsync(go.end, 0xFF, (R + 1) * sizeof(int32_t), s));                       // -1: the read does not overhang
    HIP_TRY(e, hipMemsetAsync(go.over, 0, (R + 1) * sizeof(int32_t), s));
    for (uint8_t *b : {go.mm, go.hits, go.state}) HIP_TRY(e, hipMemsetAsync(b, 0, R + 16, s));
    HIP_TRY(e, hipMemsetAsync(count, 0, count_bytes + 16, s));
    HIP_TRY(e, hipMemsetAsync(voters, 0, (E + 2) * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(new_off, 0, (T + 2) * sizeof(uint32_t), s));
    launch_gr_place(rd, cand, n_cand, en, ix, p->k, p->max_mismatches, p->max_occ, p->min_anchor, go, (unsigned long long *) e->seed_ub.p,
                    (uint32_t) (ub_words / ((size_t) blocks * SEED_WAVES)), blocks, cnt, s);
    if ((rc = alga_check_launch(e, "k_gr_place"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));

    launch_gr_vote(rd, cand, n_cand, go, p->max_grow, count, voters, tg.max_blocks, s);
    if ((rc = alga_check_launch(e, "k_gr_vote"))) return rc;
    launch_gr_decide(count, voters, (uint32_t) E, p->max_grow, p->min_cover, p->min_percent, x, (uint8_t *) e->gr_g.p, (uint8_t *) rs.estop.p, cnt, tg.max_blocks, s);
    if ((rc = alga_check_launch(e, "k_gr_decide"))) return rc;
    launch_gr_lens(tg, x, (uint32_t *) rs.left.p, (uint32_t *) rs.right.p, (int32_t *) rs.len.p, cnt, s);
    if ((rc = alga_check_launch(e, "k_gr_lens"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, GR_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[GR_BAD_NEWLEN]) return alga_fail(e, ALGA_ERR_CAPACITY, "grow: a grown target is longer than 2^31 - 1");
    const uint64_t NC = hc[GR_COLUMNS_AFTER];
    if (NC > 0xFFFFFFFEull) return alga_fail(e, ALGA_ERR_CAPACITY, "grow: the grown targets hold more than 2^32 - 2 bases");
    const size_t new_words = (size_t) ((NC + 15) >> 4) + 2;
    if ((rc = alga_ensure(e, rs.words, new_words * sizeof(uint32_t)))) return rc;
    if (T) launch_exclusive_scan((const uint32_t *) rs.len.p, T + 1, new_off, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(new lengths)"))) return rc;
    launch_gr_build(tg, new_off, NC, (const uint32_t *) rs.left.p, (const uint8_t *) e->gr_g.p, p->max_grow, (uint32_t *) rs.words.p, (unsigned long long *) rs.begin.p, s);
    if ((rc = alga_check_launch(e, "k_gr_build"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[3], s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->gr_cur = nxt; e->gr_valid = true; e->gr_reads = R; e->gr_targets = T; e->gr_columns = NC; e->gr_longest = hc[GR_LONGEST];
    out->n_reads = (int64_t) R; out->n_targets = (int64_t) T; out->max_grow = (int64_t) G; out->n_columns = NC;
    out->d_end = go.end; out->d_over = go.over; out->d_mm = go.mm; out->d_hits = go.hits; out->d_state = go.state;
    out->d_count = count; out->d_e_stop = (const uint8_t *) rs.estop.p; out->d_e_voters = voters;
    out->d_left = (const uint32_t *) rs.left.p; out->d_right = (const uint32_t *) rs.right.p; out->d_len = (const int32_t *) rs.len.p; out->d_col_off = new_off;
    out->d_begin = (const uint64_t *) rs.begin.p; out->d_words = (const uint32_t *) rs.words.p;
    if (info) {
        alga_grow_info o{};
        o.candidates = n_cand; o.overhanging = hc[GR_OVERHANGING]; o.voting = hc[GR_VOTING]; o.multi = o.overhanging - o.voting; o.hits_saturated = hc[GR_SATURATED];
        o.seeds = hc[GR_SEEDS]; o.seeds_over_max_occ = hc[GR_SEEDS_OVER]; o.index_positions = n_index;
        o.ends_with_voters = hc[GR_ENDS_VOTERS]; o.ends_grown = hc[GR_ENDS_GROWN]; o.bases_added = hc[GR_ADDED]; o.longest_growth = hc[GR_LONGEST_GROWTH];
        o.stops_cover = hc[GR_STOPS_COVER]; o.stops_percent = hc[GR_STOPS_PERCENT]; o.stops_max = hc[GR_STOPS_MAX]; o.columns_before = C; o.columns_after = NC;
        // the lengths for the N50s (no exception leaves the C ABI: a host allocation that fails is reported like a device one)
        try {
            std::vector<uint32_t> off(T + 1), noff(T + 1);
            std::vector<uint64_t> before(T), after(T);
            HIP_TRY(e, hipMemcpyAsync(off.data(), pl->d_col_off, (T + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(e, hipMemcpyAsync(noff.data(), new_off, (T + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(e, hipStreamSynchronize(s));
            for (uint64_t t = 0; t < T; t++) { before[t] = off[t + 1] - off[t]; after[t] = noff[t + 1] - noff[t]; }
            o.n50_before = n50_of(std::move(before)); o.n50_after = n50_of(std::move(after));
        } catch (const std::bad_alloc &) {
            return alga_fail(e, ALGA_ERR_OUT_OF_MEMORY, "grow: no host memory for the lengths of the N50s");
        }
        if ((rc = evs.ms(e, 0, 1, &o.ms_index))) return rc;
        if ((rc = evs.ms(e, 1, 2, &o.ms_place))) return rc;
        if ((rc = evs.ms(e, 2, 3, &o.ms_build))) return rc;
        o.ms_total = alga_ms_since(t0);
        *info = o;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" void alga_grow_default_params(alga_grow_params *p) {
    if (!p) return;
    *p = alga_grow_params{};
    p->k = 21; p->max_mismatches = 2; p->max_occ = 256; p->min_anchor = 63; p->min_cover = 3; p->min_percent = 80; p->max_grow = 64; p->flags = 0;
}

extern "C" int alga_grow_placed_device(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_polished *pol, const alga_grow_params *p,
                                       void *hip_stream, alga_grown *out, alga_grow_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if (!nodes || !pl || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes, placements and out must not be NULL");
    if ((rc = alga_check_twin_nodes(e, nodes, true))) return rc;
    if (!alga_placement_is_current(e, pl)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last placement call on this engine");
    if ((int64_t) (nodes->n / 2) != pl->n_reads) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grow: the node set does not have the placement's reads (n / 2 != n_reads)");
    if (pol && !alga_polished_is_current(e, pl, pol))
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_polish_placed_device call on this placement");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return grow_impl(e, nodes, pl, pol, p, call.s, out, info);
}

extern "C" int alga_write_grown_fasta_device(alga_engine *e, const alga_grown *grown, const char *path, alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!grown || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "grown and path must not be NULL");
    const alga_engine::GrowSet &rs = e->gr_set[e->gr_cur];
    if (!e->gr_valid || grown->n_targets < 0 || (uint64_t) grown->n_targets != e->gr_targets || grown->n_columns != e->gr_columns ||
        grown->d_words != (const uint32_t *) rs.words.p || grown->d_col_off != (const uint32_t *) rs.coloff.p || grown->d_len != (const int32_t *) rs.len.p ||
        grown->d_left != (const uint32_t *) rs.left.p || grown->d_right != (const uint32_t *) rs.right.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_grow_placed_device call on this engine");
    if (e->gr_longest + 96 > 0xFFFFFFFFull) return alga_fail(e, ALGA_ERR_CAPACITY, "a contig record of more than 2^32 bytes");
    HIP_TRY(e, hipSetDevice(e->device));
    const GrFasta f{grown->d_words, grown->d_col_off, grown->d_len, grown->d_left, grown->d_right, (uint64_t) grown->n_targets,
                    e->opt_grow_max_blocks < 8192 ? (uint32_t) e->opt_grow_max_blocks : 16384u};   // the write grid's own cap unless a test lowers it
    return alga_text_records(e, f, launch_gr_fasta_sizes, launch_gr_fasta_write, path, info);
}
