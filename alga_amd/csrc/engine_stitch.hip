// alga_amd/csrc/engine_stitch.hip -- C ABI of the stitch stage (include/alga_amd.h: alga_stitch_targets_device, alga_stitch_scaffolds_device,
// alga_write_stitched_fasta_device; kernels in stitch_kernels.hip, and from the joins on the merge stage's in merge_kernels.hip).
//
// Host side: the checks (the merge stage's over the lengths, k_st_check over the selected entries) run on workspaces and on the set of result
// buffers that does NOT hold the current result, and end in one read-back (the refusal flags, the column sum).  Then k_st_overlap, the joins,
// and the merge stage's path as it is (alga_merge_tail): cycles, ranks, places, layout; a read-back of the counters (the stitched contigs, their
// members and columns size what follows, and the longest stitched contig is the last refusal); the scan and the build.  The sets are swapped at
// the end, so a call that is refused or fails anywhere leaves an earlier result as it was, and a call may take its targets from that result.
// The lengths for the N50s come back only when `info` is given.  No step walks on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "engine_internal.h"
#include "gfa_kernels.h"
#include "ingest_kernels.h"
#include "stitch_kernels.h"

using namespace alga;

namespace {

int check_params(alga_engine *e, const alga_stitch_params *p) {
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stitch parameters must not be NULL");
    if (p->max_mismatches < 0 || p->max_mismatches > 254) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stitch: max_mismatches must be in [0, 254]");
    if (p->max_overlap > ST_MAX_OVERLAP) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stitch: max_overlap must be at most 4096");
    if (p->min_overlap < 8 || p->min_overlap > p->max_overlap) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stitch: min_overlap must be in [8, max_overlap]");
    if (p->slack < 0 || p->slack > (1 << 20)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stitch: slack must be in [0, 2^20]");
    if (p->flags || p->reserved[0] || p->reserved[1] || p->reserved[2]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stitch: flags and reserved must be 0");
    return ALGA_OK;
}

int stitch_impl(alga_engine *e, const uint32_t *d_words, const unsigned long long *d_begin, const int32_t *d_len, uint64_t T, const StEntries &en,
                const alga_stitch_params *p, hipStream_t s, std::chrono::steady_clock::time_point t0, alga_stitched *out, alga_stitch_info *info) {
    const uint64_t E = 2 * T, J = en.J;
    int rc;
    AlgaEvents<3> evs;
    if ((rc = evs.create(e))) return rc;
    if ((rc = alga_ensure(e, e->st_cnt, ST_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->st_cnt.p, *hc = e->h_counters;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, ST_COUNTERS * sizeof(unsigned long long), s));
    const MgTargets tg{d_words, d_begin, d_len, (uint32_t) T, (uint32_t) e->opt_stitch_max_blocks};

    // the checks: nothing of the current result is written, the set they write is the other one
    const int nxt = alga_other_set(e->st_valid, e->st_cur);
    alga_engine::StitchSet &rs = e->st_set[nxt];
    if ((rc = alga_ensure(e, e->st_endcnt, (E + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, rs.endentry, (E + 2) * sizeof(int32_t)))) return rc;
    uint32_t *end_count = (uint32_t *) e->st_endcnt.p;
    int32_t *end_entry = (int32_t *) rs.endentry.p;
    HIP_TRY(e, hipMemsetAsync(end_count, 0, (E + 2) * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(end_entry, 0xFF, (E + 2) * sizeof(int32_t), s));
    launch_mg_check(tg, cnt, s);
    if ((rc = alga_check_launch(e, "k_mg_check"))) return rc;
    launch_st_check(en, (uint32_t) T, end_count, end_entry, cnt, tg.max_blocks, s);
    if ((rc = alga_check_launch(e, "k_st_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, ST_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[MG_BAD] & MG_BAD_LEN) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stitch: negative target length");
    if (hc[ST_BAD] & ST_BAD_END) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stitch: a selected entry names an end that is not below 2 * n_targets");
    if (hc[ST_BAD] & ST_BAD_SAME_TARGET) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stitch: a selected entry names two ends of one target");
    if (hc[ST_BAD] & ST_BAD_END_TWICE) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stitch: an end is named by more than one selected entry");
    const uint64_t C = hc[MG_COLUMNS], n_selected = hc[ST_SELECTED];
    if (C > 0xFFFFFFFEull) return alga_fail(e, ALGA_ERR_CAPACITY, "stitch: the targets hold more than 2^32 - 2 bases");

    // the result, into the set that is not the current one
    if ((rc = alga_ensure(e, rs.jolen, (J + 2) * sizeof(int32_t)))) return rc;
    for (DevBuf *b : {&rs.jmm, &rs.jhits, &rs.jstate}) if ((rc = alga_ensure(e, *b, J + 16))) return rc;
    for (DevBuf *b : {&e->st_epartner, &e->st_eolen}) if ((rc = alga_ensure(e, *b, (E + 2) * sizeof(int32_t)))) return rc;
    for (DevBuf *b : {&e->st_emm, &e->st_ehits, &e->st_estate}) if ((rc = alga_ensure(e, *b, E + 16))) return rc;
    for (DevBuf *b : {&rs.stitched, &rs.rank, &rs.start, &rs.ovafter, &rs.soff, &rs.smembers, &rs.len, &rs.coloff}) if ((rc = alga_ensure(e, *b, (T + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, rs.orient, T + 16))) return rc;
    if ((rc = alga_ensure(e, rs.begin, (T + 2) * sizeof(unsigned long long)))) return rc;
    ChainWork w;
    if ((rc = alga_chain_work(e, T, &w))) return rc;
    const StEntryOut jo{(int32_t *) rs.jolen.p, (uint8_t *) rs.jmm.p, (uint8_t *) rs.jhits.p, (uint8_t *) rs.jstate.p};
    const MgEndOut eo{(int32_t *) e->st_epartner.p, (int32_t *) e->st_eolen.p, (uint8_t *) e->st_emm.p, (uint8_t *) e->st_ehits.p, (uint8_t *) e->st_estate.p};
    uint32_t *col_off = (uint32_t *) rs.coloff.p;
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    launch_st_overlap(tg, en, StParams{p->max_mismatches, p->min_overlap, p->max_overlap, p->slack}, jo, cnt, s);
    if ((rc = alga_check_launch(e, "k_st_overlap"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    launch_st_joins(en, jo, end_entry, (uint32_t) E, eo, w.join, tg.max_blocks, s);
    if ((rc = alga_check_launch(e, "k_st_joins"))) return rc;
    const MgLayout lo{(int32_t *) rs.stitched.p, (int32_t *) rs.rank.p, (uint8_t *) rs.orient.p, (uint32_t *) rs.start.p, (int32_t *) rs.ovafter.p, (uint32_t *) rs.soff.p,
                      (int32_t *) rs.smembers.p, (int32_t *) rs.len.p};
    // the merge stage's path from here on; a stitch the cycles lost is turned into DROPPED_CYCLE between the drop and the ranks
    const auto dropped = [&]() { launch_st_dropped(en, w.join, jo.state, tg.max_blocks, s); return alga_check_launch(e, "k_st_dropped"); };
    if ((rc = alga_merge_tail(e, tg, eo, w, lo, col_off, rs.words, (unsigned long long *) rs.begin.p, cnt, ST_COUNTERS, "stitch", "stitched", dropped, s))) return rc;
    const uint64_t NS = hc[MG_MERGED], NC = hc[MG_COLUMNS_AFTER];
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->st_cur = nxt; e->st_valid = true; e->st_targets = T; e->st_entries = J; e->st_stitched = NS; e->st_columns = NC; e->st_longest = hc[MG_LONGEST];
    out->n_targets = (int64_t) T; out->n_entries = (int64_t) J; out->n_stitched = (int64_t) NS; out->n_members = (int64_t) hc[MG_MEMBERS]; out->n_columns = NC;
    out->d_j_olen = jo.olen; out->d_j_mm = jo.mm; out->d_j_hits = jo.hits; out->d_j_state = jo.state; out->d_end_entry = end_entry;
    out->d_stitched = lo.merged; out->d_rank = lo.rank; out->d_orient = lo.orient; out->d_start = lo.start; out->d_overlap_after = lo.overlap_after;
    out->d_s_off = lo.m_off; out->d_s_members = lo.m_members;
    out->d_len = lo.m_len; out->d_col_off = col_off; out->d_begin = (const uint64_t *) rs.begin.p; out->d_words = (const uint32_t *) rs.words.p;
    if (info) {
        alga_stitch_info o{};
        o.entries = J; o.selected = n_selected; o.with_overlap = hc[ST_WITH_OVERLAP]; o.ambiguous = hc[ST_AMBIGUOUS]; o.hits_saturated = hc[ST_SATURATED];
        o.candidates_outside_slack = hc[ST_OUTSIDE_SLACK];
        o.stitched = hc[MG_JOINS]; o.dropped_cycle = hc[MG_DROPPED]; o.join_mismatches = hc[MG_JOIN_MM]; o.bases_removed = hc[MG_REMOVED]; o.longest_overlap = hc[MG_LONGEST_OVERLAP];
        o.contigs = NS; o.contigs_multi = hc[MG_MULTI]; o.longest = hc[MG_LONGEST]; o.columns_before = C; o.columns_after = NC;
        // the lengths for the N50s (no exception leaves the C ABI: a host allocation that fails is reported like a device one)
        try {
            std::vector<int32_t> tl(T), ml(NS);
            if (T) HIP_TRY(e, hipMemcpyAsync(tl.data(), d_len, T * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            if (NS) HIP_TRY(e, hipMemcpyAsync(ml.data(), lo.m_len, NS * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(e, hipStreamSynchronize(s));
            o.n50_before = n50_of(std::vector<uint64_t>(tl.begin(), tl.end())); o.n50_after = n50_of(std::vector<uint64_t>(ml.begin(), ml.end()));
        } catch (const std::bad_alloc &) {
            return alga_fail(e, ALGA_ERR_OUT_OF_MEMORY, "stitch: no host memory for the lengths of the N50s");
        }
        if ((rc = evs.ms(e, 0, 1, &o.ms_overlap))) return rc;
        if ((rc = evs.ms(e, 1, 2, &o.ms_build))) return rc;
        o.ms_total = alga_ms_since(t0);
        *info = o;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" void alga_stitch_default_params(alga_stitch_params *p) {
    if (!p) return;
    *p = alga_stitch_params{};
    p->max_mismatches = 2; p->min_overlap = 16; p->max_overlap = 512; p->slack = 1 << 20; p->flags = 0;
}

extern "C" int alga_stitch_targets_device(alga_engine *e, const uint32_t *d_words, const uint64_t *d_begin, const int32_t *d_len, int32_t n_targets,
                                          const uint32_t *d_j_a, const uint32_t *d_j_b, const int32_t *d_j_gap, const uint8_t *d_j_state, int64_t n_entries,
                                          const alga_stitch_params *p, void *hip_stream, alga_stitched *out, alga_stitch_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if (!out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "out must not be NULL");
    if (n_targets < 0 || (n_targets && (!d_words || !d_begin || !d_len))) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad target arrays");
    if (n_entries < 0 || (n_entries && (!d_j_a || !d_j_b || !d_j_gap))) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad entry arrays");
    if (n_targets > (1 << 30)) return alga_fail(e, ALGA_ERR_CAPACITY, "stitch: more than 2^30 targets");
    if (n_entries > 0x7FFFFFFFll) return alga_fail(e, ALGA_ERR_CAPACITY, "stitch: more than 2^31 - 1 entries");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return stitch_impl(e, d_words, (const unsigned long long *) d_begin, d_len, (uint64_t) n_targets, StEntries{d_j_a, d_j_b, d_j_gap, d_j_state, (uint32_t) n_entries}, p,
                       call.s, t0, out, info);
}

extern "C" int alga_stitch_scaffolds_device(alga_engine *e, const alga_placements *pl, const alga_scaffolds *scaf, const alga_polished *pol, const alga_stitch_params *p,
                                            void *hip_stream, alga_stitched *out, alga_stitch_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if (!pl || !scaf || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "placements, scaffolds and out must not be NULL");
    if (!alga_placement_is_current(e, pl)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last placement call on this engine");
    if (!e->sc_valid || e->sc_pl_serial != e->pl_serial || scaf->n_targets < 0 || (uint64_t) scaf->n_targets != e->sc_targets || e->sc_targets != e->pl_targets ||
        scaf->n_scaffolds < 0 || (uint64_t) scaf->n_scaffolds != e->sc_scaffolds || scaf->d_s_off != (const uint32_t *) e->sc_soff.p ||
        scaf->d_s_members != (const int32_t *) e->sc_smembers.p || scaf->d_s_len != (const uint64_t *) e->sc_slen.p || scaf->d_start != (const uint64_t *) e->sc_start.p ||
        scaf->d_orient != (const uint8_t *) e->sc_orient.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_scaffold_placed_device call on this placement");
    if (pol && !alga_polished_is_current(e, pl, pol))
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_polish_placed_device call on this placement");
    if (scaf->n_bundles < 0 || scaf->d_b_a != (const uint32_t *) e->sc_ba.p || scaf->d_b_b != (const uint32_t *) e->sc_bb.p || scaf->d_b_gap != (const int32_t *) e->sc_bgap.p ||
        scaf->d_b_state != (const uint8_t *) e->sc_bstate.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the bundles of the last alga_scaffold_placed_device call on this placement");
    if (scaf->n_bundles > 0x7FFFFFFFll) return alga_fail(e, ALGA_ERR_CAPACITY, "stitch: more than 2^31 - 1 entries");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    // the placement's targets as a ragged set: begin = col_off, the lengths from col_off (n_targets <= 2^30, n_columns <= 2^32 - 2: the placement's own bounds)
    const uint64_t T = (uint64_t) pl->n_targets;
    if ((rc = alga_ensure(e, e->st_tbegin, (T + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->st_tlen, (T + 2) * sizeof(int32_t)))) return rc;
    launch_st_targets(pl->d_col_off, (uint32_t) T, (unsigned long long *) e->st_tbegin.p, (int32_t *) e->st_tlen.p, (uint32_t) e->opt_stitch_max_blocks, call.s);
    if ((rc = alga_check_launch(e, "k_st_targets"))) return rc;
    return stitch_impl(e, pol ? pol->d_words : (const uint32_t *) e->pl_cols.p, (const unsigned long long *) e->st_tbegin.p, (const int32_t *) e->st_tlen.p, T,
                       StEntries{scaf->d_b_a, scaf->d_b_b, scaf->d_b_gap, scaf->d_b_state, (uint32_t) scaf->n_bundles}, p, call.s, t0, out, info);
}

extern "C" int alga_write_stitched_fasta_device(alga_engine *e, const alga_stitched *st, const char *path, alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!st || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stitched and path must not be NULL");
    const alga_engine::StitchSet &rs = e->st_set[e->st_cur];
    if (!e->st_valid || st->n_targets < 0 || (uint64_t) st->n_targets != e->st_targets || st->n_stitched < 0 || (uint64_t) st->n_stitched != e->st_stitched ||
        st->n_columns != e->st_columns || st->d_words != (const uint32_t *) rs.words.p || st->d_col_off != (const uint32_t *) rs.coloff.p ||
        st->d_len != (const int32_t *) rs.len.p || st->d_s_off != (const uint32_t *) rs.soff.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last stitch call on this engine");
    if (e->st_longest + 96 > 0xFFFFFFFFull) return alga_fail(e, ALGA_ERR_CAPACITY, "a contig record of more than 2^32 bytes");
    HIP_TRY(e, hipSetDevice(e->device));
    const MgFasta f{st->d_words, st->d_col_off, st->d_s_off, st->d_len, (uint64_t) st->n_stitched};
    return alga_text_records(e, f, launch_mg_fasta_sizes, launch_mg_fasta_write, path, info);
}
