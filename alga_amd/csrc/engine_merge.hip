// alga_amd/csrc/engine_merge.hip -- C ABI of the merge stage (include/alga_amd.h: alga_merge_targets_device, alga_write_merged_fasta_device;
// kernels in merge_kernels.hip).
//
// Host side: the check runs on a workspace and ends in one read-back (the refusal flag, the column sum).  Then, still on workspaces: W_x of
// every end and the scan; a read-back of the end columns and the indexed positions (they size the sort and the directory); the end sequences,
// the seed index over them (alga_seed_index).  The result is written into the set of buffers that does NOT hold the
// current result: k_mg_overlap, the joins, the cycles, the ranks, the layout; a read-back of the counters (the merged contigs, their members and
// columns size what follows, and the longest merged contig is the last refusal); the scan and the build.  The sets are swapped at the end, so a
// call that is refused or fails anywhere leaves an earlier result as it was, and a call may take its targets from that result.  The lengths
// for the N50s come back only when `info` is given.  No step walks on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "engine_internal.h"
#include "gfa_kernels.h"
#include "ingest_kernels.h"
#include "merge_kernels.h"

using namespace alga;

int alga_merge_tail(alga_engine *e, const MgTargets &tg, const MgEndOut &eo, const ChainWork &w, const MgLayout &lo, uint32_t *col_off, DevBuf &words, unsigned long long *begin,
                    unsigned long long *cnt, size_t n_counters, const char *stage, const char *noun, const std::function<int()> &after_drop, hipStream_t s) {
    const uint64_t T = tg.T, E = 2 * T;
    const std::string nn(noun);
    unsigned long long *hc = e->h_counters;
    int rc;
    // the joins into paths (the chain core, chain_kernels.h)
    const ChainLists *l;
    if ((rc = alga_chain_cycles(e, w, w.join, E, true, tg.max_blocks, s, &l))) return rc;
    launch_mg_cycle_drop(*l, (uint32_t) T, w.join, eo.state, cnt, tg.max_blocks, s);
    if ((rc = alga_check_launch(e, "k_mg_cycle_drop"))) return rc;
    if (after_drop && (rc = after_drop())) return rc;
    launch_mg_rank_init(tg, w.join, eo.olen, w.set[0], s);
    if ((rc = alga_chain_ranks(e, w, E, true, tg.max_blocks, s, &l))) return rc;

    HIP_TRY(e, hipMemsetAsync(lo.m_len, 0, (T + 2) * sizeof(int32_t), s));
    HIP_TRY(e, hipMemsetAsync(col_off, 0, (T + 2) * sizeof(uint32_t), s));
    launch_mg_place(tg, *l, w.join, eo, lo, w.head, w.first, w.members, cnt, s);
    if ((rc = alga_check_launch(e, "k_mg_place"))) return rc;
    if ((rc = alga_chain_scans(e, w, T, ("scan(" + nn + " contigs)").c_str(), s))) return rc;
    launch_mg_layout(tg, *l, w.head, w.first_scan, w.members_scan, lo, cnt, s);
    if ((rc = alga_check_launch(e, "k_mg_layout"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[MG_BAD_MERGED_LEN]) return alga_fail(e, ALGA_ERR_CAPACITY, (std::string(stage) + ": a " + nn + " contig is longer than 2^31 - 1").c_str());
    const uint64_t NM = hc[MG_MERGED], NC = hc[MG_COLUMNS_AFTER];
    const size_t new_words = (size_t) ((NC + 15) >> 4) + 2;
    if ((rc = alga_ensure(e, words, new_words * sizeof(uint32_t)))) return rc;
    if (NM) launch_exclusive_scan((const uint32_t *) lo.m_len, NM + 1, col_off, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, ("scan(" + nn + " lengths)").c_str()))) return rc;
    launch_mg_build(tg, lo, col_off, (uint32_t) NM, NC, (uint32_t *) words.p, begin, s);
    return alga_check_launch(e, "k_mg_build");
}

namespace {

int check_params(alga_engine *e, const alga_merge_params *p) {
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "merge parameters must not be NULL");
    if (p->k < 8 || p->k > 31) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "merge: k must be in [8, 31]");
    if (p->max_mismatches < 0 || p->max_mismatches > 254) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "merge: max_mismatches must be in [0, 254]");
    if (p->max_occ < 1 || p->max_occ > 65535) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "merge: max_occ must be in [1, 65535]");
    if (p->max_overlap > std::min(MG_MAX_OVERLAP, 64 * p->k)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "merge: max_overlap must be at most min(4096, 64 k)");
    if (p->min_overlap < p->k || p->min_overlap > p->max_overlap) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "merge: min_overlap must be in [k, max_overlap]");
    if (p->flags || p->reserved[0] || p->reserved[1]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "merge: flags and reserved must be 0");
    return ALGA_OK;
}

int merge_impl(alga_engine *e, const uint32_t *d_words, const unsigned long long *d_begin, const int32_t *d_len, int32_t n_targets, const alga_merge_params *p, hipStream_t s,
               alga_merged *out, alga_merge_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t T = (uint64_t) n_targets, E = 2 * T;
    int rc;
    AlgaEvents<4> evs;
    if ((rc = evs.create(e))) return rc;
    if ((rc = alga_ensure(e, e->mg_cnt, MG_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->mg_cnt.p, *hc = e->h_counters;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, MG_COUNTERS * sizeof(unsigned long long), s));
    const MgTargets tg{d_words, d_begin, d_len, (uint32_t) T, (uint32_t) e->opt_merge_max_blocks};

    // the check: nothing of the result is written before its verdict
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    launch_mg_check(tg, cnt, s);
    if ((rc = alga_check_launch(e, "k_mg_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, MG_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[MG_BAD] & MG_BAD_LEN) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "merge: negative target length");
    const uint64_t C = hc[MG_COLUMNS];
    if (C > 0xFFFFFFFEull) return alga_fail(e, ALGA_ERR_CAPACITY, "merge: the targets hold more than 2^32 - 2 bases");

    // workspaces: the ends
    if ((rc = alga_ensure(e, e->mg_elen, (E + 2) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->mg_epad, (E + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->mg_eoff, (E + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(E + 2)))) return rc;
    int32_t *elen = (int32_t *) e->mg_elen.p;
    uint32_t *epad = (uint32_t *) e->mg_epad.p, *eoff = (uint32_t *) e->mg_eoff.p;
    launch_mg_end_lens(tg, p->max_overlap, p->min_overlap, p->k, elen, epad, cnt, s);
    if ((rc = alga_check_launch(e, "k_mg_end_lens"))) return rc;
    launch_exclusive_scan(epad, E + 1, eoff, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(end lengths)"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, MG_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t EC = hc[MG_END_COLUMNS], n_index = hc[MG_INDEX_POS];
    if (EC > 0xFFFFFFFEull) return alga_fail(e, ALGA_ERR_CAPACITY, "merge: the padded end sequences hold more than 2^32 - 2 bases");

    // the end sequences, the index
    const size_t ec_words = (size_t) (EC >> 4) + 2;
    if ((rc = alga_ensure(e, e->mg_ecols, ec_words * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->mg_pcols, ec_words * sizeof(uint32_t)))) return rc;
    uint32_t *ecols = (uint32_t *) e->mg_ecols.p, *pcols = (uint32_t *) e->mg_pcols.p;
    const MgEnds en{{eoff, elen, (uint32_t) E, EC, ecols}, pcols};
    HIP_TRY(e, hipMemsetAsync(ecols, 0, ec_words * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(pcols, 0, ec_words * sizeof(uint32_t), s));
    launch_mg_ends(tg, en, ecols, pcols, s);
    if ((rc = alga_check_launch(e, "k_mg_ends"))) return rc;
    SeedIndex ix;
    if ((rc = alga_seed_index(e, en, p->k, n_index, nullptr, s, &ix))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    // the result, into the set that is not the current one
    const int nxt = alga_other_set(e->mg_valid, e->mg_cur);
    alga_engine::MergeSet &rs = e->mg_set[nxt];
    for (DevBuf *b : {&rs.partner, &rs.olen}) if ((rc = alga_ensure(e, *b, (E + 2) * sizeof(int32_t)))) return rc;
    for (DevBuf *b : {&rs.mm, &rs.hits, &rs.estate}) if ((rc = alga_ensure(e, *b, E + 16))) return rc;
    for (DevBuf *b : {&rs.merged, &rs.rank, &rs.start, &rs.ovafter, &rs.moff, &rs.mmembers, &rs.len, &rs.coloff}) if ((rc = alga_ensure(e, *b, (T + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, rs.orient, T + 16))) return rc;
    if ((rc = alga_ensure(e, rs.begin, (T + 2) * sizeof(unsigned long long)))) return rc;
    ChainWork w;
    if ((rc = alga_chain_work(e, T, &w))) return rc;
    const MgEndOut eo{(int32_t *) rs.partner.p, (int32_t *) rs.olen.p, (uint8_t *) rs.mm.p, (uint8_t *) rs.hits.p, (uint8_t *) rs.estate.p};
    uint32_t *col_off = (uint32_t *) rs.coloff.p;
    launch_mg_overlap(en, ix, p->k, p->max_mismatches, p->max_occ, p->min_overlap, eo, seed_blocks(E, e->n_cu), cnt, s);
    if ((rc = alga_check_launch(e, "k_mg_overlap"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));

    launch_mg_joins(eo, (uint32_t) E, w.join, tg.max_blocks, s);
    if ((rc = alga_check_launch(e, "k_mg_joins"))) return rc;
    const MgLayout lo{(int32_t *) rs.merged.p, (int32_t *) rs.rank.p, (uint8_t *) rs.orient.p, (uint32_t *) rs.start.p, (int32_t *) rs.ovafter.p, (uint32_t *) rs.moff.p,
                      (int32_t *) rs.mmembers.p, (int32_t *) rs.len.p};
    if ((rc = alga_merge_tail(e, tg, eo, w, lo, col_off, rs.words, (unsigned long long *) rs.begin.p, cnt, MG_COUNTERS, "merge", "merged", nullptr, s))) return rc;
    const uint64_t NM = hc[MG_MERGED], NC = hc[MG_COLUMNS_AFTER];
    HIP_TRY(e, hipEventRecord(evs.ev[3], s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->mg_cur = nxt; e->mg_valid = true; e->mg_targets = T; e->mg_merged = NM; e->mg_columns = NC; e->mg_longest = hc[MG_LONGEST];
    out->n_targets = (int64_t) T; out->n_merged = (int64_t) NM; out->n_members = (int64_t) hc[MG_MEMBERS]; out->n_columns = NC;
    out->d_partner = eo.partner; out->d_olen = eo.olen; out->d_mm = eo.mm; out->d_hits = eo.hits; out->d_end_state = eo.state;
    out->d_merged = lo.merged; out->d_rank = lo.rank; out->d_orient = lo.orient; out->d_start = lo.start; out->d_overlap_after = lo.overlap_after;
    out->d_m_off = lo.m_off; out->d_m_members = lo.m_members;
    out->d_len = lo.m_len; out->d_col_off = col_off; out->d_begin = (const uint64_t *) rs.begin.p; out->d_words = (const uint32_t *) rs.words.p;
    if (info) {
        alga_merge_info o{};
        o.ends = hc[MG_ENDS]; o.index_positions = n_index; o.seeds = hc[MG_SEEDS]; o.seeds_over_max_occ = hc[MG_SEEDS_OVER]; o.ends_with_overlap = hc[MG_WITH_OVERLAP];
        o.ends_ambiguous = hc[MG_AMBIGUOUS]; o.hits_saturated = hc[MG_SATURATED];
        o.joins = hc[MG_JOINS]; o.joins_dropped_cycle = hc[MG_DROPPED]; o.join_mismatches = hc[MG_JOIN_MM]; o.bases_removed = hc[MG_REMOVED]; o.longest_overlap = hc[MG_LONGEST_OVERLAP];
        o.merged = NM; o.merged_multi = hc[MG_MULTI]; o.longest = hc[MG_LONGEST]; o.columns_before = C; o.columns_after = NC;
        // the lengths for the N50s (no exception leaves the C ABI: a host allocation that fails is reported like a device one)
        try {
            std::vector<int32_t> tl(T), ml(NM);
            if (T) HIP_TRY(e, hipMemcpyAsync(tl.data(), d_len, T * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            if (NM) HIP_TRY(e, hipMemcpyAsync(ml.data(), lo.m_len, NM * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(e, hipStreamSynchronize(s));
            o.n50_before = n50_of(std::vector<uint64_t>(tl.begin(), tl.end())); o.n50_after = n50_of(std::vector<uint64_t>(ml.begin(), ml.end()));
        } catch (const std::bad_alloc &) {
            return alga_fail(e, ALGA_ERR_OUT_OF_MEMORY, "merge: no host memory for the lengths of the N50s");
        }
        if ((rc = evs.ms(e, 0, 1, &o.ms_index))) return rc;
        if ((rc = evs.ms(e, 1, 2, &o.ms_overlap))) return rc;
        if ((rc = evs.ms(e, 2, 3, &o.ms_build))) return rc;
        o.ms_total = alga_ms_since(t0);
        *info = o;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" void alga_merge_default_params(alga_merge_params *p) {
    if (!p) return;
    *p = alga_merge_params{};
    p->k = 21; p->max_mismatches = 1; p->max_occ = 256; p->min_overlap = 42; p->max_overlap = 512; p->flags = 0;
}

extern "C" int alga_merge_targets_device(alga_engine *e, const uint32_t *d_words, const uint64_t *d_begin, const int32_t *d_len, int32_t n_targets,
                                         const alga_merge_params *p, void *hip_stream, alga_merged *out, alga_merge_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if (!out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "out must not be NULL");
    if (n_targets < 0 || (n_targets && (!d_words || !d_begin || !d_len))) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad target arrays");
    if (n_targets > (1 << 30)) return alga_fail(e, ALGA_ERR_CAPACITY, "merge: more than 2^30 targets");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return merge_impl(e, d_words, (const unsigned long long *) d_begin, d_len, n_targets, p, call.s, out, info);
}

extern "C" int alga_write_merged_fasta_device(alga_engine *e, const alga_merged *merged, const char *path, alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!merged || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "merged and path must not be NULL");
    const alga_engine::MergeSet &rs = e->mg_set[e->mg_cur];
    if (!e->mg_valid || merged->n_targets < 0 || (uint64_t) merged->n_targets != e->mg_targets || merged->n_merged < 0 || (uint64_t) merged->n_merged != e->mg_merged ||
        merged->n_columns != e->mg_columns || merged->d_words != (const uint32_t *) rs.words.p || merged->d_col_off != (const uint32_t *) rs.coloff.p ||
        merged->d_len != (const int32_t *) rs.len.p || merged->d_m_off != (const uint32_t *) rs.moff.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_merge_targets_device call on this engine");
    if (e->mg_longest + 96 > 0xFFFFFFFFull) return alga_fail(e, ALGA_ERR_CAPACITY, "a contig record of more than 2^32 bytes");
    HIP_TRY(e, hipSetDevice(e->device));
    const MgFasta f{merged->d_words, merged->d_col_off, merged->d_m_off, merged->d_len, (uint64_t) merged->n_merged};
    return alga_text_records(e, f, launch_mg_fasta_sizes, launch_mg_fasta_write, path, info);
}
