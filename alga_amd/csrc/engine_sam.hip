// alga_amd/csrc/engine_sam.hip -- C ABI of the pair calls over both placement passes and of the SAM writer (include/alga_amd.h:
// alga_judge_pairs_device, alga_write_sam_device; kernels in sam_kernels.hip).
//
// Host side of the judge: the host refusals, the pair_off check on the device and its one read-back; only then are the result buffers touched,
// so a refused call leaves an earlier result as it was.  Then k_sam_judge; the counters and the histogram come back at the end (the median is
// taken on the host, as the placement takes it).  The placement and the gapped result are read, never written.
// The writer: the header lines are formatted on the host from the T target lengths (and the per-target sums for the depth form of the names),
// the records go through the chunk pipeline of every text output (alga_text_job_run); its refusals come back with the sizes pass's counters,
// before the file is opened.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "gfa_kernels.h"
#include "sam_kernels.h"

using namespace alga;

namespace {

// what both calls refuse on the host
int check_inputs(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_gapped *gp, const char *what) {
    auto fail = [&](const char *why) { return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, (std::string(what) + ": " + why).c_str()); };
    if (!nodes || !pl) return fail("nodes and placements must not be NULL");
    if (nodes->n < 0 || (nodes->n & 1)) return fail("n must be even and >= 0");
    if (nodes->n && (!nodes->words || !nodes->len || nodes->stride_words <= 0)) return fail("bad node arrays");
    if (!alga_placement_is_current(e, pl)) return fail("not the result of the last placement call on this engine");
    if (gp && !alga_gapped_is_current(e, gp)) return fail("not the result of the last alga_place_gapped_device call on this engine, or made from an earlier placement");
    if ((int64_t) (nodes->n / 2) != pl->n_reads) return fail("the node set does not have the placement's reads (n / 2 != n_reads)");
    return ALGA_OK;
}

SamReads reads_of(const alga_nodes *nodes, const uint8_t *d_pair_off, const alga_placements *pl, const alga_gapped *gp) {
    SamReads v{};
    v.len = nodes->len; v.pair_off = d_pair_off; v.R = (uint64_t) pl->n_reads;
    v.h_target = pl->d_target; v.h_pos = pl->d_pos; v.h_mm = pl->d_mm; v.h_state = pl->d_state;
    if (gp) {
        v.g_target = gp->d_target; v.g_pos = gp->d_pos; v.g_end = gp->d_end; v.g_edits = gp->d_edits; v.g_state = gp->d_state;
        v.g_cigar_off = gp->d_cigar_off; v.g_cigar = gp->d_cigar;
    }
    return v;
}

int judge_impl(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const alga_placements *pl, const alga_gapped *gp, const alga_pair_params *p, hipStream_t s,
               alga_pair_calls *out, alga_pair_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t R = (uint64_t) pl->n_reads;
    const size_t n_hist = (size_t) p->max_insert + 1;
    int rc;
    AlgaEvents<2> evs;
    if ((rc = evs.create(e))) return rc;
    if ((rc = alga_ensure(e, e->sj_cnt, SAM_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->sj_cnt.p, *hc = e->h_counters;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, SAM_COUNTERS * sizeof(unsigned long long), s));

    // the check: nothing of the result is written before its verdict
    launch_sam_pair_check(d_pair_off, 2 * R, cnt, e->opt_sam_max_blocks, s);
    if ((rc = alga_check_launch(e, "k_sam_pair_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[SAM_BAD_PAIR]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "pair calls: pair_off holds a value above 2, differs between a node and its twin, or names a mate that does not point back");

    // from here on the result is rewritten
    e->sj_valid = false;
    if ((rc = alga_ensure(e, e->sj_flag, (R + 1) * sizeof(uint16_t)))) return rc;
    if ((rc = alga_ensure(e, e->sj_tlen, (R + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->sj_hist, n_hist * sizeof(unsigned long long)))) return rc;
    uint16_t *flag = (uint16_t *) e->sj_flag.p;
    int32_t *tlen = (int32_t *) e->sj_tlen.p;
    unsigned long long *hist = (unsigned long long *) e->sj_hist.p;
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    HIP_TRY(e, hipMemsetAsync(hist, 0, n_hist * sizeof(unsigned long long), s));
    launch_sam_judge(reads_of(nodes, d_pair_off, pl, gp), p->max_insert, flag, tlen, hist, cnt, e->opt_sam_max_blocks, s);
    if ((rc = alga_check_launch(e, "k_sam_judge"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));
    std::vector<unsigned long long> h(n_hist);
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, SAM_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(h.data(), hist, n_hist * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->sj_valid = true; e->sj_reads = R; e->sj_nhist = n_hist; e->sj_pl_serial = e->pl_serial; e->sj_gp_serial = gp ? e->gp_serial : 0;
    out->n_reads = (int64_t) R; out->n_hist = (int64_t) n_hist;
    out->d_flag = flag; out->d_tlen = tlen; out->d_insert_hist = (const uint64_t *) hist;
    if (info) {
        alga_pair_info o{};
        o.reads = R; o.live = hc[SAM_LIVE]; o.placed_h = hc[SAM_PLACED_H]; o.placed_g = hc[SAM_PLACED_G]; o.unplaced = hc[SAM_UNPLACED];
        o.pairs = hc[SAM_PAIRS]; o.pairs_proper = hc[SAM_PROPER]; o.pairs_improper = hc[SAM_IMPROPER]; o.pairs_split = hc[SAM_SPLIT]; o.pairs_not_unique = hc[SAM_NOT_UNIQUE];
        o.pairs_with_gapped = hc[SAM_WITH_GAPPED]; o.proper_with_gapped = hc[SAM_PROPER_GAPPED];
        o.insert_median = -1; o.insert_mean_x100 = -1;
        if (o.pairs_proper) {
            const unsigned long long half = (o.pairs_proper + 1) / 2;
            unsigned long long cum = 0;
            for (size_t i = 0; i < n_hist; i++) { cum += h[i]; if (cum >= half) { o.insert_median = (int64_t) i; break; } }
            o.insert_mean_x100 = (int64_t) ((100ull * hc[SAM_INSERT_SUM]) / o.pairs_proper);
        }
        if ((rc = evs.ms(e, 0, 1, &o.ms_judge))) return rc;
        o.ms_total = alga_ms_since(t0);
        *info = o;
    }
    return ALGA_OK;
}

// `name(t)` as the device writes it (FastaRecord::head / depth of text_record.h)
std::string sam_name(uint64_t t, uint64_t len, bool depth, uint64_t reads, uint64_t bases) {
    char buf[160];
    if (depth) snprintf(buf, sizeof(buf), "contig_id=%llu_length=%llu_reads=%llu_depth=%llu.%02llu", (unsigned long long) t, (unsigned long long) len, (unsigned long long) reads,
                        (unsigned long long) (bases / len), (unsigned long long) (((bases % len) * 100ull) / len));
    else snprintf(buf, sizeof(buf), "contig_id=%llu_length=%llu", (unsigned long long) t, (unsigned long long) len);
    return buf;
}

}  // namespace

extern "C" void alga_pair_default_params(alga_pair_params *p) {
    if (!p) return;
    *p = alga_pair_params{};
    p->max_insert = 1000; p->flags = 0;
}

extern "C" int alga_judge_pairs_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const alga_placements *pl, const alga_gapped *gp,
                                       const alga_pair_params *p, void *hip_stream, alga_pair_calls *out, alga_pair_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "pair parameters must not be NULL");
    if (p->max_insert < 1 || p->max_insert > (1 << 20)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "pair calls: max_insert must be in [1, 2^20]");
    if (p->flags) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "pair calls: unknown flag");
    for (int32_t r : p->reserved) if (r) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "pair calls: reserved must be 0");
    if (!out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "out must not be NULL");
    int rc;
    if ((rc = check_inputs(e, nodes, pl, gp, "pair calls"))) return rc;
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return judge_impl(e, nodes, d_pair_off, pl, gp, p, call.s, out, info);
}

extern "C" int alga_write_sam_device(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_gapped *gp, const alga_pair_calls *calls,
                                     const alga_sam_params *p, const char *path, alga_gfa_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "SAM parameters must not be NULL");
    if (p->flags & ~(ALGA_SAM_NAMES_DEPTH | ALGA_SAM_SKIP_UNPLACED)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "SAM: unknown flag");
    for (int32_t r : p->reserved) if (r) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "SAM: reserved must be 0");
    if (!calls || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "pair calls and path must not be NULL");
    int rc;
    if ((rc = check_inputs(e, nodes, pl, gp, "SAM"))) return rc;
    if (!e->sj_valid || calls->n_reads < 0 || (uint64_t) calls->n_reads != e->sj_reads || (uint64_t) calls->n_reads != e->pl_reads || calls->n_hist < 0 ||
        (uint64_t) calls->n_hist != e->sj_nhist || calls->d_flag != (const uint16_t *) e->sj_flag.p || calls->d_tlen != (const int32_t *) e->sj_tlen.p ||
        calls->d_insert_hist != (const uint64_t *) e->sj_hist.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "SAM: not the result of the last alga_judge_pairs_device call on this engine");
    if (e->sj_pl_serial != e->pl_serial || e->sj_gp_serial != (gp ? e->gp_serial : 0))
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "SAM: the pair calls were not made from this placement and this gapped result");
    HIP_TRY(e, hipSetDevice(e->device));

    // the header: T + 2 lines from the lengths (and the per-target sums) on hand
    const size_t T = (size_t) pl->n_targets;
    const bool depth = p->flags & ALGA_SAM_NAMES_DEPTH;
    std::vector<uint32_t> col_off(T + 1, 0);
    std::vector<unsigned long long> tstat(2 * T + 1, 0);
    HIP_TRY(e, hipMemcpy(col_off.data(), pl->d_col_off, (T + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (depth && T) HIP_TRY(e, hipMemcpy(tstat.data(), pl->d_t_reads, 2 * T * sizeof(unsigned long long), hipMemcpyDeviceToHost));   // t_reads, then t_bases
    std::string head = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n";
    for (size_t t = 0; t < T; t++) {
        const uint64_t len = col_off[t + 1] - col_off[t];
        if (!len) continue;
        head += "@SQ\tSN:" + sam_name(t, len, depth, tstat[t], tstat[T + t]) + "\tLN:" + std::to_string(len) + "\n";
    }
    head += "@PG\tID:alga_amd\tPN:alga_amd\n";

    SamText f{};
    f.v = reads_of(nodes, nullptr, pl, gp);                              // (the pairing is in the flags)
    f.words = nodes->words; f.stride = nodes->stride_words; f.flag = calls->d_flag; f.tlen = calls->d_tlen; f.col_off = pl->d_col_off;
    f.t_reads = (const unsigned long long *) pl->d_t_reads; f.t_bases = (const unsigned long long *) pl->d_t_bases;
    f.names_depth = depth ? 1 : 0; f.skip_unplaced = (p->flags & ALGA_SAM_SKIP_UNPLACED) ? 1 : 0; f.max_blocks = e->opt_sam_max_blocks; f.n = f.v.R;
    AlgaTextJob job;
    job.items = f.n;
    job.sizes = [f](uint32_t *o, unsigned long long *counters, hipStream_t s) { launch_sam_sizes(f, o, counters, s); };
    job.format = [f](const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) { launch_sam_write(f, off, i0, i1, buf, s); };
    job.verdict = [e](const unsigned long long *hc) -> int {
        if (hc[GFA_FLAGS] & SAM_BAD_LEN) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "SAM: a live read is longer than 16 * stride_words");
        if (hc[GFA_FLAGS] & SAM_BAD_SCRIPT) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "SAM: a gapped read's script has no run or not the read's length: not the node set that was placed");
        return ALGA_OK;
    };
    job.kind = "SAM"; job.head = head.c_str();
    return alga_text_job_run(e, job, path, info, t0);
}
