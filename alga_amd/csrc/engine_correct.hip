// alga_amd/csrc/engine_correct.hip -- C ABI of the read error correction (include/alga_amd.h: alga_correct_reads_device, alga_correct_parsed_reads;
// kernels in correct_kernels.hip; alga_ingest_corrected_device is in engine_ingest.hip and calls alga_correct_impl).
//
// Host side: the twin check (one flag read back), the histogram of the occurrences by the top 12 bits of the mixed key (one 4096-count read-back),
// the bins grouped into slices of at most "correct_slice_keys" occurrences -- every slice's size is known exactly before its keys are written, the
// buffers follow the largest one -- and per slice emit -> sort -> run heads -> scan -> append (one count read back: where the next slice's solid
// keys go).  Slices ascend in the mixed key, so the solid array is sorted as a whole; its directory and k_cr_fix follow.
#include <hip/hip_runtime.h>

#include <chrono>
#include <vector>

#include "engine_internal.h"
#include "correct_kernels.h"

using namespace alga;

namespace {

// counters (64-bit words of cr_cnt): the emit cursor, the two flags, the run heads of all slices, then the sums of k_cr_fix's table
enum { CC_CURSOR = 0, CC_BAD_TWIN, CC_BAD_DIR, CC_DISTINCT, CC_FIX, CC_WORDS = CC_FIX + CR_COLS };

}  // namespace

extern "C" void alga_correct_default_params(alga_correct_params *p) {
    if (!p) return;
    p->k = 21; p->solid_min = 3; p->min_run = 1; p->reserved = 0;
}

int alga_correct_check_params(alga_engine *e, const alga_correct_params *p) {
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "correction parameters must not be NULL");
    if (p->k < 5 || p->k > 31 || !(p->k & 1)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "correction: k must be odd and in [5, 31]");
    if (p->solid_min < 1) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "correction: solid_min must be >= 1");
    if (p->min_run < 1) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "correction: min_run must be >= 1");
    return ALGA_OK;
}

int alga_correct_impl(alga_engine *e, uint32_t *d_rows, int32_t stride, const int32_t *d_len, int64_t n_nodes, const alga_correct_params *p, hipStream_t s,
                      alga_correct_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    alga_correct_info out{};
    if (info) *info = out;
    const uint64_t R = (uint64_t) n_nodes / 2;
    if (R == 0) return ALGA_OK;
    int rc;
    AlgaEvents<4> evs;
    if ((rc = evs.create(e))) return rc;
    const int fix_blocks = cr_fix_blocks(R, e->n_cu);
    const size_t table_words = std::max<size_t>((size_t) CR_HIST_BLOCKS * CR_HIST_COLS, std::max<size_t>((size_t) fix_blocks * CR_COLS, CR_RUNS_BLOCKS));
    if ((rc = alga_ensure(e, e->cr_cnt, CC_WORDS * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->cr_table, table_words * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->cr_hist, CR_HIST_COLS * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->cr_cnt.p, *hc = e->h_counters;
    uint32_t *table = (uint32_t *) e->cr_table.p;
    const CrReads c{d_rows, stride, d_len, R, p->k};
    HIP_TRY(e, hipMemsetAsync(cnt, 0, CC_WORDS * sizeof(unsigned long long), s));

    // nothing is written before the twins are known to be twins
    launch_cr_twin(c, (uint32_t *) (cnt + CC_BAD_TWIN), s);
    if ((rc = alga_check_launch(e, "k_cr_twin"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt + CC_BAD_TWIN, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[0]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "correction: a row 2r is not the reverse complement of row 2r + 1, their lengths differ, or a length exceeds the stride");

    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    const int hist_blocks = launch_cr_hist(c, table, s);
    if ((rc = alga_check_launch(e, "k_cr_hist"))) return rc;
    launch_cr_sum(table, hist_blocks, CR_HIST_COLS, (unsigned long long *) e->cr_hist.p, false, s);
    if ((rc = alga_check_launch(e, "k_cr_sum"))) return rc;
    std::vector<unsigned long long> hist(CR_HIST_COLS);
    HIP_TRY(e, hipMemcpyAsync(hist.data(), e->cr_hist.p, CR_HIST_COLS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    out.reads = hist[CR_HIST_READS];
    for (int b = 0; b < CR_BINS; b++) out.kmers_total += hist[b];

    // slices: consecutive bins while they fit the budget; a bin above it alone
    struct Slice { uint32_t lo, hi; uint64_t n; };
    std::vector<Slice> slices;
    const uint64_t budget = (uint64_t) e->opt_correct_slice_keys;
    uint64_t largest = 0;
    for (uint32_t b = 0; b < (uint32_t) CR_BINS;) {
        uint64_t n = hist[b];
        uint32_t hi = b + 1;
        while (hi < (uint32_t) CR_BINS && n + hist[hi] <= budget) n += hist[hi++];
        if (n) { slices.push_back({b, hi, n}); largest = std::max(largest, n); }
        b = hi;
    }
    if (largest >= 0xFFFFFFF0ull) return alga_fail(e, ALGA_ERR_CAPACITY, "correction: more than 2^32 occurrences in one slice of the k-mer count");
    const uint64_t solid_cap = out.kmers_total / (uint64_t) p->solid_min;        // every solid key has solid_min occurrences of its own
    if (solid_cap >= 0xFFFFFFF0ull) return alga_fail(e, ALGA_ERR_CAPACITY, "correction: more than 2^32 solid k-mers");
    for (int j = 0; j < 2; j++) if ((rc = alga_ensure(e, e->cr_keys[j], (largest + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->cr_flag, (largest + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->cr_pos, (largest + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->cr_solid, (solid_cap + 2) * sizeof(unsigned long long)))) return rc;
    const size_t temp = sort_u64_keys_temp_bytes(largest);
    if ((rc = alga_ensure(e, e->sort_temp, temp))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(largest)))) return rc;
    unsigned long long *keys0 = (unsigned long long *) e->cr_keys[0].p, *keys1 = (unsigned long long *) e->cr_keys[1].p, *solid = (unsigned long long *) e->cr_solid.p;
    uint64_t n_solid = 0;
    for (const Slice &sl : slices) {
        HIP_TRY(e, hipMemsetAsync(cnt + CC_CURSOR, 0, sizeof(unsigned long long), s));
        launch_cr_emit(c, sl.lo, sl.hi, keys0, sl.n, cnt + CC_CURSOR, s);
        if ((rc = alga_check_launch(e, "k_cr_emit"))) return rc;
        HIP_TRY(e, sort_u64_keys(e->sort_temp.p, temp, keys0, keys1, sl.n, s));
        const int run_blocks = launch_cr_runs(keys1, sl.n, p->solid_min, (uint32_t *) e->cr_flag.p, table, s);
        if ((rc = alga_check_launch(e, "k_cr_runs"))) return rc;
        launch_cr_sum(table, run_blocks, 1, cnt + CC_DISTINCT, true, s);
        launch_exclusive_scan((const uint32_t *) e->cr_flag.p, sl.n, (uint32_t *) e->cr_pos.p, (uint64_t *) e->scan_scratch.p, s);
        if ((rc = alga_check_launch(e, "scan(solid)"))) return rc;
        launch_cr_append(keys1, (const uint32_t *) e->cr_flag.p, (const uint32_t *) e->cr_pos.p, sl.n, solid, n_solid, solid_cap, s);
        if ((rc = alga_check_launch(e, "k_cr_append"))) return rc;
        HIP_TRY(e, hipMemcpyAsync(&hc[0], (uint64_t *) e->scan_scratch.p + scan_total_index(sl.n), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipMemcpyAsync(&hc[1], cnt + CC_CURSOR, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        if (hc[1] != sl.n) return alga_fail(e, ALGA_ERR_HIP, "correction: a slice holds another number of k-mers than the histogram counted");
        n_solid += hc[0];
        if (n_solid > solid_cap) return alga_fail(e, ALGA_ERR_HIP, "correction: more solid k-mers than the occurrences allow");
    }
    out.slices = slices.size();
    out.kmers_solid = n_solid;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    // the directory: about two keys per bucket unless the option says otherwise
    int bits = e->opt_correct_dir_bits;
    if (bits <= 0) { bits = 1; while (bits < CR_DIR_BITS_MAX && (n_solid >> bits) > 2) bits++; }
    if ((rc = alga_ensure(e, e->cr_dir, (((size_t) 1 << bits) + 2) * sizeof(uint32_t)))) return rc;
    launch_cr_dir(solid, n_solid, bits, (uint32_t *) e->cr_dir.p, (uint32_t *) (cnt + CC_BAD_DIR), s);
    if ((rc = alga_check_launch(e, "k_cr_dir"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt + CC_BAD_DIR, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[0]) return alga_fail(e, ALGA_ERR_HIP, "correction: the solid k-mers are not in ascending order");

    const CrFix f{solid, (const uint32_t *) e->cr_dir.p, bits, p->min_run};
    const int fb = launch_cr_fix(c, f, e->n_cu, table, s);
    if ((rc = alga_check_launch(e, "k_cr_fix"))) return rc;
    launch_cr_sum(table, fb, CR_COLS, cnt + CC_FIX, false, s);
    if ((rc = alga_check_launch(e, "k_cr_sum"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[3], s));
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, CC_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    out.kmers_distinct = hc[CC_DISTINCT];
    out.runs = hc[CC_FIX + CR_RUNS]; out.runs_fixed = hc[CC_FIX + CR_FIXED]; out.runs_ambiguous = hc[CC_FIX + CR_AMBIGUOUS];
    out.runs_no_candidate = hc[CC_FIX + CR_NO_CANDIDATE]; out.runs_skipped = hc[CC_FIX + CR_SKIPPED]; out.reads_changed = hc[CC_FIX + CR_CHANGED];
    if ((rc = evs.ms(e, 0, 1, &out.ms_count))) return rc;
    if ((rc = evs.ms(e, 1, 2, &out.ms_index))) return rc;
    if ((rc = evs.ms(e, 2, 3, &out.ms_fix))) return rc;
    out.ms_total = alga_ms_since(t0);
    if (info) *info = out;
    return ALGA_OK;
}

extern "C" int alga_correct_reads_device(alga_engine *e, uint32_t *d_rows, int32_t stride_words, const int32_t *d_len, int64_t n_nodes, const alga_correct_params *p,
                                         void *hip_stream, alga_correct_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = alga_correct_check_params(e, p))) return rc;
    if (n_nodes < 0 || (n_nodes & 1)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "n_nodes must be even and >= 0");
    if (n_nodes >= 0x7FFFFFFELL) return alga_fail(e, ALGA_ERR_CAPACITY, "too many nodes");
    if (n_nodes && (!d_rows || !d_len || stride_words <= 0)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad node arrays");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return alga_correct_impl(e, d_rows, stride_words, d_len, n_nodes, p, call.s, info);
}

extern "C" int alga_correct_parsed_reads(alga_engine *e, alga_parsed_reads *pr, const alga_correct_params *p, alga_correct_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = alga_correct_check_params(e, p))) return rc;
    if (!pr) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "parsed reads must not be NULL");
    if (pr->n_nodes < 0 || (pr->n_nodes & 1)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "n_nodes must be even and >= 0");
    if (pr->n_nodes >= 0x7FFFFFFELL) return alga_fail(e, ALGA_ERR_CAPACITY, "too many nodes");
    if (pr->n_nodes == 0) return ALGA_OK;
    if (!pr->rows || !pr->len || pr->stride_words <= 0) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad node arrays");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = e->own_stream;
    const size_t n = (size_t) pr->n_nodes, row_bytes = n * (size_t) pr->stride_words * sizeof(uint32_t);
    if ((rc = alga_ensure(e, e->pp_rows, row_bytes))) return rc;
    if ((rc = alga_ensure(e, e->pp_len, (n + 2) * sizeof(int32_t)))) return rc;
    HIP_TRY(e, hipStreamSynchronize(s));
    if ((rc = alga_staged_h2d(e, e->pp_rows.p, pr->rows, row_bytes))) return rc;
    if ((rc = alga_staged_h2d(e, e->pp_len.p, pr->len, n * sizeof(int32_t)))) return rc;
    rc = alga_correct_impl(e, (uint32_t *) e->pp_rows.p, pr->stride_words, (const int32_t *) e->pp_len.p, pr->n_nodes, p, s, info);
    (void) hipStreamSynchronize(s);
    if (rc) return rc;
    return alga_staged_d2h(e, pr->rows, e->pp_rows.p, row_bytes);
}
