// alga_amd/csrc/engine_contain.hip -- C ABI of the containment stage (include/alga_amd.h: alga_drop_contained_device,
// alga_write_kept_fasta_device; kernels in contain_kernels.hip).
//
// Host side: the check runs on a workspace and ends in one read-back (the refusal flag, the column sum, the padded columns, the indexed
// positions: they size the column arrays, the sort and the directory).  Then, still on workspaces: the scan of the padded lengths, the two
// column arrays, the seed index over the forward one (alga_seed_index), k_ct_contain.  The result is written into the set of buffers that
// does NOT hold the current result: the decision, the roots, the absorbed counts; a read-back of the counters (the kept targets and their
// columns size what follows); the scans, the numbering and the build.  The sets are swapped at the end, so a call that is refused or fails
// anywhere leaves an earlier result as it was, and a call may take its targets from that result.  The lengths for the N50s come back only
// when `info` is given.  No step walks on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "engine_internal.h"
#include "gfa_kernels.h"
#include "ingest_kernels.h"
#include "contain_kernels.h"

using namespace alga;

namespace {

int check_params(alga_engine *e, const alga_contain_params *p) {
    if (!p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "contain parameters must not be NULL");
    if (p->k < 8 || p->k > 31) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "contain: k must be in [8, 31]");
    if (p->max_permille < 0 || p->max_permille > 100) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "contain: max_permille must be in [0, 100]");
    if (p->max_occ < 1 || p->max_occ > 65535) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "contain: max_occ must be in [1, 65535]");
    if (p->flags || p->reserved[0] || p->reserved[1]) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "contain: flags and reserved must be 0");
    return ALGA_OK;
}

int contain_impl(alga_engine *e, const uint32_t *d_words, const unsigned long long *d_begin, const int32_t *d_len, int32_t n_targets, const alga_contain_params *p,
                 hipStream_t s, alga_kept *out, alga_contain_info *info) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t T = (uint64_t) n_targets, Q = 2 * T;
    int rc;
    AlgaEvents<4> evs;
    if ((rc = evs.create(e))) return rc;
    if ((rc = alga_ensure(e, e->cn_cnt, CN_COUNTERS * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->cn_pad, (T + 2) * sizeof(uint32_t)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->cn_cnt.p, *hc = e->h_counters;
    uint32_t *pad = (uint32_t *) e->cn_pad.p;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, CN_COUNTERS * sizeof(unsigned long long), s));
    const CnTargets tg{d_words, d_begin, d_len, (uint32_t) T, (uint32_t) e->opt_contain_max_blocks};

    // the check: nothing of the result is written before its verdict
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    launch_cn_check(tg, p->k, pad, cnt, s);
    if ((rc = alga_check_launch(e, "k_ct_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, CN_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (hc[CN_BAD] & CN_BAD_LEN) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "contain: negative target length");
    const uint64_t C = hc[CN_COLUMNS], CC = hc[CN_PAD_COLUMNS], n_index = hc[CN_INDEX_POS], n_queries = hc[CN_QUERIES];
    if (C > 0xFFFFFFFEull) return alga_fail(e, ALGA_ERR_CAPACITY, "contain: the targets hold more than 2^32 - 2 bases");
    if (CC > 0xFFFFFFFEull) return alga_fail(e, ALGA_ERR_CAPACITY, "contain: the word-aligned targets hold more than 2^32 - 2 bases");

    // workspaces: the offsets, the two column arrays, the index
    if ((rc = alga_ensure(e, e->cn_off, (T + 2) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(T + 2)))) return rc;
    uint32_t *off = (uint32_t *) e->cn_off.p;
    launch_exclusive_scan(pad, T + 1, off, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(padded lengths)"))) return rc;
    const size_t c_words = (size_t) (CC >> 4) + 2;
    if ((rc = alga_ensure(e, e->cn_cols, c_words * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->cn_rcols, c_words * sizeof(uint32_t)))) return rc;
    uint32_t *cols = (uint32_t *) e->cn_cols.p, *rcols = (uint32_t *) e->cn_rcols.p;
    const CnSpace sp{{off, d_len, (uint32_t) T, CC, cols}, rcols};
    HIP_TRY(e, hipMemsetAsync(cols, 0, c_words * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(rcols, 0, c_words * sizeof(uint32_t), s));
    launch_cn_cols(tg, sp, cols, rcols, s);
    if ((rc = alga_check_launch(e, "k_ct_cols"))) return rc;
    SeedIndex ix;
    if ((rc = alga_seed_index(e, sp, p->k, n_index, nullptr, s, &ix))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));

    // the hot path, on workspaces: per (c, s)
    for (DevBuf *b : {&e->cn_qmm, &e->cn_qhits, &e->cn_qhost, &e->cn_qpos}) if ((rc = alga_ensure(e, *b, (Q + 2) * sizeof(uint32_t)))) return rc;
    for (DevBuf *b : {&e->cn_keep, &e->cn_keepscan}) if ((rc = alga_ensure(e, *b, (T + 2) * sizeof(uint32_t)))) return rc;
    const CnQueryOut qo{(uint32_t *) e->cn_qmm.p, (uint32_t *) e->cn_qhits.p, (int32_t *) e->cn_qhost.p, (int32_t *) e->cn_qpos.p};
    uint32_t *keep = (uint32_t *) e->cn_keep.p, *keep_scan = (uint32_t *) e->cn_keepscan.p;
    launch_cn_contain(sp, ix, p->k, p->max_permille, p->max_occ, qo, seed_blocks(Q, e->n_cu), cnt, s);
    if ((rc = alga_check_launch(e, "k_ct_contain"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));

    // the result, into the set that is not the current one
    const int nxt = alga_other_set(e->cn_valid, e->cn_cur);
    alga_engine::ContainSet &rs = e->cn_set[nxt];
    for (DevBuf *b : {&rs.host, &rs.hostpos, &rs.mm, &rs.root[0], &rs.root[1], &rs.rootpos[0], &rs.rootpos[1], &rs.absorbed, &rs.newid, &rs.old, &rs.len, &rs.coloff})
        if ((rc = alga_ensure(e, *b, (T + 2) * sizeof(uint32_t)))) return rc;
    for (DevBuf *b : {&rs.hostorient, &rs.hits, &rs.state, &rs.rootorient[0], &rs.rootorient[1]}) if ((rc = alga_ensure(e, *b, T + 16))) return rc;
    if ((rc = alga_ensure(e, rs.begin, (T + 2) * sizeof(unsigned long long)))) return rc;
    const CnOut co{(int32_t *) rs.host.p, (int32_t *) rs.hostpos.p, (uint8_t *) rs.hostorient.p, (uint32_t *) rs.mm.p, (uint8_t *) rs.hits.p, (uint8_t *) rs.state.p};
    launch_cn_decide(tg, qo, co, keep, cnt, s);
    if ((rc = alga_check_launch(e, "k_ct_decide"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(hc, cnt, CN_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t NK = hc[CN_KEPT], NC = hc[CN_COLUMNS_AFTER], n_contained = hc[CN_CONTAINED];

    // the roots: ceil(log2 T) + 1 rounds, none where nothing is contained
    const CnRoots rt[2] = {{(int32_t *) rs.root[0].p, (int32_t *) rs.rootpos[0].p, (uint8_t *) rs.rootorient[0].p},
                           {(int32_t *) rs.root[1].p, (int32_t *) rs.rootpos[1].p, (uint8_t *) rs.rootorient[1].p}};
    int cur = 0;
    launch_cn_root_init(tg, co, rt[0], s);
    if ((rc = alga_check_launch(e, "k_ct_root_init"))) return rc;
    if (n_contained) {
        int rounds = 1;
        while ((1ull << (rounds - 1)) < T) rounds++;
        for (int r = 0; r < rounds; r++) {
            launch_cn_root_jump(tg, rt[cur], rt[1 - cur], s);
            if ((rc = alga_check_launch(e, "k_ct_root_jump"))) return rc;
            cur = 1 - cur;
        }
    }
    uint32_t *absorbed = (uint32_t *) rs.absorbed.p;
    HIP_TRY(e, hipMemsetAsync(absorbed, 0, (T + 2) * sizeof(uint32_t), s));
    if (n_contained) launch_cn_absorbed(tg, co, rt[cur], absorbed, s);
    if ((rc = alga_check_launch(e, "k_ct_absorbed"))) return rc;

    // the kept targets: new ids, lengths, columns, bases
    int32_t *d_new = (int32_t *) rs.newid.p, *d_old = (int32_t *) rs.old.p, *klen = (int32_t *) rs.len.p;
    uint32_t *col_off = (uint32_t *) rs.coloff.p;
    const size_t new_words = (size_t) ((NC + 15) >> 4) + 2;
    if ((rc = alga_ensure(e, rs.words, new_words * sizeof(uint32_t)))) return rc;
    HIP_TRY(e, hipMemsetAsync(klen, 0, (T + 2) * sizeof(int32_t), s));
    HIP_TRY(e, hipMemsetAsync(col_off, 0, (T + 2) * sizeof(uint32_t), s));
    launch_exclusive_scan(keep, T + 1, keep_scan, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(kept targets)"))) return rc;
    launch_cn_number(tg, keep, keep_scan, d_new, d_old, klen, s);
    if ((rc = alga_check_launch(e, "k_ct_number"))) return rc;
    if (NK) launch_exclusive_scan((const uint32_t *) klen, NK + 1, col_off, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(kept lengths)"))) return rc;
    launch_cn_build(tg, d_old, col_off, (uint32_t) NK, NC, (uint32_t *) rs.words.p, (unsigned long long *) rs.begin.p, s);
    if ((rc = alga_check_launch(e, "k_ct_build"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[3], s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->cn_cur = nxt; e->cn_valid = true; e->cn_targets = T; e->cn_kept = NK; e->cn_columns = NC; e->cn_longest = hc[CN_LONGEST_KEPT];
    out->n_targets = (int64_t) T; out->n_kept = (int64_t) NK; out->n_columns = NC;
    out->d_host = co.host; out->d_host_pos = co.host_pos; out->d_host_orient = co.host_orient; out->d_mm = co.mm; out->d_hits = co.hits; out->d_state = co.state;
    out->d_root = rt[cur].root; out->d_root_pos = rt[cur].pos; out->d_root_orient = rt[cur].orient; out->d_absorbed = absorbed;
    out->d_new = d_new; out->d_old = d_old;
    out->d_len = klen; out->d_col_off = col_off; out->d_begin = (const uint64_t *) rs.begin.p; out->d_words = (const uint32_t *) rs.words.p;
    if (info) {
        alga_contain_info o{};
        o.queries = n_queries; o.index_positions = n_index; o.seeds = hc[CN_SEEDS]; o.seeds_over_max_occ = hc[CN_SEEDS_OVER]; o.candidates = hc[CN_CANDIDATES];
        o.contained = n_contained; o.contained_minus = hc[CN_MINUS]; o.duplicates = hc[CN_DUPLICATES]; o.ambiguous = hc[CN_AMBIGUOUS]; o.hits_saturated = hc[CN_SATURATED];
        o.kept = NK; o.bases_removed = hc[CN_REMOVED]; o.longest_contained = hc[CN_LONGEST_CONTAINED]; o.columns_before = C; o.columns_after = NC;
        // the lengths for the N50s (no exception leaves the C ABI: a host allocation that fails is reported like a device one)
        try {
            std::vector<int32_t> tl(T), kl(NK);
            if (T) HIP_TRY(e, hipMemcpyAsync(tl.data(), d_len, T * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            if (NK) HIP_TRY(e, hipMemcpyAsync(kl.data(), klen, NK * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(e, hipStreamSynchronize(s));
            o.n50_before = n50_of(std::vector<uint64_t>(tl.begin(), tl.end())); o.n50_after = n50_of(std::vector<uint64_t>(kl.begin(), kl.end()));
        } catch (const std::bad_alloc &) {
            return alga_fail(e, ALGA_ERR_OUT_OF_MEMORY, "contain: no host memory for the lengths of the N50s");
        }
        if ((rc = evs.ms(e, 0, 1, &o.ms_index))) return rc;
        if ((rc = evs.ms(e, 1, 2, &o.ms_contain))) return rc;
        if ((rc = evs.ms(e, 2, 3, &o.ms_build))) return rc;
        o.ms_total = alga_ms_since(t0);
        *info = o;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" void alga_contain_default_params(alga_contain_params *p) {
    if (!p) return;
    *p = alga_contain_params{};
    p->k = 21; p->max_permille = 10; p->max_occ = 256; p->flags = 0;
}

extern "C" int alga_drop_contained_device(alga_engine *e, const uint32_t *d_words, const uint64_t *d_begin, const int32_t *d_len, int32_t n_targets,
                                          const alga_contain_params *p, void *hip_stream, alga_kept *out, alga_contain_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_params(e, p))) return rc;
    if (!out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "out must not be NULL");
    if (n_targets < 0 || (n_targets && (!d_words || !d_begin || !d_len))) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad target arrays");
    if (n_targets > (1 << 30)) return alga_fail(e, ALGA_ERR_CAPACITY, "contain: more than 2^30 targets");
    AlgaStageCall call;
    if ((rc = call.begin(e, hip_stream))) return rc;
    return contain_impl(e, d_words, (const unsigned long long *) d_begin, d_len, n_targets, p, call.s, out, info);
}

extern "C" int alga_write_kept_fasta_device(alga_engine *e, const alga_kept *kept, const char *path, alga_gfa_info *info) {
    if (!alga_enter(e, info)) return ALGA_ERR_INVALID_ARGUMENT;
    if (!kept || !path || !*path) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "kept and path must not be NULL");
    const alga_engine::ContainSet &rs = e->cn_set[e->cn_cur];
    if (!e->cn_valid || kept->n_targets < 0 || (uint64_t) kept->n_targets != e->cn_targets || kept->n_kept < 0 || (uint64_t) kept->n_kept != e->cn_kept ||
        kept->n_columns != e->cn_columns || kept->d_words != (const uint32_t *) rs.words.p || kept->d_col_off != (const uint32_t *) rs.coloff.p ||
        kept->d_len != (const int32_t *) rs.len.p || kept->d_old != (const int32_t *) rs.old.p || kept->d_absorbed != (const uint32_t *) rs.absorbed.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_drop_contained_device call on this engine");
    if (e->cn_longest + 96 > 0xFFFFFFFFull) return alga_fail(e, ALGA_ERR_CAPACITY, "a contig record of more than 2^32 bytes");
    HIP_TRY(e, hipSetDevice(e->device));
    const CnFasta f{kept->d_words, kept->d_col_off, kept->d_absorbed, kept->d_len, kept->d_old, (uint64_t) kept->n_kept};
    return alga_text_records(e, f, launch_cn_fasta_sizes, launch_cn_fasta_write, path, info);
}
