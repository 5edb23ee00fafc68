// alga_amd/csrc/engine_consensus.hip -- C ABI of the unitig consensus (include/alga_amd.h: alga_unitig_consensus_device; kernels in
// consensus_kernels.hip).  The FASTA of the windows is written by engine_gfa.hip (alga_write_consensus_fasta_device).
//
// Host side: the device's verdict on the input (one read-back, before anything is written), the vote, one read-back of the counters that says
// whether any word is left to the wide kernel, the windows.
#include <hip/hip_runtime.h>

#include <chrono>

#include "consensus_kernels.h"
#include "engine_internal.h"

using namespace alga;

namespace {

int consensus_impl(alga_engine *e, const alga_nodes *nodes, const alga_unitigs *u, int32_t min_votes, int32_t flags, hipStream_t s, alga_consensus *out,
                   alga_consensus_info *info) {
    const uint64_t P = (uint64_t) u->n_pairs;
    int rc;
    AlgaEvents<3> evs;
    if ((rc = evs.create(e))) return rc;
    // the sizes of the ragged arrays: the last entries of the two offset arrays
    unsigned long long totals[2] = {0, 0};
    if (P) {
        HIP_TRY(e, hipMemcpyAsync(&e->h_counters[0], u->d_word_off + P, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipMemcpyAsync(&e->h_counters[1], u->d_path_off + P, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        totals[0] = e->h_counters[0]; totals[1] = e->h_counters[1];
    }
    ConsCfg c{nodes->words, nodes->stride_words, nodes->len, nodes->n, u->d_path_node, u->d_path_pos, (const unsigned long long *) u->d_path_off,
              (const unsigned long long *) u->d_word_off, u->d_len, u->d_words, (uint32_t) P, totals[0], totals[1], min_votes, (uint32_t) e->opt_consensus_max_blocks};
    if ((rc = alga_ensure(e, e->cs_cnt, CS_COUNTERS * sizeof(unsigned long long)))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->cs_cnt.p;
    HIP_TRY(e, hipMemsetAsync(cnt, 0, CS_COUNTERS * sizeof(unsigned long long), s));
    HIP_TRY(e, hipEventRecord(evs.ev[0], s));
    launch_cons_check(c, cnt, s);
    if ((rc = alga_check_launch(e, "k_cons_check"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (const unsigned long long bad = e->h_counters[CS_FLAGS]) {
        const char *why = (bad & CS_BAD_NODE) ? "a path node is outside [0, n)" : (bad & CS_BAD_LEN) ? "a path node's length is 0 or does not fit its row"
                        : "the node lengths do not give the layout of the unitigs (not the node set of the unitig call)";
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, why);
    }
    // the input is valid: from here on the previous consensus is rewritten
    e->cs_valid = false; e->fc_valid = false;
    const bool want_votes = flags & ALGA_CONSENSUS_VOTES;
    if ((rc = alga_ensure(e, e->cs_words, (size_t) (c.n_words + 4) * sizeof(uint32_t)))) return rc;      // (a 16-base fetch may touch the word behind a row)
    if ((rc = alga_ensure(e, e->cs_mask, (size_t) (c.n_words + 1) * sizeof(uint32_t)))) return rc;
    if (want_votes && (rc = alga_ensure(e, e->cs_votes, (size_t) (c.n_words + 1) * 16))) return rc;
    if ((rc = alga_ensure(e, e->cs_trim, (size_t) (P + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->cs_len, (size_t) (P + 1) * sizeof(int32_t)))) return rc;
    if ((rc = alga_ensure(e, e->cs_changed, (size_t) (P + 1) * sizeof(int32_t)))) return rc;
    uint32_t *words = (uint32_t *) e->cs_words.p, *mask = (uint32_t *) e->cs_mask.p;
    uint8_t *votes = want_votes ? (uint8_t *) e->cs_votes.p : nullptr;
    int32_t *changed = (int32_t *) e->cs_changed.p;
    HIP_TRY(e, hipMemsetAsync(changed, 0, (size_t) (P + 1) * sizeof(int32_t), s));
    HIP_TRY(e, hipMemsetAsync(words + c.n_words, 0, 4 * sizeof(uint32_t), s));
    launch_cons_vote(c, words, mask, votes, changed, cnt, s);
    if ((rc = alga_check_launch(e, "k_cons_vote"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, CS_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t wide = e->h_counters[CS_WIDE];
    if (wide) {
        launch_cons_vote_wide(c, words, mask, votes, changed, cnt, s);
        if ((rc = alga_check_launch(e, "k_cons_vote_wide"))) return rc;
    }
    HIP_TRY(e, hipEventRecord(evs.ev[1], s));
    launch_cons_window(c, mask, (int32_t *) e->cs_trim.p, (int32_t *) e->cs_len.p, cnt, s);
    if ((rc = alga_check_launch(e, "k_cons_window"))) return rc;
    HIP_TRY(e, hipEventRecord(evs.ev[2], s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, CS_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));

    e->cs_valid = true; e->cs_has_votes = want_votes;
    out->n_pairs = u->n_pairs;
    out->d_words = words; out->d_trim_left = (const int32_t *) e->cs_trim.p; out->d_len = (const int32_t *) e->cs_len.p;
    out->d_changed = changed; out->d_votes = votes;
    if (info) {
        info->pairs = P; info->pairs_kept = e->h_counters[CS_KEPT]; info->trimmed_bases = e->h_counters[CS_TRIMMED];
        info->changed = e->h_counters[CS_CHANGED]; info->max_depth = e->h_counters[CS_MAX_DEPTH]; info->wide_words = wide;
        info->columns = e->ut_total_bases;
        if ((rc = evs.ms(e, 0, 1, &info->ms_vote))) return rc;
        if ((rc = evs.ms(e, 1, 2, &info->ms_window))) return rc;
    }
    return ALGA_OK;
}

}  // namespace

extern "C" int alga_unitig_consensus_device(alga_engine *e, const alga_nodes *nodes, const alga_unitigs *u, int32_t min_votes, int32_t flags, void *hip_stream,
                                            alga_consensus *out, alga_consensus_info *info) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    const auto t0 = std::chrono::steady_clock::now();
    if (info) *info = alga_consensus_info{};
    if (!nodes || !u || !out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes, unitigs and out must not be NULL");
    if (flags & ~ALGA_CONSENSUS_VOTES) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unknown consensus flag");
    if (min_votes < 0) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "min_votes must not be negative");
    if (!e->ut_valid || u->d_len != (const int32_t *) e->ut_ulen.p || (uint64_t) u->n_pairs != e->ut_n_pairs || u->n_edges != e->ut_n_edges ||
        u->d_words != (const uint32_t *) e->ut_words.p || u->d_path_node != (const int32_t *) e->ut_path_node.p ||
        u->d_path_pos != (const int32_t *) e->ut_path_pos.p || u->d_path_off != (const uint64_t *) e->ut_path_off.p ||
        u->d_word_off != (const uint64_t *) e->ut_word_off.p)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the result of the last alga_unitigs_device call on this engine");
    if (nodes->n < 0 || (nodes->n & 1)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "the node count must be even (twin layout)");
    if (nodes->n != e->ut_n_nodes) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "not the node set of the unitig call (another node count)");
    if (nodes->n && (!nodes->len || !nodes->words || nodes->stride_words <= 0)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad node set");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    const int rc = consensus_impl(e, nodes, u, min_votes, flags, s, out, info);
    if (rc != ALGA_OK) { (void) hipStreamSynchronize(s); return rc; }
    if (info) info->ms_total = alga_ms_since(t0);
    return ALGA_OK;
}
