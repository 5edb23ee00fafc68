// alga_amd/csrc/engine.hip -- host side of the C ABI declared in include/alga_amd.h.
//
// Orchestrates the kernels of prefsuf_kernels.hip on one HIP stream.  Phases of a build:
//   seed   : memset + k_seed_build
//   probe  : k_probe_sources                      (dominant kernel; retried with a larger record
//                                                  buffer if the first capacity guess overflows)
//   group  : k_make_keys + radix sort by target + k_rowptr_from_sorted + k_gather_heads
//   reduce : k_reduce_targets
//   emit   : scan(out-degree) + k_scatter_by_source + k_sort_rows
// With the source-side reduction (alga_reduction) the probing wave emits final edges and
// group/reduce disappear: seed, probe, emit (radix sort of the edges by (src, dst)).
// There is no CPU fallback anywhere in this file: every failure is reported to the caller.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "engine_internal.h"
#include "prefsuf_shard.h"

using namespace alga;

namespace {

using Prepared = AlgaPrepared;

// Validates arguments, measures max read length / live nodes on the device and derives the
// iteration bounds of GraphCreatorPrefSuf::startAlignmentGraphCreation (GraphCreatorPrefSuf.cpp:91-100).
int prepare(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, hipStream_t s, Prepared &out) {
    if (!nodes || !p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes/params must not be NULL");
    if (nodes->n < 0) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "negative node count");
    if (nodes->n > 0 && (!nodes->words || !nodes->len)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "words/len must not be NULL");
    if (nodes->stride_words <= 0 && nodes->n > 0) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stride_words must be positive");
    if (p->min_overlap < 1 || p->min_overlap > 501) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "min_overlap must be in [1, 501]");
    if (p->soes != 3) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "soes must be 3 (the reference hard-codes SOES = 3)");
    if (p->max_len_cap < 1 || p->max_len_cap > 500) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "max_len_cap must be in [1, 500]");
    if (p->rsoe_min_overlap < 0) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "rsoe_min_overlap must be >= 0");
    if (p->keys_shared < 0 || p->keys_shared > 2) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "keys_shared must be 0, 1 or 2");
    int rc;
    if ((rc = alga_ensure(e, e->counters, (CNT_TOTAL + 2) * sizeof(unsigned long long)))) return rc;
    HIP_TRY(e, hipMemsetAsync(e->counters.p, 0, (CNT_TOTAL + 2) * sizeof(unsigned long long), s));
    NodesDev nd;
    nd.words = nodes->words; nd.len = nodes->len; nd.from = nodes->align_from; nd.to = nodes->align_to;
    nd.n = nodes->n; nd.stride = nodes->stride_words;
    unsigned long long *cnt = (unsigned long long *) e->counters.p;
    int *d_maxlen = (int *) (cnt + CNT_TOTAL);
    unsigned long long mask_asym = 0;
    int min_len = 0;
    if (p->keys_shared == 2 && e->store_n == nodes->n && e->store_words == (const void *) nodes->words && e->stat_len == (const void *) nodes->len &&
        e->stat_from == (const void *) nodes->align_from && e->stat_to == (const void *) nodes->align_to) {
        // a further piece of the build that measured this node set last (keys_shared = 2 promises nothing came in between)
        out.max_len = e->stat_max_len; out.live = e->stat_live; mask_asym = e->stat_mask_asym; min_len = e->stat_min_len;
    } else {
        launch_node_stats(nd, cnt, d_maxlen, s);
        if ((rc = alga_check_launch(e, "k_node_stats"))) return rc;
        HIP_TRY(e, hipMemcpyAsync(e->h_counters, e->counters.p, (CNT_TOTAL + 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        out.max_len = (int) (e->h_counters[CNT_TOTAL] & 0xFFFFFFFFull);
        min_len = out.max_len > 0 ? 0x7FFFFFFF - (int) (e->h_counters[CNT_TOTAL] >> 32) : 0;
        out.live = e->h_counters[CNT_LIVE_NODES];
        mask_asym = e->h_counters[CNT_MASK_ASYM];
        e->stat_max_len = out.max_len; e->stat_min_len = min_len; e->stat_live = out.live; e->stat_mask_asym = mask_asym;
        e->stat_len = (const void *) nodes->len; e->stat_from = (const void *) nodes->align_from; e->stat_to = (const void *) nodes->align_to;
    }
    out.nd = nd;
    out.uniform_len = (out.max_len > 0 && min_len == out.max_len && !nodes->align_from) ? out.max_len : 0;
    if ((int64_t) blocks_of(out.max_len) > (int64_t) nodes->stride_words)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "stride_words is smaller than the longest read needs");
    if (out.max_len > OL_MAX_NODE_LEN) return alga_fail(e, ALGA_ERR_CAPACITY, "a node is longer than 4 194 303 nt (overlap records keep the offset in 22 bits)");
    PrefSufCfg c;
    c.Lmin = p->min_overlap;
    c.rsoemo = p->rsoe_min_overlap;
    c.Lcap = std::min(out.max_len, p->max_len_cap) + 1;              // last value of currentPrefSufLength
    c.soes = p->soes;
    const int seed_nt = std::min(c.Lmin, SEED_MAX_NT);             // candidates are verified over the whole overlap anyway
    c.seed_words = (2 * seed_nt + 31) >> 5;
    c.seed_last_mask = (2 * seed_nt & 31) ? ((1u << (2 * seed_nt & 31)) - 1u) : 0xFFFFFFFFu;
    // The reversal at L == rsoemo (GraphCreatorPrefSuf.cpp:288) only happens if that iteration exists.
    // If rsoemo lies beyond the last iteration every overlap stays "small", the graph is never
    // reversed mid-way and the final reverseGraphInPlace (:107) hands back the REVERSED graph.
    c.reversed = (c.rsoemo > c.Lcap) ? 1 : 0;
    c.stats = p->collect_stats ? 1 : 0;
    out.cfg = c;
    if (p->reduction < ALGA_REDUCTION_AUTO || p->reduction > ALGA_REDUCTION_SOURCE_SIDE)
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "reduction must be an alga_reduction value");
    // preconditions of the source-side reduction (prefsuf_device.h: local_reduce; tests/source_side_rule.py)
    out.local_ok = out.max_len <= p->max_len_cap && out.max_len - c.Lmin <= LOCAL_MAX_SPAN && c.Lmin <= c.rsoemo && c.rsoemo <= c.Lcap &&
                   mask_asym == 0;
    out.local_sw = out.max_len - c.Lmin <= 63 ? 1 : 2;
    // Which probe feeds the source-side form.  The clustered minimizer join (prefsuf_cluster.hip) takes one-word offset masks and
    // rows of up to 13 words; AUTO uses it whenever it takes the input (measured faster than the seed-table probe from 1.7 M
    // nodes, where everything is cache-resident, to 90 M: DESIGN.md section 5c).
    out.cluster_eq = 0;
    // (wide inputs -- more than 64 suffix windows or rows of more than 13 words: 250-bp reads -- go through the clustered probe's general
    // kernel alone; while table and rows fit the caches the seed-table probe is faster there: 3.4 against 3.8 ms at 1.8 M nodes, 19.8 against
    // 15.7 ms at 7.2 M (tools/forms_compare.py ... 250): AUTO takes the clustered probe for them from 4 M live nodes on)
    const bool wide = out.local_sw == 2 || blocks_of(out.max_len) > 13;
    if (out.local_ok && e->opt_probe != ALGA_PROBE_TABLE && !(wide && e->opt_probe == ALGA_PROBE_AUTO && out.live < (4ull << 20))) {
        int eq = 0;
        if (cluster_plan(c, out.max_len, out.live, e->opt_cluster_bucket_bias, &out.cluster, &eq)) out.cluster_eq = eq;
    }
    out.keys_shared = p->keys_shared;
    out.reduction = p->reduction;
    if (out.reduction == ALGA_REDUCTION_AUTO && e->opt_force_per_target) out.reduction = ALGA_REDUCTION_PER_TARGET;
    return ALGA_OK;
}

// buffers of the clustered minimizer join for pp's node set
int cluster_alloc(alga_engine *e, const Prepared &pp) {
    int rc;
    const uint64_t n = (uint64_t) pp.nd.n;
    // keys[0] / meta: ALGA_KEY_ARRAY_SLACK entries of room past n, so that equal-sized all-gather slices may run past the last node
    for (int k = 0; k < 2; k++) {
        if ((rc = alga_ensure(e, e->cl_keys[k], (n + ALGA_KEY_ARRAY_SLACK + 1) * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->cl_vals[k], (n + 1) * sizeof(uint32_t)))) return rc;
    }
    if ((rc = alga_ensure(e, e->cl_meta, (n + ALGA_KEY_ARRAY_SLACK + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->cl_runs, (n + 1) * CL_RMAX * 8))) return rc;
    if ((rc = alga_ensure(e, e->cl_nruns, n + 16))) return rc;
    if ((rc = alga_ensure(e, e->cl_store, (n + 2) * 16 * (size_t) pp.cluster_eq))) return rc;
    if ((rc = alga_ensure(e, e->cl_dir, ((size_t) pp.cluster.n_buckets + 2) * 16))) return rc;
    return alga_ensure(e, e->sort_temp, cluster_sort_temp_bytes(n));
}

// buffers of the pile path (prefsuf_pile.hip).  The bucket table is never cleared between builds -- a record is valid when it carries the
// epoch of the build at hand -- so it is zeroed here when it is (re)allocated, and the epoch starts over.
int pile_alloc(alga_engine *e, uint64_t n, uint32_t n_buckets, hipStream_t s) {
    int rc;
    if ((rc = alga_ensure(e, e->cl_pile_rec, pile_record_bytes(n)))) return rc;
    if ((rc = alga_ensure(e, e->cl_pile_rec2, pile_record_bytes(n)))) return rc;
    if ((rc = alga_ensure(e, e->cl_pile_succ, ((size_t) n + 64) * 16))) return rc;
    if ((rc = alga_ensure(e, e->cl_pile_cnt, PILE_CNT_WORDS * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->cl_pile_own, pile_own_mask_bytes(n)))) return rc;
    if (e->opt_pile_runs_list && (rc = alga_ensure(e, e->cl_pile_list, pile_list_bytes(n)))) return rc;
    if ((rc = alga_ensure(e, e->cl_defer, (size_t) (n + 64) * sizeof(int32_t)))) return rc;      // (the list of own-list ids first, the probe's defer list later)
    const void *before = e->cl_pile_tab.p;
    const size_t cap_before = e->cl_pile_tab.cap;
    if ((rc = alga_ensure(e, e->cl_pile_tab, pile_table_bytes(n_buckets)))) return rc;
    if (e->cl_pile_tab.p != before || e->cl_pile_tab.cap != cap_before) {
        HIP_TRY(e, hipMemsetAsync(e->cl_pile_tab.p, 0, e->cl_pile_tab.cap, s));
        HIP_TRY(e, hipStreamSynchronize(s));               // (once per allocation; the next build may come on another stream)
        e->pile_epoch = 0;
    }
    return ALGA_OK;
}

// seed + probe.  On return e->rec_dst / e->rec_val hold *n_rec record slots (chunk padding included).
// local: source-side reduction inside the probe; the records are then final edges (*overflow: a source exceeded its capacity).
int discover_impl(alga_engine *e, const Prepared &pp, int32_t src_begin, int32_t src_end, hipStream_t s, uint64_t *n_rec, bool local = false,
                  bool *overflow = nullptr) {
    int rc;
    const NodesDev &nd = pp.nd;
    const PrefSufCfg &cfg = pp.cfg;
    unsigned long long *cnt = (unsigned long long *) e->counters.p;
    *n_rec = 0;
    HIP_TRY(e, hipEventRecord(e->ev[EV_START], s));
    if (pp.live >= (1ull << 31)) return alga_fail(e, ALGA_ERR_CAPACITY, "too many nodes for one seed table; shard the input");
    const bool clustered = local && pp.cluster_eq != 0;
    e->pairs_timed = false;
    e->store_timed = false;
    e->pile_timed = false;
    e->pile_deg_pending = false;
    // the probe through piles: all sources in entry order, reads of one length without masks (prefsuf_pile.hip: pile_plan)
    // (a range of ids -- a rank's share of the strong-scaling N-GPU build, option pile_range: the same index, the range's side records compacted for the probe)
    const bool all_sources = src_begin == 0 && src_end == pp.nd.n;
    // (keys_shared = 2, a further piece of a rank's range: the piles of the build before it, where that build made them for this node set)
    const bool pile_index_left = e->opt_pile_range != 0 && e->pile_n == pp.nd.n && e->pile_words == (const void *) pp.nd.words;
    bool pile = clustered && e->opt_pile != 0 && e->opt_cluster_pairs != 0 && e->opt_cluster_order != 0 && pp.local_sw == 1 &&
                      (pp.keys_shared == 0 || (pp.keys_shared == 2 && pile_index_left)) &&
                      (all_sources || (e->opt_pile_range != 0 && src_begin >= 0 && src_end <= pp.nd.n && src_begin < src_end)) && pile_plan(cfg, pp.cluster, pp.cluster_eq, pp.uniform_len, pp.nd.from != nullptr || pp.nd.to != nullptr);
    e->loc_second_used = false;
    bool keys_only = false;                                // the key pass made no run lists (see there)
    const bool need_vals = !e->opt_own_sort || e->opt_test_unsorted_index;
    uint32_t n_buckets = 0, filter_bits = 0;
    bool have_table = false;
    auto build_table = [&]() -> int {                      // bucketised seed table + prefilter of prefsuf_kernels.hip
        n_buckets = seed_buckets_for(pp.live, e->seed_fill_x10);
        const size_t table_bytes = (size_t) n_buckets * SEED_BUCKET * sizeof(unsigned long long);
        int r;
        if ((r = alga_ensure(e, e->table, table_bytes))) return r;
        HIP_TRY(e, hipMemsetAsync(e->table.p, 0xFF, table_bytes, s));
        filter_bits = seed_filter_bits_for(pp.live);
        if (filter_bits) {
            if ((r = alga_ensure(e, e->filter, filter_bits / 8))) return r;
            HIP_TRY(e, hipMemsetAsync(e->filter.p, 0, filter_bits / 8, s));
        }
        launch_seed_build(nd, cfg, (unsigned long long *) e->table.p, n_buckets, (uint32_t *) e->filter.p, filter_bits, s);
        if ((r = alga_check_launch(e, "k_seed_build"))) return r;
        e->stats.table_slots = (uint64_t) n_buckets * SEED_BUCKET;
        have_table = true;
        return ALGA_OK;
    };
    ClusterCfg cc{};
    if (clustered) {
        // targets in minimizer-hash order: sort keys, entry array, bucket index
        cc = pp.cluster;
        if ((rc = cluster_alloc(e, pp))) return rc;
        if (pp.keys_shared == 2) {
            // the entry array, index, directory and runs of the previous build are still what this node set needs (a rank that
            // builds its source range in several pieces so that the gather of one piece overlaps the probe of the next)
            // (a build the pile path kept in its pure form left no entry array and needs none: its piles serve this piece -- the kernels read the
            // sample's verdict from the device as they did then)
            const bool store_left = e->store_n == nd.n && e->store_words == (const void *) nd.words && e->store_eq == pp.cluster_eq && e->store_buckets == cc.n_buckets;
            const bool piles_serve = pile && e->pile_kept_pure && e->store_buckets == cc.n_buckets && e->store_eq == pp.cluster_eq;
            if (!(store_left || piles_serve) || src_begin < e->store_run_begin || src_end > e->store_run_end)
                return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "keys_shared = 2: no entry array of this node set that covers the sources is left from the previous build");
            keys_only = pile && e->pile_keys_only;
        } else {
            int32_t run_begin = 0, run_end = nd.n;
            if (pp.keys_shared == 1) {
                // keys / meta of every node are in place (this rank's share by alga_prefsuf_keys_device, the others' by the caller's
                // all-gather); the runs of this rank's share are what the probe of [src_begin, src_end) reads
                if (e->keyed_n != nd.n || e->keyed_words != (const void *) nd.words || src_begin < e->keyed_begin || src_end > e->keyed_end)
                    return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "keys_shared: alga_prefsuf_keys_device has not been called on this node set for a range that covers the sources");
                run_begin = e->keyed_begin; run_end = e->keyed_end;
            } else {
                // A build the pile path keeps takes its run lists from the piles' consensus (k_pile_runs_consensus): the key pass then computes the
                // TARGET keys alone, and own lists only where one is read (entries outside a first group, sources handed to the general
                // kernel).  Whether the path keeps the build is decided on the device, after the sort: where the build before this one was declined
                // (reads with errors) the full pass runs up front as before; else it follows behind the sample, for a declined build only.
                keys_only = pile && e->opt_pile_runs != 0 && !e->expect_pairwise && !e->opt_pile_check;
                // (the sort payload -- the node ids -- is made up by the engine's own sort in its first pass: nobody writes or reads that array)
                launch_cluster_keys(nd, cfg, cc, 0, nd.n, (uint32_t *) e->cl_keys[0].p, need_vals ? (uint32_t *) e->cl_vals[0].p : nullptr, (uint32_t *) e->cl_meta.p, e->cl_runs.p,
                                    (uint8_t *) e->cl_nruns.p, s, !keys_only);
                if ((rc = alga_check_launch(e, "k_node_runs"))) return rc;
            }
            HIP_TRY(e, hipEventRecord(e->ev[EV_KEYS], s));
            e->keyed_n = -1;                               // the sort below may reuse the key buffers: one build per key pass
            e->store_n = -1;
            HIP_TRY(e, launch_cluster_sort(nd, cc, (uint32_t *) e->cl_keys[0].p, (uint32_t *) e->cl_vals[0].p, (uint32_t *) e->cl_keys[1].p,
                                           (uint32_t *) e->cl_vals[1].p, e->sort_temp.p, cluster_sort_temp_bytes((uint64_t) nd.n), pp.keys_shared == 1 || !need_vals,
                                           e->ev[EV_SORT], e->opt_test_unsorted_index != 0, s, e->opt_own_sort != 0));
            // The bucket directory.  With option pile_dir >= 1 the pile path's sample does not read it and comes first; with pile_dir = 2 the fill and
            // k_tgt_dir then read the sample's verdict and leave at once for a build the path keeps in its pure form: its pile kernels take the bucket
            // records from the keys, the pairwise kernels behind them (the by-id instances, which alone run for that form) from the piles' table
            // (bucket_record).  That needs every pairwise kernel of such a build to be a by-id instance: pile_skip_gather, no statistics build.
            const bool dir_late = pile && e->opt_pile_dir >= 1;
            e->dir_late = dir_late;
            if (!dir_late) {
                HIP_TRY(e, launch_cluster_dir(nd, cc, (const uint32_t *) e->cl_keys[1].p, e->cl_dir.p, cnt + CNT_TOTAL + 1, nullptr, s));
                HIP_TRY(e, hipEventRecord(e->ev[EV_DIR], s));
            }
            e->pile_n = -1;
            if (pile) {
                // piles of the key order: belong to the index (a function of the targets alone), read by k_pile_probe.  The sample first: a
                // build the pile path keeps has no use for the entry array, and k_tgt_gather reads the sample's two counters like the probes do
                rc = e->opt_test_pile_oom ? alga_fail(e, ALGA_ERR_OUT_OF_MEMORY, "pile_alloc (option test_pile_oom)") : pile_alloc(e, (uint64_t) nd.n, cc.n_buckets, s);
                if (rc == ALGA_ERR_OUT_OF_MEMORY) {
                    // the pile path needs ~180 B per node on top of the pairwise kernels' buffers (bucket table, group records, side records): an input
                    // that fitted without it must not fail because of it.  Give back what was allocated of it and take the pairwise kernels.
                    (void) hipGetLastError();
                    alga_release(e->cl_pile_tab); alga_release(e->cl_pile_rec); alga_release(e->cl_pile_rec2); alga_release(e->cl_pile_succ); alga_release(e->cl_pile_own);
                    alga_release(e->cl_pile_list);
                    e->pile_epoch = 0; e->pile_n = -1;
                    e->err.clear();
                    pile = false;
                    rc = ALGA_OK;
                    if (keys_only) {                       // the pairwise kernels read every node's run list
                        launch_cluster_keys(nd, cfg, cc, 0, nd.n, (uint32_t *) e->cl_keys[0].p, (uint32_t *) e->cl_vals[0].p, (uint32_t *) e->cl_meta.p, e->cl_runs.p,
                                            (uint8_t *) e->cl_nruns.p, s, true);
                        if ((rc = alga_check_launch(e, "k_node_runs"))) return rc;
                        keys_only = false;
                    }
                } else if (rc) return rc;
            }
            if (pile) {
                launch_pile_sample(nd, cc, pp.uniform_len, (const uint32_t *) e->cl_keys[1].p, (const uint32_t *) e->cl_vals[1].p, e->cl_dir.p,
                                   (unsigned long long *) e->cl_pile_cnt.p, e->opt_pile >= 2 ? e->opt_pile - 1 : 0, s, e->opt_pile_dir >= 1);
                if ((rc = alga_check_launch(e, "k_pile_build<sample>"))) return rc;
            }
            e->pile_tab_index = pile && e->opt_pile_dir >= 2 && e->opt_pile_skip_gather && !cfg.stats;
            if (dir_late) {
                HIP_TRY(e, hipEventRecord(e->ev[EV_SAMPLE], s));
                HIP_TRY(e, launch_cluster_dir(nd, cc, (const uint32_t *) e->cl_keys[1].p, e->cl_dir.p, cnt + CNT_TOTAL + 1,
                                              e->pile_tab_index ? (const unsigned long long *) e->cl_pile_cnt.p : nullptr, s));
                HIP_TRY(e, hipEventRecord(e->ev[EV_DIR], s));
            }
            HIP_TRY(e, launch_cluster_gather(nd, cc, pp.cluster_eq, (const uint32_t *) e->cl_keys[1].p, (const uint32_t *) e->cl_vals[1].p, (const uint32_t *) e->cl_meta.p,
                                             pp.uniform_len, e->cl_store.p, (pile && e->opt_pile_skip_gather) ? (const unsigned long long *) e->cl_pile_cnt.p : nullptr, s));
            HIP_TRY(e, hipEventRecord(e->ev[EV_GATHER], s));
            if (pile) {
                if (e->pile_epoch >= 511u) {               // the epoch (9 bits of a record) wraps: every record of the table becomes "empty" again
                    HIP_TRY(e, hipMemsetAsync(e->cl_pile_tab.p, 0, e->cl_pile_tab.cap, s));
                    e->pile_epoch = 0;
                }
                e->pile_epoch++;
                const bool from_consensus = e->opt_pile_runs != 0;
                launch_pile_build(nd, cfg, cc, pp.uniform_len, (const uint32_t *) e->cl_keys[1].p, (const uint32_t *) e->cl_vals[1].p, e->cl_dir.p, e->cl_pile_rec.p, e->cl_pile_rec2.p, e->cl_pile_tab.p,
                                  e->pile_epoch, e->cl_pile_succ.p, e->cl_runs.p, pp.uniform_len - cfg.Lmin + 1, (const unsigned long long *) e->cl_pile_cnt.p,
                                  from_consensus ? (uint32_t *) e->cl_pile_own.p : nullptr, (from_consensus && e->opt_pile_runs_list) ? e->cl_pile_list.p : nullptr, s,
                                  e->opt_pile_dir >= 1, cnt + CNT_TOTAL + 1, e->pile_tab_index, e->opt_pile_runs_ahead != 0);
                if ((rc = alga_check_launch(e, "k_pile_build"))) return rc;
                if (keys_only) {
                    // own run lists of the entries outside a first group (6 % at the north-star size) ...
                    launch_pile_own_ids((const uint32_t *) e->cl_pile_own.p, (const uint32_t *) e->cl_vals[1].p, (uint64_t) nd.n, (int32_t *) e->cl_defer.p, (uint32_t) nd.n,
                                        (unsigned long long *) e->cl_pile_cnt.p, s);
                    launch_cluster_runs_list(nd, cfg, cc, (const int32_t *) e->cl_defer.p, (const unsigned long long *) e->cl_pile_cnt.p + 3, (uint32_t) nd.n, (uint32_t) e->n_cu * 16u,
                                             e->cl_runs.p, (uint8_t *) e->cl_nruns.p, s);
                    // ... and every node's, after all, for a build the sample hands to the pairwise kernels
                    launch_cluster_keys(nd, cfg, cc, 0, nd.n, (uint32_t *) e->cl_keys[0].p, (uint32_t *) e->cl_vals[0].p, (uint32_t *) e->cl_meta.p, e->cl_runs.p,
                                        (uint8_t *) e->cl_nruns.p, s, true, (const unsigned long long *) e->cl_pile_cnt.p);
                    if ((rc = alga_check_launch(e, "k_node_runs (own lists)"))) return rc;
                }
                if (e->opt_pile_check && from_consensus)
                    launch_pile_check(e->cl_pile_succ.p, (uint64_t) nd.n, cc.n_buckets, e->cl_pile_tab.p, e->cl_pile_rec2.p, e->pile_epoch, e->cl_runs.p, nd.n, pp.uniform_len - cfg.Lmin + 1,
                                      (unsigned long long *) e->cl_pile_cnt.p, s);
                e->pile_n = nd.n; e->pile_words = (const void *) nd.words;
                e->pile_keys_only = keys_only; e->pile_kept_pure = false;            // (the verdict: after the probe)
                e->pile_timed = nd.n > 0;
            }
            e->store_timed = nd.n > 0;
            e->store_n = pile ? -1 : nd.n;                   // (a build the pile path may have kept -- decided on the device -- leaves no entry array for keys_shared = 2)
            e->store_words = (const void *) nd.words; e->store_eq = pp.cluster_eq; e->store_buckets = cc.n_buckets;
            e->store_run_begin = run_begin; e->store_run_end = run_end;
        }
        e->stats.table_slots = cc.n_buckets;
    } else if ((rc = build_table())) return rc;
    HIP_TRY(e, hipEventRecord(e->ev[EV_SEED], s));

    const uint64_t n_src = (uint64_t) std::max<int64_t>(0, (int64_t) src_end - src_begin);
    const uint64_t slack = std::max(probe_record_slack(e->n_cu, n_src, local), clustered ? cluster_record_slack(e->n_cu, n_src) : 0);   // invalid padding of the chunked record list
    uint64_t &hint = local ? e->rec_cap_hint_local : e->rec_cap_hint;
    uint64_t cap = std::max<uint64_t>(hint, (local ? 2 : 16) * n_src + 4096) + slack;
    if (local) {
        if ((rc = alga_ensure(e, e->outdeg, (size_t) (n_src + 1) * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->loc_first, (size_t) (n_src + 1) * sizeof(unsigned long long)))) return rc;
    }
    const uint32_t big_list_cap = 1u << 20;
    if (local && (rc = alga_ensure(e, e->loc_big_list, big_list_cap * sizeof(int32_t)))) return rc;
    bool pure_streamed = false;                            // a build of the pure pile form sent its handed-on sources through k_probe_stream as well (option pile_stream_by_id)
    for (int attempt = 0; attempt < 4; attempt++) {
        if (cap >= (1ull << 32) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 overlap records; shard the input");
        if (local) HIP_TRY(e, hipMemsetAsync(e->outdeg.p, 0, (size_t) (n_src + 1) * sizeof(uint32_t), s));
        if ((rc = alga_ensure(e, e->rec_dst, cap * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->rec_val, cap * sizeof(unsigned long long)))) return rc;
        HIP_TRY(e, hipMemsetAsync(cnt, 0, CNT_TOTAL * sizeof(unsigned long long), s));
        ProbeBig big{(int32_t *) e->loc_big_list.p, big_list_cap, 0u, nullptr, 0u};
        e->defer_list_valid = clustered && e->opt_cluster_pairs && pp.local_sw == 1 && pp.cluster_eq <= 4;           // k_probe_stream first: every source with records is on cl_defer (finalize_local)
        if (clustered) {
            // Two kernels: k_probe_stream (the entries of consecutive sources packed densely onto the lanes) finishes the regular sources
            // and lists the others; the general kernel (one source per wave, any shape) takes the list.  No host round trip in between:
            // the general kernel runs as a persistent grid over a list whose length it reads from the device counter the first
            // kernel left.  Data on which most sources are irregular (sequencing errors: several items per offset): the waves of the
            // first kernel notice it on their own first sources and hand the rest of their share on unseen -- a decision taken from
            // THIS build's data, not from an earlier build.
            if (e->opt_cluster_pairs && pp.local_sw == 1 && pp.cluster_eq <= 4) {      // (k_probe_stream: one-word offset masks, rows of up to 13 words)
                if ((rc = alga_ensure(e, e->cl_defer, (size_t) (n_src + 64) * sizeof(int32_t)))) return rc;
                // (LOCAL_SLOTS_MAX - 1 further slots per source: k_probe_stream finishes sources with up to four standing items -- option stream_slots = 2: two, as until round 4)
                const uint32_t slot_stride = e->opt_stream_slots >= 4 ? (uint32_t) (n_src + 1) : 0u;
                if ((rc = alga_ensure(e, e->loc_second, (size_t) (slot_stride ? LOCAL_SLOTS_MAX - 1 : 1) * (n_src + 1) * sizeof(unsigned long long)))) return rc;
                e->loc_second_used = true;
                e->loc_slot_stride = slot_stride;
                // all sources: in the order of the entry array (consecutive sources share a locus: option cluster_order); a range of
                // ids (a rank's share, a piece): in id order
                const bool by_key = e->opt_cluster_order != 0 && src_begin == 0 && src_end == nd.n;
                const bool piled = pile && e->pile_n == nd.n && e->pile_words == (const void *) nd.words;
                if (piled) {
                    if (!all_sources) {
                        if ((rc = alga_ensure(e, e->cl_pile_side_r, (size_t) (n_src + 64) * 16))) return rc;
                        if ((rc = alga_ensure(e, e->cl_pile_cursor, 64))) return rc;
                    }
                    // k_pile_probe first; it and k_probe_stream read the same two counters k_pile_build left and exactly one of them works
                    launch_pile_probe(nd, cfg, cc, pp.uniform_len, e->cl_pile_tab.p, e->pile_epoch, e->cl_pile_rec.p, e->cl_pile_rec2.p, e->cl_pile_succ.p,
                                      e->cl_runs.p, cnt, (uint32_t *) e->outdeg.p, (unsigned long long *) e->loc_first.p, (unsigned long long *) e->loc_second.p,
                                      (int32_t *) e->cl_defer.p, (uint32_t) n_src, (const unsigned long long *) e->cl_pile_cnt.p, e->n_cu, s, src_begin, src_end,
                                      e->cl_pile_side_r.p, (unsigned long long *) e->cl_pile_cursor.p, e->opt_pile_probe_lean != 0, e->opt_pile_probe_tail != 0);
                    if ((rc = alga_check_launch(e, "k_pile_probe"))) return rc;
                    // the sources it handed on have no run list of their own yet (the general kernel reads it): a list-driven key pass over the
                    // defer list, whose length the device knows
                    if (keys_only)
                        launch_cluster_runs_list(nd, cfg, cc, (const int32_t *) e->cl_defer.p, cnt + CNT_DEFERRED, (uint32_t) std::min<uint64_t>(n_src + 64, 0xFFFFFFFFull),
                                                 (uint32_t) e->n_cu * 16u, e->cl_runs.p, (uint8_t *) e->cl_nruns.p, s);
                }
                launch_probe_stream(nd, cfg, cc, pp.cluster_eq, e->cl_store.p, e->cl_dir.p, e->cl_runs.p, (const uint8_t *) e->cl_nruns.p,
                                    src_begin, src_end, by_key, cnt, e->n_cu, (uint32_t *) e->outdeg.p, (unsigned long long *) e->loc_first.p,
                                    (unsigned long long *) e->loc_second.p, (int32_t *) e->cl_defer.p, (uint32_t) n_src,
                                    piled ? (const unsigned long long *) e->cl_pile_cnt.p : nullptr, s, slot_stride);
                if ((rc = alga_check_launch(e, "k_probe_stream"))) return rc;
                if (piled) {
                    // the MIXED form (more than one irregular bucket in 250, not more than one in 20 -- the kernels read the sample's counters themselves):
                    // what k_pile_probe handed on goes through the stream kernel, by list, before the general kernel gets what is left; the PURE form
                    // too (option pile_stream_by_id), with the entries taken by id from the sorted (key, id) pairs -- it has no entry array
                    if ((rc = alga_ensure(e, e->cl_defer2, (size_t) (n_src + 64) * sizeof(int32_t)))) return rc;
                    pure_streamed = launch_probe_stream_list(nd, cfg, cc, pp.cluster_eq, e->cl_store.p, e->cl_dir.p, e->cl_runs.p, (const uint8_t *) e->cl_nruns.p, (int32_t *) e->cl_defer.p,
                                             (uint32_t) n_src, cnt, e->n_cu, (uint32_t *) e->outdeg.p, (unsigned long long *) e->loc_first.p,
                                             (unsigned long long *) e->loc_second.p, (int32_t *) e->cl_defer2.p, (const unsigned long long *) e->cl_pile_cnt.p, s, slot_stride, src_begin,
                                             (const uint32_t *) e->cl_keys[1].p, (const uint32_t *) e->cl_vals[1].p, pp.uniform_len, e->opt_pile_stream_by_id != 0,
                                             e->pile_tab_index ? e->cl_pile_tab.p : nullptr, e->pile_epoch);
                    if ((rc = alga_check_launch(e, "k_probe_stream (list)"))) return rc;
                }
                HIP_TRY(e, hipEventRecord(e->ev[EV_PAIRS], s));
                e->pairs_timed = true;
                launch_probe_clustered(nd, cfg, cc, pp.cluster_eq, e->cl_store.p, e->cl_dir.p, e->cl_runs.p, (const uint8_t *) e->cl_nruns.p, 0,
                                       (int32_t) n_src, (const int32_t *) e->cl_defer.p, src_begin, (uint32_t *) e->rec_dst.p, (unsigned long long *) e->rec_val.p,
                                       cap, cnt, e->n_cu, (uint32_t *) e->outdeg.p, (unsigned long long *) e->loc_first.p, &big, cnt + CNT_DEFERRED, 1, s,
                                       (const uint32_t *) e->cl_keys[1].p, (const uint32_t *) e->cl_vals[1].p, pp.uniform_len,
                                       (piled && e->opt_pile_skip_gather) ? (const unsigned long long *) e->cl_pile_cnt.p : nullptr,
                                       (piled && e->pile_tab_index) ? e->cl_pile_tab.p : nullptr, e->pile_epoch);
                // the out-degrees k_pile_probe left in the slots: moved to outdeg by the first pass of finalize_local's scan (option pile_deg_fold), or here
                e->pile_deg_pending = piled && e->opt_pile_deg_fold != 0;
                if (piled && !e->pile_deg_pending) launch_pile_deg((int32_t) n_src, (unsigned long long *) e->loc_first.p, (uint32_t *) e->outdeg.p, (const unsigned long long *) e->cl_pile_cnt.p, s);
            } else {
                launch_probe_clustered(nd, cfg, cc, pp.cluster_eq, e->cl_store.p, e->cl_dir.p, e->cl_runs.p, (const uint8_t *) e->cl_nruns.p, src_begin,
                                       src_end, nullptr, src_begin, (uint32_t *) e->rec_dst.p, (unsigned long long *) e->rec_val.p, cap, cnt, e->n_cu,
                                       (uint32_t *) e->outdeg.p, (unsigned long long *) e->loc_first.p, &big, nullptr, pp.local_sw, s);
            }
        }
        else
            launch_probe(nd, cfg, (const unsigned long long *) e->table.p, n_buckets, (const uint32_t *) e->filter.p, filter_bits, src_begin, src_end,
                         (uint32_t *) e->rec_dst.p, (unsigned long long *) e->rec_val.p, cap, cnt, e->n_cu, local ? pp.local_sw : 0, (uint32_t *) e->outdeg.p,
                         (unsigned long long *) e->loc_first.p, local ? &big : nullptr, s);
        if ((rc = alga_check_launch(e, "k_probe_sources"))) return rc;
        HIP_TRY(e, hipEventRecord(e->ev[EV_PROBE], s));
        HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, (CNT_TOTAL + 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipStreamSynchronize(s));
        if (clustered && e->h_counters[CNT_TOTAL + 1] != 0) {
            // k_tgt_dir found the sorted key array out of order (a sort that did not sort): the directory describes nothing.  The probe
            // clamps its entry reads, so nothing faulted; nothing it produced is used either.
            e->store_n = -1; e->keyed_n = -1;
            return alga_fail(e, ALGA_ERR_HIP, "clustered index: the sorted key array is not in order (entry directory invalid)");
        }
        if (local && e->h_counters[CNT_LOCAL_OVERFLOW] != 0) {
            // Some sources have more raw overlaps than a wave's LDS holds (repeat-rich input): the first pass listed them, a second
            // pass probes exactly those with their items in a global slice per wave.  Too many of them, or too many overlaps for the
            // largest slice the engine allocates: the caller takes the per-target pipeline.
            const uint64_t n_big = e->h_counters[CNT_LOCAL_OVERFLOW], max_items = e->h_counters[CNT_LOCAL_MAXITEMS];
            const uint64_t limit = e->big_limit >= 0 ? (uint64_t) e->big_limit : (uint64_t) local_big_limit();
            if (n_big > big_list_cap || max_items > limit) { if (overflow) *overflow = true; *n_rec = 0; return ALGA_OK; }
            big.count = (uint32_t) n_big;
            big.item_cap = (uint32_t) ((max_items + 63) & ~63ull);
            if ((rc = alga_ensure(e, e->loc_big_items, probe_big_bytes(e->n_cu, big.count, pp.local_sw, big.item_cap)))) return rc;
            big.items = e->loc_big_items.p;
            if (!have_table && (rc = build_table())) return rc;            // the second pass probes through the seed table
            if (e->pile_deg_pending) {                     // (the second pass finds the out-degrees where the first pass's kernels leave them)
                launch_pile_deg((int32_t) n_src, (unsigned long long *) e->loc_first.p, (uint32_t *) e->outdeg.p, (const unsigned long long *) e->cl_pile_cnt.p, s);
                e->pile_deg_pending = false;
            }
            HIP_TRY(e, hipMemsetAsync(cnt + CNT_LOCAL_OVERFLOW, 0, sizeof(unsigned long long), s));
            launch_probe(nd, cfg, (const unsigned long long *) e->table.p, n_buckets, (const uint32_t *) e->filter.p, filter_bits, src_begin, src_end,
                         (uint32_t *) e->rec_dst.p, (unsigned long long *) e->rec_val.p, cap, cnt, e->n_cu, pp.local_sw, (uint32_t *) e->outdeg.p,
                         (unsigned long long *) e->loc_first.p, &big, s);
            if ((rc = alga_check_launch(e, "k_probe_sources (second pass)"))) return rc;
            HIP_TRY(e, hipEventRecord(e->ev[EV_PROBE], s));
            HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, CNT_TOTAL * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
            HIP_TRY(e, hipStreamSynchronize(s));
            if (e->h_counters[CNT_LOCAL_OVERFLOW] != 0) { if (overflow) *overflow = true; *n_rec = 0; return ALGA_OK; }
            e->stats.big_sources = n_big;
        }
        const uint64_t need = e->h_counters[CNT_RECORDS];
        if (need <= cap) {
            *n_rec = need;
            hint = std::max<uint64_t>(hint, need + need / 16 + 4096);
            if (overflow) *overflow = false;
            if (local) { e->stats.transitive_compares = e->h_counters[CNT_TR_COMPARES]; e->stats.generic_sources = e->h_counters[CNT_LOCAL_GENERIC]; }
            e->stats.records = e->h_counters[CNT_VALID_RECORDS];
            e->stats.raw_overlaps = e->h_counters[CNT_RAW];
            e->stats.windows_probed = e->h_counters[CNT_WINDOWS];
            e->stats.slots_scanned = e->h_counters[CNT_SLOTS];
            e->stats.probe_rounds = e->h_counters[CNT_ROUNDS];
            e->stats.pile_buckets = e->h_counters[CNT_PILE_BUCKETS]; e->stats.pile_irregular = e->h_counters[CNT_PILE_IRREGULAR];
            e->stats.pile_own_lists = e->h_counters[CNT_PILE_OWN];
            if (pile && pp.keys_shared != 2 && e->pile_n == nd.n) {
                // the sample's verdict is on the host now: a build the pile path DECLINED (or one with pile_skip_gather off) did build the entry
                // array, and a later keys_shared = 2 build of this node set may use it
                const bool kept = e->opt_pile == 2 || e->stats.pile_irregular * (uint64_t) ALGA_PILE_DECLINE_ONE_IN <= e->stats.pile_buckets;
                e->stats.pile_mixed = kept && e->stats.pile_irregular * (uint64_t) ALGA_PILE_IRREGULAR_ONE_IN > e->stats.pile_buckets;
                e->stats.pile_deferred = (e->stats.pile_mixed || (kept && pure_streamed)) ? e->h_counters[CNT_DEFERRED_PILE] : (kept ? e->h_counters[CNT_DEFERRED] : 0);
                if (!kept || e->stats.pile_mixed || !e->opt_pile_skip_gather) e->store_n = nd.n;      // (the entry array was built: k_tgt_gather leaves only for a build of the pure pile form)
                e->expect_pairwise = !kept;               // (how the NEXT build's key pass is laid out -- never what it computes)
                e->pile_kept_pure = kept && !e->stats.pile_mixed && e->opt_pile_skip_gather != 0;
                e->stats.pile_list_checked = 0; e->stats.pile_list_mismatch = 0;
                if (e->opt_pile_check) {
                    unsigned long long chk[2] = {0ull, 0ull};
                    HIP_TRY(e, hipMemcpyAsync(chk, (const unsigned long long *) e->cl_pile_cnt.p + 4, sizeof(chk), hipMemcpyDeviceToHost, s));
                    HIP_TRY(e, hipStreamSynchronize(s));
                    e->stats.pile_list_checked = chk[0]; e->stats.pile_list_mismatch = chk[1];
                }
            }
            if (!pile) e->expect_pairwise = false;
            e->stats.probe_used = clustered ? ALGA_PROBE_CLUSTER : ALGA_PROBE_TABLE;
            if (clustered) e->stats.deferred_sources = e->defer_list_valid ? e->h_counters[CNT_DEFERRED] : n_src;
            return ALGA_OK;
        }
        cap = need + need / 16 + 4096 + slack; // the cursor kept counting past the capacity: the need is known
    }
    return alga_fail(e, ALGA_ERR_HIP, "record buffer kept overflowing");
}

int key_bits_for(int64_t n_owned) {   // valid keys are < n_owned; the invalid key (all ones) must sort behind them
    int b = 1;
    while (b < 31 && (1ll << b) < n_owned) b++;
    return std::min(32, b + 1);
}

// group (sort by target) + reduce + emit for the targets in [dst_begin, dst_end)
int reduce_impl(alga_engine *e, const Prepared &pp, const uint32_t *rec_dst, const unsigned long long *rec_val, uint64_t n_rec,
                uint64_t n_valid_hint, int32_t dst_begin, int32_t dst_end, hipStream_t s, uint64_t *n_edges) {
    int rc;
    const NodesDev &nd = pp.nd;
    const PrefSufCfg &cfg = pp.cfg;
    unsigned long long *cnt = (unsigned long long *) e->counters.p;
    const int32_t n_owned = dst_end - dst_begin;
    *n_edges = 0;
    if (n_rec >= (1ull << 32) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 overlap records; shard the input");
    const int bits = key_bits_for(n_owned);
    const size_t temp_bytes = sort_records_temp_bytes(n_rec, bits);
    if ((rc = alga_ensure(e, e->keys, (size_t) (n_rec + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->seg_key, (size_t) (n_rec + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->seg_val, (size_t) (n_rec + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->sort_temp, temp_bytes))) return rc;
    if ((rc = alga_ensure(e, e->heads, (size_t) (n_rec + 1) * 16))) return rc;
    if ((rc = alga_ensure(e, e->rowptr, (size_t) (n_owned + 2) * sizeof(uint32_t)))) return rc;
    HIP_TRY(e, hipMemsetAsync(cnt + CNT_SORT_VALID, 0, sizeof(unsigned long long), s));
    launch_make_keys(rec_dst, n_rec, dst_begin, dst_end, (uint32_t *) e->keys.p, cnt + CNT_SORT_VALID, s);
    if ((rc = alga_check_launch(e, "k_make_keys"))) return rc;
    HIP_TRY(e, sort_records(e->sort_temp.p, temp_bytes, (const uint32_t *) e->keys.p, (uint32_t *) e->seg_key.p, rec_val,
                            (unsigned long long *) e->seg_val.p, n_rec, bits, s));
    launch_rowptr_from_sorted((const uint32_t *) e->seg_key.p, cnt + CNT_SORT_VALID, n_rec, n_owned, (uint32_t *) e->rowptr.p, s);
    if ((rc = alga_check_launch(e, "k_rowptr_from_sorted"))) return rc;
    launch_gather_heads(nd, (const unsigned long long *) e->seg_val.p, cnt + CNT_SORT_VALID, n_rec, e->heads.p, s);
    if ((rc = alga_check_launch(e, "k_gather_heads"))) return rc;
    HIP_TRY(e, hipEventRecord(e->ev[EV_GROUP], s));

    if ((rc = alga_ensure(e, e->out_cnt, (size_t) (n_owned + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->outdeg, (size_t) (nd.n + 1) * sizeof(uint32_t)))) return rc;
    HIP_TRY(e, hipMemsetAsync(e->outdeg.p, 0, (size_t) (nd.n + 1) * sizeof(uint32_t), s));
    const int tpb = reduce_targets_per_block(n_valid_hint, (uint64_t) std::max(1, n_owned));
    launch_reduce_targets(nd, cfg, dst_begin, n_owned, tpb, (const uint32_t *) e->rowptr.p, (unsigned long long *) e->seg_val.p,
                          e->heads.p, (uint32_t *) e->out_cnt.p, (uint32_t *) e->outdeg.p, cnt, s);
    if ((rc = alga_check_launch(e, "k_reduce_targets"))) return rc;
    HIP_TRY(e, hipEventRecord(e->ev[EV_REDUCE], s));

    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes((uint64_t) nd.n)))) return rc;
    if ((rc = alga_ensure(e, e->out_rowptr, (size_t) (nd.n + 1) * sizeof(uint32_t)))) return rc;
    launch_exclusive_scan((const uint32_t *) e->outdeg.p, (uint64_t) nd.n, (uint32_t *) e->out_rowptr.p, (uint64_t *) e->scan_scratch.p, s);
    if ((rc = alga_check_launch(e, "scan(outdeg)"))) return rc;
    uint64_t *d_total = (uint64_t *) e->scan_scratch.p + scan_total_index((uint64_t) nd.n);
    HIP_TRY(e, hipMemcpyAsync(&e->h_counters[CNT_TOTAL], d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(e->h_counters, cnt, CNT_TOTAL * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t E = e->h_counters[CNT_TOTAL];
    if (E >= (1ull << 32) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 edges; shard the input");
    if ((rc = alga_ensure(e, e->edges, (size_t) (E + 1) * sizeof(alga_edge_dev)))) return rc;
    launch_scatter_by_source(cfg, dst_begin, n_owned, (const uint32_t *) e->rowptr.p, (const unsigned long long *) e->seg_val.p,
                             (const uint32_t *) e->out_cnt.p, (const uint32_t *) e->out_rowptr.p, (uint32_t *) e->outdeg.p,
                             (alga_edge_dev *) e->edges.p, s);
    if ((rc = alga_check_launch(e, "k_scatter_by_source"))) return rc;
    launch_sort_rows(nd.n, (const uint32_t *) e->out_rowptr.p, (alga_edge_dev *) e->edges.p, s);
    if ((rc = alga_check_launch(e, "k_sort_rows"))) return rc;
    HIP_TRY(e, hipEventRecord(e->ev[EV_EMIT], s));
    HIP_TRY(e, hipStreamSynchronize(s));
    *n_edges = E;
    e->stats.edges = E;
    e->stats.transitive_listed = e->h_counters[CNT_TR_LISTED];
    e->stats.transitive_compares = e->h_counters[CNT_TR_COMPARES];
    e->stats.transitive_removed = e->h_counters[CNT_TR_REMOVED];
    e->stats.max_in_records = e->h_counters[CNT_MAX_IN];
    return ALGA_OK;
}

// source-side reduction: adjacency lists from the out-degrees, one-edge slots and record list the probe left behind
int finalize_local(alga_engine *e, const Prepared &pp, int32_t src_begin, int32_t src_end, uint64_t n_rec, hipStream_t s, uint64_t *n_edges) {
    int rc;
    *n_edges = 0;
    const uint64_t n_src = (uint64_t) std::max<int64_t>(0, (int64_t) src_end - src_begin);
    if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(n_src)))) return rc;
    if ((rc = alga_ensure(e, e->out_rowptr, (size_t) (n_src + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->out_cnt, (size_t) (n_src + 1) * sizeof(uint32_t)))) return rc;
    HIP_TRY(e, hipEventRecord(e->ev[EV_GROUP], s));
    HIP_TRY(e, hipEventRecord(e->ev[EV_REDUCE], s));
    // option emit_fused: the scan and the slot edges in two passes over the slots (launch_local_emit); 0: the scan first, as until round 8
    const bool fused = e->opt_emit_fused != 0;
    const unsigned long long *pile_cnt = e->pile_deg_pending ? (const unsigned long long *) e->cl_pile_cnt.p : nullptr;      // (not pending: k_pile_deg has moved the out-degrees, or no pile kernel ran)
    if (!fused) {
        if (e->pile_deg_pending)
            launch_exclusive_scan_pile_deg((uint32_t *) e->outdeg.p, n_src, (uint32_t *) e->out_rowptr.p, (uint64_t *) e->scan_scratch.p, (unsigned long long *) e->loc_first.p, pile_cnt, s);
        else
            launch_exclusive_scan((const uint32_t *) e->outdeg.p, n_src, (uint32_t *) e->out_rowptr.p, (uint64_t *) e->scan_scratch.p, s);
        if ((rc = alga_check_launch(e, "scan(outdeg)"))) return rc;
    }
    e->pile_deg_pending = false;
    const uint64_t E = e->stats.records;                                   // CNT_VALID_RECORDS of the probe == sum of the out-degrees (launch_local_emit zeroes the cursors it needs)
    if (E >= (1ull << 32) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 edges; shard the input");
    if ((rc = alga_ensure(e, e->edges, (size_t) (E + 1) * sizeof(alga_edge_dev)))) return rc;
    launch_local_emit(src_begin, (int32_t) n_src, (const uint32_t *) e->outdeg.p, (const unsigned long long *) e->loc_first.p,
                      e->loc_second_used ? (const unsigned long long *) e->loc_second.p : nullptr, (const uint32_t *) e->rec_dst.p, (const unsigned long long *) e->rec_val.p, n_rec, (uint32_t *) e->out_rowptr.p,
                      (uint32_t *) e->out_cnt.p, (alga_edge_dev *) e->edges.p,
                      e->defer_list_valid ? (const int32_t *) e->cl_defer.p : nullptr, (const unsigned long long *) e->counters.p + CNT_DEFERRED, (uint32_t) n_src, s,
                      e->loc_second_used ? e->loc_slot_stride : 0u, fused ? (uint64_t *) e->scan_scratch.p : nullptr, fused ? pile_cnt : nullptr);
    if ((rc = alga_check_launch(e, "k_local_emit"))) return rc;
    HIP_TRY(e, hipEventRecord(e->ev[EV_EMIT], s));
    uint64_t *d_total = (uint64_t *) e->scan_scratch.p + scan_total_index(n_src);
    HIP_TRY(e, hipMemcpyAsync(&e->h_counters[CNT_TOTAL], d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (e->h_counters[CNT_TOTAL] != E) return alga_fail(e, ALGA_ERR_HIP, "source-side emit: out-degrees and edge count disagree");
    *n_edges = E;
    e->stats.edges = E;
    return ALGA_OK;
}

// Source-side form for the sources [src_begin, src_end): ALGA_ERR_UNSUPPORTED when it is not exact for the input.
int build_local(alga_engine *e, const Prepared &pp, int32_t src_begin, int32_t src_end, hipStream_t s, uint64_t *n_edges) {
    if (!pp.local_ok) return alga_fail(e, ALGA_ERR_UNSUPPORTED, "source-side reduction is not exact for this input (read lengths / masks / rsoemo)");
    uint64_t n_rec = 0;
    bool overflow = false;
    int rc = discover_impl(e, pp, src_begin, src_end, s, &n_rec, true, &overflow);
    if (rc) return rc;
    if (overflow) return alga_fail(e, ALGA_ERR_UNSUPPORTED, "a source node has more raw overlaps than the source-side reduction holds");
    if ((rc = finalize_local(e, pp, src_begin, src_end, n_rec, s, n_edges))) return rc;
    e->stats.reduction_used = ALGA_REDUCTION_SOURCE_SIDE;
    return ALGA_OK;
}

double now_ms_host() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

float ev_ms(alga_engine *e, int a, int b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e->ev[a], e->ev[b]) != hipSuccess) return 0.f;
    return ms;
}

// the parts of the index build of the clustered probe (what ms_seed is made of)
void store_phase_stats(alga_engine *e) {
    if (!e->store_timed) return;
    e->stats.ms_keys = ev_ms(e, EV_START, EV_KEYS);
    e->stats.ms_sort = ev_ms(e, EV_KEYS, EV_SORT);
    // (option pile_dir >= 1: the sample runs between the sort and the directory pass; it stays with the gather phase)
    e->stats.ms_dir = ev_ms(e, e->dir_late ? EV_SAMPLE : EV_SORT, EV_DIR);
    e->stats.ms_gather = ev_ms(e, EV_DIR, EV_GATHER) + (e->dir_late ? ev_ms(e, EV_SORT, EV_SAMPLE) : 0.0);      // (with the pile path's sample in front of k_tgt_gather: all there is of this phase when that path keeps the build)
    e->stats.ms_pile = e->pile_timed ? ev_ms(e, EV_GATHER, EV_SEED) : 0.0;
}

} // namespace

// for engine_shard.hip (the bucket-sharded N-GPU build shares the argument checks, the node statistics and the key buffers)
int alga_prepare(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, hipStream_t s, AlgaPrepared &out) { return prepare(e, nodes, p, s, out); }
int alga_cluster_alloc(alga_engine *e, const AlgaPrepared &pp) { return cluster_alloc(e, pp); }

// ============================================================================================
// C ABI
// ============================================================================================
extern "C" {

int alga_abi_version(void) { return ALGA_AMD_ABI_VERSION; }

// the caller's current HIP device stays what it was across create / destroy (the engine sets its own device in every call that
// needs it; a host program with several GPUs must not find its device switched by a library call)
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void) hipSetDevice(prev); }
};

static void engine_free_handles(alga_engine *e) {
    if (e->h_counters) (void) hipHostFree(e->h_counters);
    for (int i = 0; i < EV_COUNT; i++) if (e->ev[i]) (void) hipEventDestroy(e->ev[i]);
    if (e->own_stream) (void) hipStreamDestroy(e->own_stream);
    if (e->side_stream) (void) hipStreamDestroy(e->side_stream);
    if (e->ev_side) (void) hipEventDestroy(e->ev_side);
    e->h_counters = nullptr; e->own_stream = nullptr; e->side_stream = nullptr; e->ev_side = nullptr;
    for (int i = 0; i < EV_COUNT; i++) e->ev[i] = nullptr;
}

int alga_engine_create(int hip_device, alga_engine **out) {
    if (!out) return ALGA_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int ndev = 0;
    hipError_t err = hipGetDeviceCount(&ndev);
    if (err != hipSuccess || ndev <= 0) return ALGA_ERR_NO_DEVICE;
    if (hip_device < 0 || hip_device >= ndev) return ALGA_ERR_INVALID_ARGUMENT;
    DeviceGuard guard;
    if (hipSetDevice(hip_device) != hipSuccess) return ALGA_ERR_NO_DEVICE;
    alga_engine *e = new (std::nothrow) alga_engine();
    if (!e) return ALGA_ERR_OUT_OF_MEMORY;
    e->device = hip_device;
    memset(&e->stats, 0, sizeof(e->stats));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, hip_device) == hipSuccess) {
        snprintf(e->dev_name, sizeof(e->dev_name), "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
        if (prop.multiProcessorCount > 0) e->n_cu = prop.multiProcessorCount;
    }
    int rc = ALGA_OK;
    if (hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking) != hipSuccess) { e->own_stream = nullptr; rc = ALGA_ERR_HIP; }
    if (rc == ALGA_OK && hipStreamCreateWithFlags(&e->side_stream, hipStreamNonBlocking) != hipSuccess) { e->side_stream = nullptr; rc = ALGA_ERR_HIP; }
    if (rc == ALGA_OK && hipEventCreateWithFlags(&e->ev_side, hipEventDisableTiming) != hipSuccess) { e->ev_side = nullptr; rc = ALGA_ERR_HIP; }
    for (int i = 0; i < EV_COUNT && rc == ALGA_OK; i++)
        if (hipEventCreate(&e->ev[i]) != hipSuccess) { e->ev[i] = nullptr; rc = ALGA_ERR_HIP; }
    if (rc == ALGA_OK && hipHostMalloc((void **) &e->h_counters, (CNT_TOTAL + 2 + alga_engine::H_EXTRA) * sizeof(unsigned long long)) != hipSuccess) { e->h_counters = nullptr; rc = ALGA_ERR_OUT_OF_MEMORY; }
    if (rc == ALGA_OK && hipHostGetDevicePointer((void **) &e->h_counters_dev, e->h_counters, 0) != hipSuccess) rc = ALGA_ERR_HIP;
    if (rc != ALGA_OK) { engine_free_handles(e); delete e; return rc; }     // nothing the failed attempt created is left behind
    *out = e;
    return ALGA_OK;
}

void alga_engine_destroy(alga_engine *e) {
    if (!e) return;
    DeviceGuard guard;
    (void) hipSetDevice(e->device);
    if (e->own_stream) (void) hipStreamSynchronize(e->own_stream);
    if (e->side_stream) (void) hipStreamSynchronize(e->side_stream);
    for (DevBuf *b : e->owned) alga_release(*b);           // everything alga_ensure ever allocated
    alga_release(e->up_raw);
    for (DevBuf *b : {&e->in_bytes[0], &e->in_bytes[1], &e->in_nl[0], &e->in_nl[1], &e->in_tiles, &e->in_tile_off}) alga_release(*b);
    for (DevBuf *b : {&e->sp_rowptr, &e->sp_sorted, &e->sp_list, &e->sp_cnt, &e->sp_orow, &e->sp_out, &e->sp_in}) alga_release(*b);
    alga_staging_release(e);
    for (void *&p : e->gfa_pin) { if (p) (void) hipHostFree(p); p = nullptr; }
    for (auto &kv : e->host_lists) free(kv.first);         // host edge lists the caller never gave back (alga_free_edges after this is an error: alga_amd.h)
    e->host_lists.clear();
    engine_free_handles(e);
    delete e;
}

const char *alga_last_error(const alga_engine *e) { return e ? e->err.c_str() : "no engine"; }

int alga_engine_device_name(const alga_engine *e, char *buf, size_t buflen) {
    if (!e || !buf || buflen == 0) return ALGA_ERR_INVALID_ARGUMENT;
    snprintf(buf, buflen, "%s", e->dev_name);
    return ALGA_OK;
}

int alga_engine_set_option(alga_engine *e, const char *name, int64_t value) {
    if (!e || !name) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!strcmp(name, "probe")) {
        if (value < ALGA_PROBE_AUTO || value > ALGA_PROBE_CLUSTER) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option probe: 0 auto, 1 table, 2 cluster");
        e->opt_probe = (int) value;
    } else if (!strcmp(name, "cluster_bucket_bias")) {
        if (value < -8 || value > 8) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option cluster_bucket_bias: -8 .. 8");
        e->opt_cluster_bucket_bias = (int) value;
    } else if (!strcmp(name, "cluster_pairs")) {
        e->opt_cluster_pairs = value != 0;
    } else if (!strcmp(name, "pile")) {
        e->opt_pile = (value == 2 || value == 3) ? (int) value : (value != 0);       // (2, 3, tests only: no sample -- the pile kernels take every build they can, however many buckets are irregular; 3: in the mixed form)
    } else if (!strcmp(name, "pile_runs")) {
        e->opt_pile_runs = value != 0;
    } else if (!strcmp(name, "pile_runs_list")) {
        e->opt_pile_runs_list = value != 0;
    } else if (!strcmp(name, "pile_dir")) {
        if (value < 0 || value > 2) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option pile_dir: 0 directory records, 1 k_pile_build from the keys, 2 ... and no directory for a pure pile build");
        e->opt_pile_dir = (int) value;
    } else if (!strcmp(name, "pile_deg_fold")) {
        e->opt_pile_deg_fold = value != 0;
    } else if (!strcmp(name, "emit_fused")) {
        e->opt_emit_fused = value != 0;
    } else if (!strcmp(name, "pile_probe_lean")) {
        e->opt_pile_probe_lean = value != 0;
    } else if (!strcmp(name, "pile_probe_tail")) {
        e->opt_pile_probe_tail = value != 0;
    } else if (!strcmp(name, "pile_runs_ahead")) {
        e->opt_pile_runs_ahead = value != 0;
    } else if (!strcmp(name, "pile_stream_by_id")) {
        e->opt_pile_stream_by_id = value != 0;
    } else if (!strcmp(name, "pile_check")) {
        e->opt_pile_check = value != 0;
    } else if (!strcmp(name, "pile_skip_gather")) {
        e->opt_pile_skip_gather = value != 0;
    } else if (!strcmp(name, "cluster_order")) {
        e->opt_cluster_order = value != 0;
    } else if (!strcmp(name, "local_big_max")) {
        e->big_limit = value < 0 ? -1 : (int) std::min<int64_t>(value, 1 << 20);
    } else if (!strcmp(name, "shard_bucket_max")) {
        e->opt_shard_dmax = (int) std::max<int64_t>(1, std::min<int64_t>(value, 4096));
    } else if (!strcmp(name, "rsort_variant")) {
        // tuning only, and PROCESS-WIDE (not per engine): the tile shape of radix_sort.hip's (u32, u32) sort for every engine of this process
        if (value < 0 || value > 1) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option rsort_variant: 0 tiles of 8192 pairs, 1 tiles of 16384 pairs");
        rsort_set_variant((int) value);
    } else if (!strcmp(name, "stream_slots")) {
        e->opt_stream_slots = value >= 4 ? 4 : 2;
    } else if (!strcmp(name, "pile_range")) {
        e->opt_pile_range = value != 0;
    } else if (!strcmp(name, "pkb_legacy")) {
        e->opt_pkb_legacy = (int) value;
    } else if (!strcmp(name, "own_sort")) {
        e->opt_own_sort = value != 0;
    } else if (!strcmp(name, "test_presort_oom")) {
        e->opt_test_presort_oom = value != 0;              // tests only: the supplement's look-ahead buffers answer out of memory; the rounds must go on serially
    } else if (!strcmp(name, "test_pile_oom")) {
        e->opt_test_pile_oom = value != 0;                 // tests only: the pile path's allocation answers out of memory; the build must continue on the pairwise kernels
    } else if (!strcmp(name, "test_unsorted_index")) {
        e->opt_test_unsorted_index = value != 0;           // tests only: the clustered index is built over UNSORTED keys; the build must fail, not fault
    } else if (!strcmp(name, "gfa_chunk_mb")) {
        if (value < 1 || value > 4096) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option gfa_chunk_mb: 1 .. 4096");
        e->opt_gfa_chunk_mb = (int) value;
    } else if (!strcmp(name, "mst_mid_nodes")) {
        if (value < 8 || value > (1 << 20)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option mst_mid_nodes: 8 .. 2^20");
        e->opt_mst_mid_nodes = (int) value;
    } else if (!strcmp(name, "consensus_max_blocks")) {
        if (value < 0 || value > (1 << 20)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option consensus_max_blocks: 0 .. 2^20");
        e->opt_consensus_max_blocks = (int) value;
    } else if (!strcmp(name, "unitig_ruling")) {
        if (value < -1 || value > 1) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option unitig_ruling: -1, 0 or 1");
        e->opt_unitig_ruling = (int) value;
    } else if (!strcmp(name, "correct_slice_keys")) {
        if (value < 1 || value > (1ll << 31)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option correct_slice_keys: 1 .. 2^31");
        e->opt_correct_slice_keys = value;
    } else if (!strcmp(name, "correct_dir_bits")) {
        if (value < 0 || value > 28) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option correct_dir_bits: 0 (auto) or 1 .. 28");
        e->opt_correct_dir_bits = (int) value;
    } else if (!strcmp(name, "place_dir_bits")) {
        if (value < 0 || value > 26) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option place_dir_bits: 0 (auto) or 1 .. 26");
        e->opt_place_dir_bits = (int) value;
    } else if (!strcmp(name, "ipolish_max_blocks")) {
        if (value < 1 || value > 8192) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option ipolish_max_blocks: 1 .. 8192");
        e->opt_ipolish_max_blocks = (int) value;
    } else if (!strcmp(name, "merge_max_blocks")) {
        if (value < 1 || value > 8192) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option merge_max_blocks: 1 .. 8192");
        e->opt_merge_max_blocks = (int) value;
    } else if (!strcmp(name, "contain_max_blocks")) {
        if (value < 1 || value > 8192) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option contain_max_blocks: 1 .. 8192");
        e->opt_contain_max_blocks = (int) value;
    } else if (!strcmp(name, "stitch_max_blocks")) {
        if (value < 1 || value > 8192) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option stitch_max_blocks: 1 .. 8192");
        e->opt_stitch_max_blocks = (int) value;
    } else if (!strcmp(name, "grow_max_blocks")) {
        if (value < 1 || value > 8192) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option grow_max_blocks: 1 .. 8192");
        e->opt_grow_max_blocks = (int) value;
    } else if (!strcmp(name, "scaffold_max_blocks")) {
        if (value < 1 || value > 8192) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option scaffold_max_blocks: 1 .. 8192");
        e->opt_scaffold_max_blocks = (int) value;
    } else if (!strcmp(name, "sam_max_blocks")) {
        if (value < 0 || value > 16384) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "option sam_max_blocks: 0 (the launches' own caps) or 1 .. 16384");
        e->opt_sam_max_blocks = (int) value;
    } else if (!strcmp(name, "auto_reduction_per_target")) {
        e->opt_force_per_target = value != 0;
    } else return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "unknown option");
    return ALGA_OK;
}

int alga_engine_reserve(alga_engine *e, int32_t n_nodes, int32_t max_len, int32_t min_overlap, uint64_t n_edges_hint) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (n_nodes < 0 || max_len < 1 || min_overlap < 1) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "alga_engine_reserve: n_nodes >= 0, max_len >= 1, min_overlap >= 1");
    DeviceGuard guard;
    HIP_TRY(e, hipSetDevice(e->device));
    int rc;
    const uint64_t n = (uint64_t) n_nodes;
    const uint64_t E = n_edges_hint ? n_edges_hint : n + n / 16 + 4096;
    if ((rc = alga_ensure(e, e->counters, (CNT_TOTAL + 2) * sizeof(unsigned long long)))) return rc;
    // what prepare() would derive for this shape: the same sizing functions as the build itself
    Prepared pp;
    pp.nd.n = n_nodes; pp.max_len = max_len; pp.live = n;
    pp.cfg.Lmin = min_overlap; pp.cfg.Lcap = std::min(max_len, 500) + 1; pp.cfg.rsoemo = min_overlap; pp.cfg.soes = 3;
    int eq = 0;
    const bool local = max_len <= 500 && max_len - min_overlap <= LOCAL_MAX_SPAN;
    const bool clustered = local && e->opt_probe != ALGA_PROBE_TABLE &&
                           cluster_plan(pp.cfg, max_len, n, e->opt_cluster_bucket_bias, &pp.cluster, &eq);
    if (clustered) {
        pp.cluster_eq = eq;
        if ((rc = cluster_alloc(e, pp))) return rc;
        if (max_len - min_overlap <= 63 && eq <= 4) {
            if ((rc = alga_ensure(e, e->cl_defer, (size_t) (n + 64) * sizeof(int32_t)))) return rc;
            if ((rc = alga_ensure(e, e->loc_second, (size_t) (e->opt_stream_slots >= 4 ? LOCAL_SLOTS_MAX - 1 : 1) * (n + 1) * sizeof(unsigned long long)))) return rc;
        }
        // the pile path, should the reads turn out to have one length and no masks (what reserve assumes: it is told one length)
        if (e->opt_pile != 0 && e->opt_cluster_pairs != 0 && e->opt_cluster_order != 0 && max_len - min_overlap <= 63 && pile_plan(pp.cfg, pp.cluster, eq, max_len, false)) {
            if ((rc = pile_alloc(e, n, pp.cluster.n_buckets, e->own_stream))) return rc;
        }
    } else {
        const uint32_t nb = seed_buckets_for(n, e->seed_fill_x10);
        if ((rc = alga_ensure(e, e->table, (size_t) nb * SEED_BUCKET * sizeof(unsigned long long)))) return rc;
        const uint32_t fb = seed_filter_bits_for(n);
        if (fb && (rc = alga_ensure(e, e->filter, fb / 8))) return rc;
    }
    if (local) {
        const uint64_t slack = std::max(probe_record_slack(e->n_cu, n, true), clustered ? cluster_record_slack(e->n_cu, n) : 0);
        const uint64_t cap = std::max<uint64_t>(e->rec_cap_hint_local, 2 * n + 4096) + slack;
        if ((rc = alga_ensure(e, e->outdeg, (size_t) (n + 1) * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->loc_first, (size_t) (n + 1) * sizeof(unsigned long long)))) return rc;
        if ((rc = alga_ensure(e, e->loc_big_list, (1u << 20) * sizeof(int32_t)))) return rc;
        if ((rc = alga_ensure(e, e->rec_dst, cap * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->rec_val, cap * sizeof(unsigned long long)))) return rc;
        if ((rc = alga_ensure(e, e->scan_scratch, scan_scratch_bytes(n)))) return rc;
        if ((rc = alga_ensure(e, e->out_rowptr, (size_t) (n + 1) * sizeof(uint32_t)))) return rc;
        if ((rc = alga_ensure(e, e->out_cnt, (size_t) (n + 1) * sizeof(uint32_t)))) return rc;
    }
    if ((rc = alga_ensure(e, e->edges, (size_t) (E + 1) * sizeof(alga_edge_dev)))) return rc;
    // The other cost of a process's first build is not memory: the HIP runtime loads a kernel's code object when the kernel is first
    // launched (~20 ms for the kernels of one build, measured: a fresh engine's first build 58 ms against 37 ms for the second fresh
    // engine of the same process).  A miniature build of the same SHAPE -- 4096 random reads of max_len nucleotides, so the very
    // template instantiations the real build will use -- pays that here, ahead of time.
    if (!e->warmed && n_nodes > 0) {
        const int W = blocks_of(max_len), stride = hbm_row_stride(W), wn = 4096;
        std::vector<uint32_t> rows((size_t) wn * stride, 0u);
        std::vector<int32_t> lens((size_t) wn, max_len);
        uint64_t x = 0x9E3779B97F4A7C15ull;
        for (int i = 0; i < wn; i++)
            for (int k = 0; k < W; k++) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                uint32_t w = (uint32_t) (x >> 16);
                const int used = 2 * max_len - 32 * k;                           // bits of this block that belong to the read (tail bits stay zero)
                if (used < 32) w &= used <= 0 ? 0u : ((1u << used) - 1u);
                rows[(size_t) i * stride + k] = w;
            }
        void *d_rows = nullptr, *d_len = nullptr;
        if (hipMalloc(&d_rows, rows.size() * 4) == hipSuccess && hipMalloc(&d_len, lens.size() * 4) == hipSuccess &&
            hipMemcpy(d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d_len, lens.data(), lens.size() * 4, hipMemcpyHostToDevice) == hipSuccess) {
            alga_nodes nd{(const uint32_t *) d_rows, stride, (const int32_t *) d_len, wn, nullptr, nullptr};
            alga_prefsuf_params wp;
            alga_prefsuf_default_params(&wp);
            wp.min_overlap = min_overlap; wp.rsoe_min_overlap = std::min(max_len, min_overlap + (max_len - min_overlap) / 2);
            const alga_edge *d = nullptr;
            uint64_t m = 0;
            const int wrc = alga_prefsuf_build_device(e, &nd, &wp, nullptr, &d, &m);   // its result is of no interest; a failure is not one of reserve
            (void) wrc;
            e->err.clear();
            e->warmed = true;
        }
        if (d_rows) (void) hipFree(d_rows);
        if (d_len) (void) hipFree(d_len);
        (void) hipGetLastError();
        alga_forget_node_set(e);
        memset(&e->stats, 0, sizeof(e->stats));
    }
    return ALGA_OK;
}

void alga_prefsuf_default_params(alga_prefsuf_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->min_overlap = 0;          /* caller must set: src/main.cpp:100-110 derives it from the read length */
    p->rsoe_min_overlap = 0;
    p->soes = 3;                 /* include/GraphCreators/GraphCreatorPrefSuf.h:62 */
    p->max_len_cap = 500;        /* src/GraphCreators/GraphCreatorPrefSuf.cpp:92 */
    p->collect_stats = 0;
}

int alga_prefsuf_build_device(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, void *hip_stream,
                              const alga_edge **d_edges, uint64_t *n_edges) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!d_edges || !n_edges) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *d_edges = nullptr; *n_edges = 0;
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    memset(&e->stats, 0, sizeof(e->stats));
    Prepared pp;
    int rc = prepare(e, nodes, p, s, pp);
    if (rc) return rc;
    e->stats.nodes_live = pp.live;
    uint64_t n_rec = 0, E = 0;
    bool done = false;
    if (pp.reduction == ALGA_REDUCTION_SOURCE_SIDE || (pp.reduction == ALGA_REDUCTION_AUTO && pp.local_ok)) {
        rc = build_local(e, pp, 0, nodes->n, s, &E);
        if (rc == ALGA_OK) done = true;
        else if (rc != ALGA_ERR_UNSUPPORTED || pp.reduction == ALGA_REDUCTION_SOURCE_SIDE) return rc;
        else { e->err.clear(); memset(&e->stats, 0, sizeof(e->stats)); e->stats.nodes_live = pp.live; }    // AUTO: capacity case, per-target pipeline
    }
    if (!done) {
        if ((rc = discover_impl(e, pp, 0, nodes->n, s, &n_rec))) return rc;
        if ((rc = reduce_impl(e, pp, (const uint32_t *) e->rec_dst.p, (const unsigned long long *) e->rec_val.p, n_rec, e->stats.records,
                              0, nodes->n, s, &E))) return rc;
        e->stats.reduction_used = ALGA_REDUCTION_PER_TARGET;
    }
    e->stats.ms_seed = ev_ms(e, EV_START, EV_SEED);
    e->stats.ms_probe = ev_ms(e, EV_SEED, EV_PROBE);
    e->stats.ms_probe_pairs = e->pairs_timed ? ev_ms(e, EV_SEED, EV_PAIRS) : 0.0;
    store_phase_stats(e);
    e->stats.ms_group = ev_ms(e, EV_PROBE, EV_GROUP);
    e->stats.ms_reduce = ev_ms(e, EV_GROUP, EV_REDUCE);
    e->stats.ms_emit = ev_ms(e, EV_REDUCE, EV_EMIT);
    e->stats.ms_total = ev_ms(e, EV_START, EV_EMIT);
    *d_edges = (const alga_edge *) e->edges.p;
    *n_edges = E;
    return ALGA_OK;
}

// Host node set -> the engine's own upload buffers, in the engine's row layout (hbm_row_stride: 16-byte aligned rows that never
// straddle a 64-byte line take the wide-load kernels); *dev describes the resident copy (masks included when given).
// mode 0: all of it.  The N-GPU host entry point (engine_multi.hip) cuts it in two so that the rows cross PCIe ONCE per node, not once per GPU:
// mode 1 -- checks, lengths, and the rows [row_begin, row_end) of the caller's row array alone, into the raw buffer at their own place (room for
// raw_rows_cap rows: the other ranks' slices arrive there by all-gather; *d_raw = the buffer); mode 2 -- what follows once the raw buffer is
// complete: twin expansion / re-stride into the engine's layout, the masks.
static int upload_nodes_impl(alga_engine *e, const alga_nodes *nodes, alga_nodes *dev, bool twin_rows, int mode = 0, uint64_t row_begin = 0, uint64_t row_end = 0,
                             uint64_t raw_rows_cap = 0, uint32_t **d_raw = nullptr);

int alga_upload_nodes(alga_engine *e, const alga_nodes *nodes, alga_nodes *dev) { return upload_nodes_impl(e, nodes, dev, false); }
int alga_upload_twin_nodes(alga_engine *e, const alga_nodes *nodes, alga_nodes *dev) { return upload_nodes_impl(e, nodes, dev, true); }
int alga_upload_nodes_phase(alga_engine *e, const alga_nodes *nodes, bool twin_rows, int mode, uint64_t row_begin, uint64_t row_end, uint64_t raw_rows_cap, alga_nodes *dev,
                            uint32_t **d_raw) { return upload_nodes_impl(e, nodes, dev, twin_rows, mode, row_begin, row_end, raw_rows_cap, d_raw); }

// twin_rows: nodes->words holds the rows of the ODD nodes only (row k = node 2k + 1); len / masks have all n entries
static int upload_nodes_impl(alga_engine *e, const alga_nodes *nodes, alga_nodes *dev, bool twin_rows, int mode, uint64_t row_begin, uint64_t row_end, uint64_t raw_rows_cap,
                             uint32_t **d_raw) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!nodes || !dev) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes / output must not be NULL");
    if (nodes->n < 0 || (nodes->n > 0 && (!nodes->words || !nodes->len || nodes->stride_words <= 0)))
        return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad node set");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = e->own_stream;
    int rc;
    const size_t n = (size_t) nodes->n;
    // ONE parallel pass over the lengths (0.36 GB at 90 M nodes: a single core needs 30 ms for it, eight need four): the longest read -- the
    // caller's rows must hold the caller's reads, the upload below changes the stride -- and, for twin rows, that node 2k is removed (0) or
    // as long as node 2k + 1, from which it is rebuilt.  For large node sets it runs BESIDE the upload of the rows (which does not depend on
    // it; a node set it refuses has then travelled for nothing).
    const double t_check0 = now_ms_host();
    int32_t max_len = 0;
    if (twin_rows && (n & 1)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "twin_rows: the node count must be even");
    const char *check_msg = nullptr;                       // (written by the checking thread, read after its join)
    double check_ms = 0.0;
    auto check = [&]() {
        const int T = n >= (1u << 22) ? 8 : 1;
        int32_t part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        char bad[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        auto job = [&](int t) {
            int32_t m = 0; char b = 0;
            size_t i0 = n * (size_t) t / T, i1 = n * (size_t) (t + 1) / T;
            i0 &= ~(size_t) 1; if (t + 1 < T) i1 &= ~(size_t) 1;              // whole pairs
            if (twin_rows) { for (size_t i = i0; i + 1 < i1 + 1 && i + 1 < n; i += 2) { const int32_t a = nodes->len[i], c = nodes->len[i + 1]; m = std::max(m, std::max(a, c)); b |= (a != 0 && a != c); } }
            else for (size_t i = i0; i < i1; i++) m = std::max(m, nodes->len[i]);
            part[t] = m; bad[t] = b;
        };
        std::vector<std::thread> th;
        try { for (int t = 1; t < T; t++) th.emplace_back(job, t); } catch (...) { }
        job(0);
        for (size_t t = th.size() + 1; t < (size_t) T; t++) job((int) t);       // (threads that could not be started: their share here)
        for (std::thread &x : th) x.join();
        bool any_bad = false;
        int32_t mx = 0;
        for (int t = 0; t < T; t++) { mx = std::max(mx, part[t]); any_bad = any_bad || bad[t]; }
        max_len = mx;
        if ((int64_t) blocks_of(mx) > (int64_t) nodes->stride_words) check_msg = "stride_words is smaller than the longest read needs";
        else if (any_bad) check_msg = "twin_rows: node 2k is neither removed nor as long as node 2k + 1";
        check_ms = now_ms_host() - t_check0;
    };
    struct Joiner { std::thread t; ~Joiner() { if (t.joinable()) t.join(); } } chk;
    bool async_check = n >= (1u << 22) && mode != 2;
    if (mode == 2) async_check = false;
    if (async_check) { try { chk.t = std::thread(check); } catch (...) { async_check = false; } }
    if (!async_check && mode != 2) { check(); if (check_msg) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, check_msg); }
    const double t_up0 = now_ms_host();
    // the lengths cross PCIe as narrow as they are: a byte per node where no read is longer than 255 nt (every short-read set: 0.09 GB instead
    // of 0.36 GB at 90 M nodes), two up to 65 535; narrowed by the staging threads on their way into the pinned buffers, widened on the device
    auto upload_len = [&]() -> int {
        int r;
        const int len_bytes = max_len <= 255 ? 1 : (max_len <= 65535 ? 2 : 4);
        if (len_bytes == 4 || n < (1u << 20)) return alga_staged_h2d(e, e->up_len.p, nodes->len, n * sizeof(int32_t));
        if ((r = alga_ensure(e, e->up_len_narrow, n * (size_t) len_bytes + 16))) return r;
        const int32_t *src = nodes->len;
        const AlgaStageFill fill = [src, len_bytes](void *dst, size_t off, size_t bytes) {
            if (len_bytes == 1) { uint8_t *d = (uint8_t *) dst; const int32_t *p = src + off; for (size_t i = 0; i < bytes; i++) d[i] = (uint8_t) p[i]; }
            else { uint16_t *d = (uint16_t *) dst; const int32_t *p = src + off / 2; for (size_t i = 0; i < bytes / 2; i++) d[i] = (uint16_t) p[i]; }
        };
        if ((r = alga_staged_h2d_fill(e, e->up_len_narrow.p, n * (size_t) len_bytes, fill))) return r;
        launch_widen_len(e->up_len_narrow.p, len_bytes, (int32_t *) e->up_len.p, (uint64_t) n, s);
        return alga_check_launch(e, "k_widen_len");
    };
    // what the rows' upload waits for: the check (when it runs beside it) -- before anything reads max_len
    auto join_check = [&]() -> int {
        if (chk.t.joinable()) chk.t.join();
        return check_msg ? alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, check_msg) : ALGA_OK;
    };
    // Rows travel at the caller's stride through pinned staging buffers (staging.hip) and are re-strided on the DEVICE.
    const int stride_up = alga::hbm_row_stride(nodes->stride_words);
    const size_t wbytes = n * (size_t) stride_up * sizeof(uint32_t);
    const size_t raw_bytes = (twin_rows ? n / 2 : n) * (size_t) nodes->stride_words * sizeof(uint32_t);
    if (mode != 2) alga_forget_node_set(e);
    if ((rc = alga_ensure(e, e->up_words, wbytes))) return rc;
    if ((rc = alga_ensure(e, e->up_len, n * sizeof(int32_t)))) return rc;
    alga_nodes dn = *nodes;
    const size_t rows_total = twin_rows ? n / 2 : n, row_bytes = (size_t) nodes->stride_words * sizeof(uint32_t);
    const bool via_raw = twin_rows || stride_up != nodes->stride_words || mode != 0;
    if (n && mode != 2) {
        HIP_TRY(e, hipStreamSynchronize(s));                       // nothing of an earlier call still reads the upload buffers
        if (via_raw) {
            if ((rc = alga_ensure(e, e->up_raw, std::max(raw_bytes, (size_t) raw_rows_cap * row_bytes) + 64))) return rc;
            const size_t r0 = mode == 1 ? (size_t) std::min<uint64_t>(row_begin, rows_total) : 0, r1 = mode == 1 ? (size_t) std::min<uint64_t>(row_end, rows_total) : rows_total;
            if (r1 > r0 && (rc = alga_staged_h2d(e, (char *) e->up_raw.p + r0 * row_bytes, (const char *) nodes->words + r0 * row_bytes, (r1 - r0) * row_bytes))) return rc;
        } else if ((rc = alga_staged_h2d(e, e->up_words.p, nodes->words, raw_bytes))) return rc;
        if ((rc = join_check())) return rc;
        if ((rc = upload_len())) return rc;                         // (the twin expansion reads the lengths)
        HIP_TRY(e, hipStreamSynchronize(s));
    }
    if (d_raw) *d_raw = (uint32_t *) e->up_raw.p;
    if (mode == 1) { e->stats_host[0] = check_ms; e->stats_host[1] = now_ms_host() - t_up0; return ALGA_OK; }
    if (n && via_raw) {
        if (twin_rows) {
            launch_expand_twins((const uint32_t *) e->up_raw.p, nodes->stride_words, (const int32_t *) e->up_len.p, (uint32_t *) e->up_words.p, stride_up, (uint64_t) (n / 2), s);
            if ((rc = alga_check_launch(e, "k_expand_twins"))) return rc;
        } else {
            launch_restride((const uint32_t *) e->up_raw.p, nodes->stride_words, (uint32_t *) e->up_words.p, stride_up, (uint64_t) n, s);
            if ((rc = alga_check_launch(e, "k_restride"))) return rc;
        }
        HIP_TRY(e, hipStreamSynchronize(s));
    }
    if ((rc = join_check())) return rc;
    e->stats_host[0] = check_ms;
    dn.stride_words = stride_up;
    dn.words = (const uint32_t *) e->up_words.p;
    dn.len = (const int32_t *) e->up_len.p;
    if (nodes->align_from) {
        if ((rc = alga_ensure(e, e->up_from, n))) return rc;
        if (n && (rc = alga_staged_h2d(e, e->up_from.p, nodes->align_from, n))) return rc;
        dn.align_from = (const uint8_t *) e->up_from.p;
    }
    if (nodes->align_to) {
        if ((rc = alga_ensure(e, e->up_to, n))) return rc;
        if (n && (rc = alga_staged_h2d(e, e->up_to.p, nodes->align_to, n))) return rc;
        dn.align_to = (const uint8_t *) e->up_to.p;
    }
    *dev = dn;
    e->stats_host[1] = (mode == 2 ? e->stats_host[1] : 0.0) + now_ms_host() - t_up0;
    return ALGA_OK;
}

int alga_download_edges(alga_engine *e, const alga_edge *d_edges, uint64_t n_edges, alga_edge **edges) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!edges || (n_edges && !d_edges)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "pointers must not be NULL");
    *edges = nullptr;
    HIP_TRY(e, hipSetDevice(e->device));
    alga_edge *h = (alga_edge *) alga_host_list_take(e, (size_t) (n_edges ? n_edges : 1) * sizeof(alga_edge));
    if (!h) return alga_fail(e, ALGA_ERR_OUT_OF_MEMORY, "host edge buffer");
    int rc;
    if (n_edges && (rc = alga_staged_d2h(e, h, d_edges, (size_t) n_edges * sizeof(alga_edge)))) { alga_host_list_give(e, h); return rc; }
    *edges = h;
    return ALGA_OK;
}

int alga_prefsuf_build_host(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, alga_edge **edges, uint64_t *n_edges) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!edges || !n_edges) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *edges = nullptr; *n_edges = 0;
    if (!nodes || !p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes/params must not be NULL");
    alga_nodes dn;
    int rc = upload_nodes_impl(e, nodes, &dn, p->twin_rows != 0);
    if (rc) return rc;
    const alga_edge *d_edges = nullptr;
    uint64_t E = 0;
    const double t0 = now_ms_host();
    if ((rc = alga_prefsuf_build_device(e, &dn, p, (void *) e->own_stream, &d_edges, &E))) return rc;
    const double t1 = now_ms_host();
    if ((rc = alga_download_edges(e, d_edges, E, edges))) return rc;
    *n_edges = E;
    e->stats.host_ms_check = e->stats_host[0]; e->stats.host_ms_upload = e->stats_host[1]; e->stats.host_ms_build = t1 - t0; e->stats.host_ms_download = now_ms_host() - t1;
    return ALGA_OK;
}

// An edge list on the device (grouped by src: a build's result, or the supplement's) -> host, in COMPACT form: a byte per node (out-degree), per
// edge its neighbour (4 bytes) and its offset (1 byte), lists in node order -- 5.1 bytes per edge on the way down instead of 12 (0.56 GB instead
// of 1.1 GB at the north-star size: the host entry point is PCIe-bound).  ALGA_ERR_UNSUPPORTED where a degree or an offset does not fit a byte.
int alga_download_edges_compact(alga_engine *e, int32_t n_nodes, const alga_edge *d_edges, uint64_t E, alga_compact_edges *out) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output must not be NULL");
    memset(out, 0, sizeof(*out));
    if (n_nodes < 0 || (E && !d_edges)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad edge list");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = e->own_stream;
    int rc;
    const size_t n = (size_t) n_nodes;
    if ((rc = alga_ensure(e, e->counters, (CNT_TOTAL + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->cp_deg, n + 16))) return rc;
    if ((rc = alga_ensure(e, e->cp_dst, (size_t) (E + 4) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->cp_off, (size_t) E + 16))) return rc;
    unsigned long long *bad = (unsigned long long *) e->counters.p + CNT_TOTAL + 1;
    HIP_TRY(e, hipMemsetAsync(bad, 0, sizeof(unsigned long long), s));
    launch_compact_edges((const alga_edge_dev *) d_edges, n_nodes, E, (uint8_t *) e->cp_deg.p, (uint32_t *) e->cp_dst.p, (uint8_t *) e->cp_off.p, bad, s);
    if ((rc = alga_check_launch(e, "k_compact_edges"))) return rc;
    HIP_TRY(e, hipMemcpyAsync(&e->h_counters[CNT_TOTAL + 1], bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (e->h_counters[CNT_TOTAL + 1] != 0) return alga_fail(e, ALGA_ERR_UNSUPPORTED, "compact edges: an out-degree or an offset does not fit a byte; take the edge triples");
    // one host block: [dst: 4 E][off: E][deg: n], each part 64-byte aligned
    const size_t o_off = (((size_t) E * 4) + 63) & ~(size_t) 63, o_deg = (o_off + (size_t) E + 63) & ~(size_t) 63, total = o_deg + n + 64;
    char *h = (char *) alga_host_list_take(e, total);
    if (!h) return alga_fail(e, ALGA_ERR_OUT_OF_MEMORY, "host edge buffer");
    if ((E && ((rc = alga_staged_d2h(e, h, e->cp_dst.p, (size_t) E * 4)) || (rc = alga_staged_d2h(e, h + o_off, e->cp_off.p, (size_t) E)))) ||
        (n && (rc = alga_staged_d2h(e, h + o_deg, e->cp_deg.p, n)))) { alga_host_list_give(e, h); return rc; }
    out->n_nodes = n_nodes; out->n_edges = E;
    out->dst = (const uint32_t *) h; out->offset = (const uint8_t *) (h + o_off); out->degree = (const uint8_t *) (h + o_deg);
    return ALGA_OK;
}

// The build of alga_prefsuf_build_host with the graph handed back in that form.
int alga_prefsuf_build_host_compact(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, alga_compact_edges *out) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output must not be NULL");
    memset(out, 0, sizeof(*out));
    if (!nodes || !p) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "nodes/params must not be NULL");
    alga_nodes dn;
    int rc = upload_nodes_impl(e, nodes, &dn, p->twin_rows != 0);
    if (rc) return rc;
    const alga_edge *d_edges = nullptr;
    uint64_t E = 0;
    const double t0 = now_ms_host();
    if ((rc = alga_prefsuf_build_device(e, &dn, p, (void *) e->own_stream, &d_edges, &E))) return rc;
    const double t1 = now_ms_host();
    if ((rc = alga_download_edges_compact(e, nodes->n, d_edges, E, out))) return rc;
    e->stats.host_ms_check = e->stats_host[0]; e->stats.host_ms_upload = e->stats_host[1]; e->stats.host_ms_build = t1 - t0; e->stats.host_ms_download = now_ms_host() - t1;
    return ALGA_OK;
}

void alga_free_compact_edges(alga_engine *e, alga_compact_edges *c) {
    if (!c) return;
    alga_host_list_give(e, const_cast<uint32_t *>(c->dst));
    memset(c, 0, sizeof(*c));
}

// Host memory the DMA engines read and write directly (pinned): node arrays allocated here go up without the copy through the engine's staging
// buffers, and nothing else about them differs from malloc'ed memory.  (Allocation itself is slow -- the pages are mapped and locked: seconds
// per ten GB -- an assembler asks once, while it still parses.)
void *alga_host_alloc(alga_engine *e, size_t bytes) {
    if (!e) return nullptr;
    e->err.clear();
    DeviceGuard guard;
    if (hipSetDevice(e->device) != hipSuccess) return nullptr;
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16) != hipSuccess) { (void) hipGetLastError(); alga_fail(e, ALGA_ERR_OUT_OF_MEMORY, "alga_host_alloc"); return nullptr; }
    return p;
}
void alga_host_free(alga_engine *e, void *p) {
    (void) e;
    if (p) (void) hipHostFree(p);
}

void alga_free_edges(alga_engine *e, alga_edge *edges) { alga_host_list_give(e, edges); }

int alga_copy_to_host(alga_engine *e, void *dst, const void *d_src, size_t bytes) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (bytes == 0) return ALGA_OK;
    if (!dst || !d_src) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "pointers must not be NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return ALGA_OK;
}

int alga_device_alloc(alga_engine *e, size_t bytes, void **d_out) {
    if (!e || !d_out) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    *d_out = nullptr;
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipMalloc(d_out, bytes ? bytes : 16));
    return ALGA_OK;
}

void alga_device_free(alga_engine *e, void *d_ptr) {
    if (!e || !d_ptr) return;
    (void) hipSetDevice(e->device);
    (void) hipFree(d_ptr);
}

int alga_copy_to_device(alga_engine *e, void *d_dst, const void *src, size_t bytes) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (bytes == 0) return ALGA_OK;
    if (!d_dst || !src) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "pointers must not be NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return ALGA_OK;
}

int alga_prefsuf_last_stats(const alga_engine *e, alga_prefsuf_stats *out) {
    if (!e || !out) return ALGA_ERR_INVALID_ARGUMENT;
    *out = e->stats;
    return ALGA_OK;
}

int alga_prefsuf_discover_device(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, int32_t src_begin, int32_t src_end,
                                 void *hip_stream, const uint32_t **d_dst, const uint64_t **d_val, uint64_t *n_records) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!d_dst || !d_val || !n_records) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    memset(&e->stats, 0, sizeof(e->stats));
    Prepared pp;
    int rc = prepare(e, nodes, p, s, pp);
    if (rc) return rc;
    if (src_begin < 0 || src_end > nodes->n || src_begin > src_end) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad source range");
    e->stats.nodes_live = pp.live;
    uint64_t n_rec = 0;
    if ((rc = discover_impl(e, pp, src_begin, src_end, s, &n_rec))) return rc;
    e->stats.ms_seed = ev_ms(e, EV_START, EV_SEED);
    e->stats.ms_probe = ev_ms(e, EV_SEED, EV_PROBE);
    e->stats.ms_total = ev_ms(e, EV_START, EV_PROBE);
    *d_dst = (const uint32_t *) e->rec_dst.p; *d_val = (const uint64_t *) e->rec_val.p;
    *n_records = n_rec;
    return ALGA_OK;
}

int alga_prefsuf_build_range_device(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, int32_t src_begin, int32_t src_end,
                                    void *hip_stream, const alga_edge **d_edges, uint64_t *n_edges) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!d_edges || !n_edges) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *d_edges = nullptr; *n_edges = 0;
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    memset(&e->stats, 0, sizeof(e->stats));
    Prepared pp;
    int rc = prepare(e, nodes, p, s, pp);
    if (rc) return rc;
    if (src_begin < 0 || src_end > nodes->n || src_begin > src_end) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad source range");
    if (pp.reduction == ALGA_REDUCTION_PER_TARGET) return alga_fail(e, ALGA_ERR_UNSUPPORTED, "per-target reduction requested: use discover + exchange + reduce");
    e->stats.nodes_live = pp.live;
    uint64_t E = 0;
    if ((rc = build_local(e, pp, src_begin, src_end, s, &E))) return rc;
    e->stats.ms_seed = ev_ms(e, EV_START, EV_SEED);
    e->stats.ms_probe = ev_ms(e, EV_SEED, EV_PROBE);
    e->stats.ms_probe_pairs = e->pairs_timed ? ev_ms(e, EV_SEED, EV_PAIRS) : 0.0;
    store_phase_stats(e);
    e->stats.ms_emit = ev_ms(e, EV_REDUCE, EV_EMIT);
    e->stats.ms_total = ev_ms(e, EV_START, EV_EMIT);
    *d_edges = (const alga_edge *) e->edges.p;
    *n_edges = E;
    return ALGA_OK;
}

int alga_prefsuf_keys_device(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, int32_t node_begin, int32_t node_end,
                             void *hip_stream, alga_node_keys *out) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!out) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointer must not be NULL");
    memset(out, 0, sizeof(*out));
    e->keyed_n = -1;
    e->store_n = -1;                                       // the key pass rewrites runs and keys
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    Prepared pp;
    int rc = prepare(e, nodes, p, s, pp);
    if (rc) return rc;
    if (node_begin < 0 || node_end > nodes->n || node_begin > node_end) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad node range");
    out->n = nodes->n;
    if (pp.cluster_eq == 0 || pp.reduction == ALGA_REDUCTION_PER_TARGET || nodes->n == 0) return ALGA_OK;      // eligible = 0: nothing to share
    if ((rc = cluster_alloc(e, pp))) return rc;
    launch_cluster_keys(pp.nd, pp.cfg, pp.cluster, node_begin, node_end, (uint32_t *) e->cl_keys[0].p, (uint32_t *) e->cl_vals[0].p, (uint32_t *) e->cl_meta.p,
                        e->cl_runs.p, (uint8_t *) e->cl_nruns.p, s);
    if ((rc = alga_check_launch(e, "k_node_runs"))) return rc;
    e->keyed_n = nodes->n; e->keyed_begin = node_begin; e->keyed_end = node_end; e->keyed_words = (const void *) nodes->words;
    out->eligible = 1;
    out->meta_needed = pp.uniform_len > 0 ? 0 : 1;
    out->d_keys = (uint32_t *) e->cl_keys[0].p;
    out->d_meta = (uint32_t *) e->cl_meta.p;
    return ALGA_OK;
}

int alga_prefsuf_reduce_device(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, const uint32_t *d_dst,
                               const uint64_t *d_val, uint64_t n_records, int32_t dst_begin, int32_t dst_end,
                               void *hip_stream, const alga_edge **d_edges, uint64_t *n_edges) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!d_edges || !n_edges) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *d_edges = nullptr; *n_edges = 0;
    if (n_records && (!d_dst || !d_val)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "record arrays must not be NULL");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    Prepared pp;
    int rc = prepare(e, nodes, p, s, pp);
    if (rc) return rc;
    if (dst_begin < 0 || dst_end > nodes->n || dst_begin > dst_end) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bad target range");
    HIP_TRY(e, hipEventRecord(e->ev[EV_PROBE], s));
    uint64_t E = 0;
    if ((rc = reduce_impl(e, pp, d_dst, (const unsigned long long *) d_val, n_records, n_records, dst_begin, dst_end, s, &E))) return rc;
    e->stats.ms_group = ev_ms(e, EV_PROBE, EV_GROUP);
    e->stats.ms_reduce = ev_ms(e, EV_GROUP, EV_REDUCE);
    e->stats.ms_emit = ev_ms(e, EV_REDUCE, EV_EMIT);
    *d_edges = (const alga_edge *) e->edges.p;
    *n_edges = E;
    return ALGA_OK;
}

int alga_sort_records_device(alga_engine *e, const uint32_t *d_dst, const uint64_t *d_val, uint64_t n_records, int32_t n_nodes,
                             void *hip_stream, const uint32_t **d_dst_sorted, const uint64_t **d_val_sorted, uint64_t *n_valid) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!d_dst_sorted || !d_val_sorted || !n_valid) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *d_dst_sorted = nullptr; *d_val_sorted = nullptr; *n_valid = 0;
    if (n_records && (!d_dst || !d_val)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "record arrays must not be NULL");
    if (n_nodes < 0) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "negative node count");
    if (n_records >= (1ull << 32) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 overlap records; shard the input");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    int rc;
    const int bits = key_bits_for(n_nodes);
    const size_t temp_bytes = sort_records_temp_bytes(n_records, bits);
    if ((rc = alga_ensure(e, e->counters, (CNT_TOTAL + 2) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->keys, (size_t) (n_records + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->xs_dst, (size_t) (n_records + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->xs_val, (size_t) (n_records + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->sort_temp, temp_bytes))) return rc;
    unsigned long long *cnt = (unsigned long long *) e->counters.p;
    HIP_TRY(e, hipMemsetAsync(cnt + CNT_SORT_VALID, 0, sizeof(unsigned long long), s));
    launch_make_keys(d_dst, n_records, 0, n_nodes, (uint32_t *) e->keys.p, cnt + CNT_SORT_VALID, s);
    if ((rc = alga_check_launch(e, "k_make_keys"))) return rc;
    HIP_TRY(e, sort_records(e->sort_temp.p, temp_bytes, (const uint32_t *) e->keys.p, (uint32_t *) e->xs_dst.p, (const unsigned long long *) d_val,
                            (unsigned long long *) e->xs_val.p, n_records, bits, s));
    HIP_TRY(e, hipMemcpyAsync(&e->h_counters[CNT_SORT_VALID], cnt + CNT_SORT_VALID, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    *d_dst_sorted = (const uint32_t *) e->xs_dst.p; *d_val_sorted = (const uint64_t *) e->xs_val.p;
    *n_valid = e->h_counters[CNT_SORT_VALID];
    return ALGA_OK;
}

int alga_sort_edges_device(alga_engine *e, const alga_edge *d_edges, uint64_t n_edges, int32_t n_nodes, void *hip_stream,
                           const alga_edge **d_sorted) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!d_sorted) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointer must not be NULL");
    *d_sorted = nullptr;
    if (n_edges && !d_edges) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "edge array must not be NULL");
    if (n_edges >= (1ull << 32) - 16) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 edges");
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    int rc;
    const size_t temp_bytes = sort_edges_temp_bytes(n_edges);
    if ((rc = alga_ensure(e, e->edge_keys, (size_t) (n_edges + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->edge_keys2, (size_t) (n_edges + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->edge_vals, (size_t) (n_edges + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->edge_vals2, (size_t) (n_edges + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->edges_sorted, (size_t) (n_edges + 1) * sizeof(alga_edge_dev)))) return rc;
    if ((rc = alga_ensure(e, e->sort_temp, temp_bytes))) return rc;
    launch_edges_to_keys((const alga_edge_dev *) d_edges, n_edges, (unsigned long long *) e->edge_keys.p, (uint32_t *) e->edge_vals.p, s);
    if ((rc = alga_check_launch(e, "k_edges_to_keys"))) return rc;
    int src_bits = 1;
    while (src_bits < 31 && (1ll << src_bits) < (long long) n_nodes) src_bits++;
    HIP_TRY(e, sort_edges(e->sort_temp.p, temp_bytes, (const unsigned long long *) e->edge_keys.p, (unsigned long long *) e->edge_keys2.p,
                          (const uint32_t *) e->edge_vals.p, (uint32_t *) e->edge_vals2.p, n_edges, src_bits, s));
    launch_keys_to_edges((const unsigned long long *) e->edge_keys2.p, (const uint32_t *) e->edge_vals2.p, n_edges, (alga_edge_dev *) e->edges_sorted.p, s);
    if ((rc = alga_check_launch(e, "k_keys_to_edges"))) return rc;
    HIP_TRY(e, hipStreamSynchronize(s));
    *d_sorted = (const alga_edge *) e->edges_sorted.p;
    return ALGA_OK;
}

// the (u32 key, u32 value) sort of the index build on its own (tests / tools): stable on the key bits [begin_bit, 32).  d_vals == NULL with own != 0:
// the values are 0, 1, 2, ... (the index build's, the final-contig filter's and the supplement's form of the call)
int alga_sort_u32_pairs_device(alga_engine *e, const uint32_t *d_keys, const uint32_t *d_vals, uint64_t n, int32_t begin_bit, int32_t own, int32_t repeat,
                               void *hip_stream, const uint32_t **d_keys_sorted, const uint32_t **d_vals_sorted, double *ms_best) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!d_keys_sorted || !d_vals_sorted) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *d_keys_sorted = nullptr; *d_vals_sorted = nullptr;
    if (n && !d_keys) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "key / value arrays must not be NULL");
    if (n && !d_vals && !own) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "value array must not be NULL for the library's sort (own = 0)");
    if (begin_bit < 0 || begin_bit > 31) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "begin_bit must be in [0, 31]");
    if (n >= (1ull << 32) - (1u << 16)) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 pairs");
    DeviceGuard guard;
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    int rc;
    const size_t temp_bytes = sort_u32_pairs_temp_bytes(n);
    if ((rc = alga_ensure(e, e->cl_keys[1], (size_t) (n + ALGA_KEY_ARRAY_SLACK + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->cl_vals[1], (size_t) (n + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = alga_ensure(e, e->sort_temp, temp_bytes))) return rc;
    e->store_n = -1; e->keyed_n = -1; e->pile_n = -1;      // (the sort buffers of a clustered build are rewritten)
    double best = 0.0;
    for (int it = 0; it < std::max(1, repeat); it++) {
        HIP_TRY(e, hipEventRecord(e->ev[EV_START], s));
        HIP_TRY(e, sort_u32_pairs(e->sort_temp.p, temp_bytes, d_keys, (uint32_t *) e->cl_keys[1].p, d_vals, (uint32_t *) e->cl_vals[1].p, n, begin_bit, s, own != 0));
        HIP_TRY(e, hipEventRecord(e->ev[EV_SORT], s));
        HIP_TRY(e, hipStreamSynchronize(s));
        const double ms = ev_ms(e, EV_START, EV_SORT);
        best = it == 0 ? ms : std::min(best, ms);
    }
    if (ms_best) *ms_best = best;
    *d_keys_sorted = (const uint32_t *) e->cl_keys[1].p; *d_vals_sorted = (const uint32_t *) e->cl_vals[1].p;
    return ALGA_OK;
}

// the (u64 key, u64 value) sort of the supplement's k-mer entries on its own (tests / tools): stable on the key bits [0, bits)
int alga_sort_u64_pairs_device(alga_engine *e, const uint64_t *d_keys, const uint64_t *d_vals, uint64_t n, int32_t bits, int32_t own, int32_t repeat,
                               void *hip_stream, const uint64_t **d_keys_sorted, const uint64_t **d_vals_sorted, double *ms_best) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!d_keys_sorted || !d_vals_sorted) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *d_keys_sorted = nullptr; *d_vals_sorted = nullptr;
    if (n && (!d_keys || !d_vals)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "key / value arrays must not be NULL");
    if (bits < 1 || bits > (own ? 50 : 64)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "bits must be in [1, 50] (the library's sort: [1, 64])");
    if (n >= (1ull << 32) - (1u << 16)) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 pairs");
    DeviceGuard guard;
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    int rc;
    const size_t temp_bytes = std::max(rsort_u64_pairs_temp_bytes(n), sort_u64_pairs_temp_bytes(n, bits));
    if ((rc = alga_ensure(e, e->pk_keys2, (size_t) (n + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->pk_vals2, (size_t) (n + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->sort_temp, temp_bytes))) return rc;
    double best = 0.0;
    for (int it = 0; it < std::max(1, repeat); it++) {
        HIP_TRY(e, hipEventRecord(e->ev[EV_START], s));
        if (own) HIP_TRY(e, rsort_u64_pairs(e->sort_temp.p, temp_bytes, (const unsigned long long *) d_keys, (unsigned long long *) e->pk_keys2.p,
                                            (const unsigned long long *) d_vals, (unsigned long long *) e->pk_vals2.p, n, bits, s));
        else HIP_TRY(e, sort_u64_pairs(e->sort_temp.p, temp_bytes, (const unsigned long long *) d_keys, (unsigned long long *) e->pk_keys2.p,
                                       (const unsigned long long *) d_vals, (unsigned long long *) e->pk_vals2.p, n, bits, s));
        HIP_TRY(e, hipEventRecord(e->ev[EV_SORT], s));
        HIP_TRY(e, hipStreamSynchronize(s));
        const double ms = ev_ms(e, EV_START, EV_SORT);
        best = it == 0 ? ms : std::min(best, ms);
    }
    if (ms_best) *ms_best = best;
    *d_keys_sorted = (const uint64_t *) e->pk_keys2.p; *d_vals_sorted = (const uint64_t *) e->pk_vals2.p;
    return ALGA_OK;
}

// the (u32 key, u64 value) sort of the sharded build's run descriptors on its own (tests / tools): stable on the key bits [begin_bit, end_bit);
// a window that is not one is [0, 32) (sort_desc)
int alga_sort_desc_device(alga_engine *e, const uint32_t *d_keys, const uint64_t *d_vals, uint64_t n, int32_t begin_bit, int32_t end_bit, int32_t own, int32_t repeat,
                          void *hip_stream, const uint32_t **d_keys_sorted, const uint64_t **d_vals_sorted, double *ms_best) {
    if (!e) return ALGA_ERR_INVALID_ARGUMENT;
    e->err.clear();
    if (!d_keys_sorted || !d_vals_sorted) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "output pointers must not be NULL");
    *d_keys_sorted = nullptr; *d_vals_sorted = nullptr;
    if (n && (!d_keys || !d_vals)) return alga_fail(e, ALGA_ERR_INVALID_ARGUMENT, "key / value arrays must not be NULL");
    if (n >= (1ull << 32) - (1u << 16)) return alga_fail(e, ALGA_ERR_CAPACITY, "more than 2^32 records");
    DeviceGuard guard;
    HIP_TRY(e, hipSetDevice(e->device));
    hipStream_t s = hip_stream ? (hipStream_t) hip_stream : e->own_stream;
    int rc;
    const size_t temp_bytes = sort_desc_temp_bytes(n);
    if ((rc = alga_ensure(e, e->pk_keys2, (size_t) (n + 1) * sizeof(unsigned long long)))) return rc;      // (the buffers of alga_sort_u64_pairs_device)
    if ((rc = alga_ensure(e, e->pk_vals2, (size_t) (n + 1) * sizeof(unsigned long long)))) return rc;
    if ((rc = alga_ensure(e, e->sort_temp, temp_bytes))) return rc;
    double best = 0.0;
    for (int it = 0; it < std::max(1, repeat); it++) {
        HIP_TRY(e, hipEventRecord(e->ev[EV_START], s));
        HIP_TRY(e, sort_desc(e->sort_temp.p, temp_bytes, d_keys, (uint32_t *) e->pk_keys2.p, (const unsigned long long *) d_vals, (unsigned long long *) e->pk_vals2.p, n,
                             begin_bit, end_bit, s, own != 0));
        HIP_TRY(e, hipEventRecord(e->ev[EV_SORT], s));
        HIP_TRY(e, hipStreamSynchronize(s));
        const double ms = ev_ms(e, EV_START, EV_SORT);
        best = it == 0 ? ms : std::min(best, ms);
    }
    if (ms_best) *ms_best = best;
    *d_keys_sorted = (const uint32_t *) e->pk_keys2.p; *d_vals_sorted = (const uint64_t *) e->pk_vals2.p;
    return ALGA_OK;
}

int alga_write_graph(const char *path, int32_t n_nodes, const alga_edge *edges, uint64_t n_edges) {
    if (!path || n_nodes < 0 || (n_edges && !edges)) return ALGA_ERR_INVALID_ARGUMENT;
    FILE *f = fopen(path, "wb");
    if (!f) return ALGA_ERR_IO;
    std::string buf;
    buf.reserve(1 << 20);
    auto put = [&](int32_t v) { buf.append((const char *) &v, 4); };
    uint32_t s = (uint32_t) n_nodes;
    buf.append((const char *) &s, 4);
    uint64_t k = 0;
    bool ok = true;
    for (int32_t i = 0; i < n_nodes && ok; i++) {
        uint64_t end = k;
        while (end < n_edges && edges[end].src == i) end++;
        put(i); put((int32_t) (end - k));
        for (; k < end; k++) { put(edges[k].dst); put(edges[k].offset); }
        if (buf.size() >= (1 << 20)) { ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size(); buf.clear(); }
    }
    if (ok && !buf.empty()) ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (fclose(f) != 0) ok = false;
    if (!ok || k != n_edges) return ALGA_ERR_IO; /* k != n_edges: edges were not sorted by src / out of range */
    return ALGA_OK;
}

} // extern "C"
