// alga_amd/csrc/engine_internal.h -- engine state and small helpers shared by engine.hip and engine_pkb.hip
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <algorithm>
#include <string>
#include <vector>
#include <unordered_map>

#include "../../include/alga_amd.h"
#include "prefsuf_common.h"
#include "prefsuf_kernels.h"
#include "pkb_kernels.h"

struct DevBuf {
    void  *p = nullptr;
    size_t cap = 0;
};

enum { EV_START = 0, EV_SEED, EV_PROBE, EV_GROUP, EV_REDUCE, EV_EMIT, EV_PAIRS, EV_KEYS, EV_SORT, EV_GATHER, EV_DIR, EV_SAMPLE, EV_COUNT };
constexpr int ALGA_STAGE_THREADS = 8;      // worker threads (pinned buffer pairs, streams) of the staged host <-> HBM copies

struct alga_engine {
    std::vector<DevBuf *> owned;              // the members below that hold an allocation (alga_ensure)
    int         device = -1;
    hipStream_t own_stream = nullptr;
    hipStream_t side_stream = nullptr;         // supplement: the next round's sort beside this round's groups (pkb_presort)
    hipEvent_t  ev_side = nullptr;             // ... its end
    std::string err;
    char        dev_name[256] = {0};
    int         n_cu = 256;
    int         seed_fill_x10 = 20;           // average seed-table bucket fill x10
    // alga_engine_set_option (include/alga_amd.h): every switch that changes how (never what) the engine computes
    int         opt_probe = 0;                // ALGA_PROBE_AUTO / _TABLE / _CLUSTER
    int         opt_cluster_bucket_bias = 0;  // log2 factor on the bucket count of the clustered probe's index
    int         opt_force_per_target = 0;     // AUTO reduction resolves to PER_TARGET
    int         opt_shard_dmax = 4096;        // bucket-sharded join: descriptors of one bucket it takes (option "shard_bucket_max"; tests lower it to see the decline)
    int         opt_test_unsorted_index = 0;  // tests only: skip the sort of the clustered index (the directory pass must flag it, the build must fail)
    hipEvent_t  ev[EV_COUNT] = {};
    // device buffers, grown on demand and kept between calls
    DevBuf table, filter, counters, rowptr, rec_dst, rec_val, keys, seg_key, seg_val, heads, sort_temp, out_cnt, outdeg, out_rowptr, edges, scan_scratch;
    DevBuf cl_defer;                                        // sources the pair kernel hands to the general kernel
    uint32_t h_first_hkey = 255;                            // supplement: sort key of the longest group of a round (255 - min(D, 255))
    // alga_prefsuf_keys_device: the node range whose keys / runs this engine computed last (n < 0: none), consumed by a build with
    // params.keys_shared
    int32_t keyed_n = -1, keyed_begin = 0, keyed_end = 0;
    bool defer_list_valid = false;     // the last discover ran k_probe_stream first: cl_defer / counters[CNT_DEFERRED] list every source whose row came from records
    const void *keyed_words = nullptr;
    // the entry array / index / directory / runs left by the last clustered build (n < 0: none): reusable with params.keys_shared = 2
    int32_t store_n = -1, store_run_begin = 0, store_run_end = 0, store_eq = 0;
    uint32_t store_buckets = 0;
    const void *store_words = nullptr;
    // node statistics of the last prepare() (k_node_stats): reused by the further pieces of a build (params.keys_shared = 2)
    int stat_max_len = 0, stat_min_len = 0; uint64_t stat_live = 0; unsigned long long stat_mask_asym = 0;
    const void *stat_len = nullptr, *stat_from = nullptr, *stat_to = nullptr;
    bool   warmed = false;                                  // alga_engine_reserve has run its miniature build (kernel code objects loaded)
    bool   pairs_timed = false;                             // EV_PAIRS was recorded in the last discovery
    bool   store_timed = false;                             // EV_KEYS / EV_SORT / EV_GATHER were recorded in the last discovery
    bool   pile_keys_only = false, pile_kept_pure = false;  // of the build that made the piles at hand: its key pass made no run lists / it kept the build in the pure pile form (no entry array)
    int    opt_pile_range = 1;                              // option "pile_range": the pile path also for a source id range (a rank's share of the N-GPU build); 0: all sources only, as until round 5
    int    opt_pile_skip_gather = 1;                        // option "pile_skip_gather": no entry array for a build the pile path keeps
    int    opt_pile = 1;                                    // option "pile": the probe through piles (prefsuf_pile.hip) where the input allows it
    int    opt_pile_runs = 1;                               // option "pile_runs": 1 = a pile's run list from its consensus (k_pile_runs_consensus; the key pass of a kept build makes target keys only), 0 = from its outer members' own lists (round 4)
    int    opt_pile_runs_list = 1;                          // option "pile_runs_list": 1 = k_pile_build lists its piles and k_pile_runs_consensus_list works through the lists (four waves per SIMD), 0 = k_pile_runs_consensus sweeps the side records for them (round 5)
    DevBuf cl_pile_list;                                    // the piles of every k_pile_build workgroup and their counts (pile_list_bytes)
    int    opt_pile_deg_fold = 1;                           // option "pile_deg_fold": 1 = the first pass of the out-degree scan moves the out-degrees k_pile_probe left in the slots (no k_pile_deg), 0 = k_pile_deg behind the probe
    int    opt_emit_fused = 1;                              // option "emit_fused": 1 = finalize_local sums the out-degrees per tile and one pass writes row pointers and slot edges (k_emit_tile_sums, k_emit_scan_tiles: nothing moved to deg[], no row pointer read back), 0 = scan of deg[] first, k_local_emit_first behind it (until round 8)
    int    opt_pile_dir = 2;                                // option "pile_dir": 0 = k_pile_build reads the bucket directory (until round 7), 1 = it takes bucket starts, counts and class offsets from the sorted keys and never reads cl_dir, 2 = ... and a build of the pure pile form has no directory at all
    bool   dir_late = false;                                // the last index build ran the pile path's sample in front of the directory pass (EV_SAMPLE was recorded)
    bool   pile_tab_index = false;                          // the last index build made the directory only for a build the pile path did not keep pure: the pairwise kernels of a pure build read the piles' table (bucket_record)
    int    opt_pile_stream_by_id = 0;                       // option "pile_stream_by_id": 1 = a build kept in the pure pile form sends what k_pile_probe hands on through k_probe_stream (list mode, entries by id) before the general kernel, 0 = to the general kernel at once (the default until the pass is measured)
    int    opt_pile_probe_lean = 1;                         // option "pile_probe_lean": 1 = k_pile_probe<true> (the source's row taken in slot 0 only, no last-mismatch search past position 63), 0 = k_pile_probe<false> (round 5)
    int    opt_pile_probe_tail = 1;                         // option "pile_probe_tail" (with pile_probe_lean): 1 = k_pile_probe<true, true> (the look-ups of a tile's one or two targets batched, the further groups' bucket words read an iteration ahead), 0 = the serial tail
    int    opt_pile_runs_ahead = 0;                         // option "pile_runs_ahead": 1 = k_pile_runs_consensus_list reads its piles' records a round ahead of the work on them, 0 = round by round (the default: the look-ahead measured no gain)
    bool   pile_deg_pending = false;                       // the last discovery left that move to finalize_local's scan
    int    opt_pile_check = 0;                              // option "pile_check" (tests): every node gets its own run list and every first-group member's is compared with its pile's clipped list (stats.pile_list_*)
    bool   expect_pairwise = false;                         // the pile path declined the build before this one: the next key pass makes every run list up front
    DevBuf cl_pile_side_r, cl_pile_cursor;                  // the side records of a source id range (k_pile_side_range), its block cursor
    DevBuf cl_pile_own;                                     // bit j: entry j of the key order reads a run list of its own
    int    opt_pkb_legacy = 0;                              // option "pkb_legacy" (A/B and tests): bit 0 groups of 8 .. 16 k-mers a wave each, bit 1 the library's k-mer sort, bit 2 head list in three kernels, bit 3 groups of 8 .. 16 replayed inside the pair kernel, bit 4 the library's unique + a row-pointer pass after the merge, bit 5 the k-mer walk on a 128-bit value, bit 6 every tip record's snapshot half rewritten every round, bit 7 a k-mer walk per round
    int    opt_own_sort = 1;                                // option "own_sort": the (key, id) sort of the index build is the engine's own radix sort (radix_sort.hip); 0: rocPRIM's
    int    opt_test_presort_oom = 0;                        // tests only: the allocation of the supplement's look-ahead buffers reports out of memory (the rounds must go on one after the other)
    int    opt_test_pile_oom = 0;                           // tests only: the pile path's allocation reports out of memory (the build must continue on the pairwise kernels)
    bool   pile_timed = false;                              // EV_DIR was recorded in the last discovery (k_pile_build ran behind it)
    DevBuf cl_pile_succ;                                    // per entry (16 B): its id, the member of its own pile that starts next to its right, its place in the pile (k_pile_probe reads this, not the entry)
    DevBuf cl_pile_rec2;                                    // run lists of the further k-mer groups of a bucket (64 B at the group's slot, laid out like the second half of a bucket's line)
    DevBuf cl_pile_rec, cl_pile_cnt, cl_pile_tab;   // records of further k-mer groups (64 B per entry slot), group of every entry, {buckets, irregular buckets} of the sample, bucket records (128 B per bucket)
    uint32_t pile_epoch = 0;                                // of the last k_pile_build: what makes a record of cl_pile_tab valid (the table is cleared when it is allocated, and when this wraps)
    int32_t pile_n = -1; const void *pile_words = nullptr;  // the node set the pile records describe (n < 0: none)
    int    opt_cluster_order = 1;                           // option "cluster_order": k_probe_stream walks all sources in entry-array (key) order (0: id order)
    int    opt_cluster_pairs = 1;                           // option "cluster_pairs": 0 = general kernel only, 1 = k_probe_stream first
    DevBuf cl_keys[2], cl_vals[2], cl_meta, cl_runs, cl_nruns, cl_store, cl_dir;   // clustered minimizer join: sort buffers, per-node minimizer runs, entry array, bucket directory
    DevBuf loc_second;                                      // ... the other edge of a two-edge source the pair kernel finished (clustered probe)
    bool   loc_second_used = false;                         // the last discovery wrote loc_second
    uint32_t loc_slot_stride = 0;                           // ... with three slots per source, this many entries apart (0: one slot)
    int    opt_stream_slots = 4;                            // option "stream_slots": standing items of a source k_probe_stream writes to slots itself (4; 2: round 4's form)
    DevBuf loc_first, loc_big_list, loc_big_items;          // source-side form: one-edge slots; second pass over repeat-rich sources
    int    big_limit = -1;                                  // largest per-wave item slice of that pass; -1 = built-in (option "local_big_max": tests)
    DevBuf edge_keys, edge_keys2, edge_vals, edge_vals2, edges_sorted, xs_dst, xs_val;
    DevBuf up_words, up_len, up_from, up_to;   // uploads of the host-buffer entry points
    DevBuf up_len_narrow;                      // ... the lengths as they cross PCIe (one or two bytes per node), widened on the device
    DevBuf cp_deg, cp_dst, cp_off;             // compact edge list (alga_prefsuf_build_host_compact): degree bytes, neighbours, offset bytes
    // approximate supplement (engine_pkb.hip)
    DevBuf cl_defer2;                           // mixed form of a pile-path build: the sources k_probe_stream (list mode) hands on
    DevBuf pk_keys, pk_keys2, pk_vals, pk_vals2, pk_marks, pk_big, pk_add, pk_ekeys, pk_ekeys2, pk_flag, pk_pos, pk_edges[2], pk_rowptr, pk_deg,
           pk_mask, pk_cnt, pk_io, pk_io2, pk_tips, pk_heads, pk_g[2], pk_addk, pk_addk2, pk_merged, pk_hsz, pk_hsz2, pk_heads2, pk_nadd, pk_koff,
           pk_gsz, pk_fixlist, pk_bounds, pk_tiprec, pk_tipidx, pk_keys_all, pk_vals_all;
    // the supplement's look-ahead (engine_pkb.hip: pkb_presort): the NEXT round's sorted entries and group heads, made on side_stream while this round's groups and merge run
    DevBuf pk_keys2b, pk_vals2b, pk_headsb, pk_hszb, sort_temp2, pk_fixlist2, pk_cnt2;
    // duplicate / prefix-read removal (engine_ingest.hip)
    DevBuf pp_rows, pp_len, pp_perm[2], pp_keys[2], pp_mark, pp_keep, pp_pos, pp_out_rows, pp_out_len, pp_out_pair, pp_tally;
    // staged host <-> HBM copies (staging.hip)
    bool        stage_ready = false;
    void       *stage_pin[ALGA_STAGE_THREADS][2] = {};
    hipEvent_t  stage_ev[ALGA_STAGE_THREADS][2] = {};
    hipStream_t stage_stream[ALGA_STAGE_THREADS] = {};
    DevBuf      up_raw;                        // the caller's rows at the caller's stride, before the device re-stride
    // host edge lists handed out by the *_host entry points: capacity of every live one; one released list is kept for the
    // next call (its pages are already mapped: a fresh 1 GB malloc costs more in page faults than the copy into it)
    std::unordered_map<void *, size_t> host_lists;
    void       *host_spare = nullptr;
    size_t      host_spare_cap = 0;
    DevBuf      in_bytes[2], in_nl[2], in_tiles, in_tile_off;   // device ingest: file bytes, line ends, newline counts per tile
    DevBuf      sp_rowptr, sp_sorted, sp_list, sp_cnt, sp_orow, sp_out, sp_in;   // first simplifier step (engine_simplify.hip)
    // dangling-branch removal (engine_simplify.hip, tip_kernels.hip): counters, sort buffers, the unique sorted edges and their reverse, row pointers,
    // alive / kill bytes, node records of both directions, branching and overflow lists, the overflow route's workspaces, the result
    DevBuf      tp_cnt, tp_keys[2], tp_vals[2], tp_flag, tp_pos, tp_best, tp_est, tp_rev, tp_rfid, tp_rowptr[2], tp_alive, tp_kill, tp_rec[2], tp_branch,
                tp_overflow, tp_ws, tp_out;
    // removal of short parallel paths (engine_simplify.hip, mst_kernels.hip): counters, the mutable rows (row pointers, entries, lengths), owner[],
    // the two pending lists, winners, the overflow list, the overflow route's workspaces, the output row pointers, the result
    DevBuf      mp_cnt, mp_rowptr, mp_rows, mp_len, mp_owner, mp_pend[2], mp_win, mp_overflow, mp_overflow2, mp_ws, mp_ws_big, mp_orow, mp_out;
    // the overflow states whose maps are known to be empty (mst_clear leaves them so): buffer, size and geometry of the last 0xFF fill of each tier;
    // p == nullptr: fill before use (never filled, reallocated, another geometry, or a call that did not reach its end)
    struct MstFilled { const void *p = nullptr; size_t bytes = 0; uint32_t hbits = 0, cap_nodes = 0, cap_edges = 0; int32_t n_ws = 0; } mp_filled[2];
    int         opt_mst_mid_nodes = 4096;          // option "mst_mid_nodes": nodes a state of the first overflow tier holds (and twice as many edges); tests lower it to reach the second tier
    // GFA export (engine_gfa.hip): line sizes, their 64-bit byte offsets, per-source row pointers, scan tile sums, chunk bounds, the device chunk
    DevBuf      gfa_sizes, gfa_off, gfa_rowptr, gfa_tiles, gfa_bounds, gfa_buf;
    void       *gfa_pin[2] = {nullptr, nullptr};   // pinned host chunks (hipHostMalloc), gfa_pin_cap bytes each
    size_t      gfa_pin_cap = 0;
    int         opt_gfa_chunk_mb = 256;            // option "gfa_chunk_mb": size of a formatted chunk of the GFA text
    // unitig graph (engine_unitig.hip): sort buffers of the 2 m twin records / the unitig edges, group flags and their scan, E*, its row pointers,
    // next / offset / prev per node, the two rank and min arrays, tails, winners, pair numbers, per-pair sizes, the result arrays
    DevBuf      ut_cnt, ut_keys[2], ut_vals[2], ut_flag, ut_pos, ut_best, ut_estar, ut_rowptr, ut_nxt, ut_noff, ut_prv, ut_rank[2], ut_min[2], ut_tail,
                ut_win, ut_pair, ut_pcnt, ut_ulen, ut_ulen2, ut_uwords, ut_path_off, ut_word_off, ut_tiles, ut_path_node, ut_path_pos, ut_uid, ut_words,
                ut_edges, ut_link, ut_rnode, ut_rrec[2];      // (ruling set: next / offset pairs, the rulers, their records)
    int         opt_unitig_ruling = -1;            // option "unitig_ruling": the list ranking ranks a ruling set first (1), never (0), from 2^16 nodes on (-1)
    uint64_t    ut_n_pairs = 0, ut_n_edges = 0;    // the result at hand (ut_valid: the buffers hold one)
    bool        ut_valid = false;
    int32_t     ut_n_nodes = 0;                    // ... the n of the node set it was made from, the sum of its lengths
    uint64_t    ut_total_bases = 0;
    bool        ut_is_contig = false;              // the result at hand came from alga_contigs_device (the FASTA names its records contig_id=<j>)
    // extension of contigs by paired connections (engine_extend.hip): counters, the contig graph's row pointers, per oriented contig its weight,
    // entries, direct link, links of L*, the only one, head / bases / links before it on its path, new oriented id; the seam list; and the new
    // result, built beside the one it is read from and swapped in at the end
    DevBuf      ex_cnt, ex_rowptr, ex_w, ex_kcnt, ex_dlink, ex_outcnt, ex_sole, ex_xhead, ex_xbase, ex_xrank, ex_uid, ex_scnt, ex_seam_off,
                ex_seam_entry, ex_pcnt, ex_uwords, ex_ulen, ex_ulen2, ex_path_off, ex_word_off, ex_path_node, ex_path_pos, ex_words, ex_edges;
    bool        ut_is_extended = false;            // the result at hand came from alga_extend_contigs_device: ex_seam_off / ex_seam_entry describe it
    // contigs (engine_contig.hip): counters, the base graph B of a round (two buffers in turn) and its row pointers, P flags, per-run smallest read
    // index, the chain records and the chain that enters every run, drop marks, flags and their scan, the group sort, the per-group best
    // (weight, key), H with the triangle cut's workspaces, and for the contig graph: winners, pair numbers, oriented ids, their chains, degrees,
    // the edge sort
    DevBuf      ct_cnt, ct_B[2], ct_rowptr, ct_pflag, ct_runkey, ct_chain, ct_headchain, ct_drop, ct_flag, ct_pos, ct_keys[2], ct_vals[2], ct_hw, ct_hk, ct_H,
                ct_hrow, ct_hsorted, ct_hlist, ct_hcnt, ct_win, ct_pair, ct_oid, ct_cid, ct_deg, ct_epos, ct_ekeys[2], ct_evals[2], ct_names;
    // consensus of the unitigs (engine_consensus.hip): counters, the sequences, the per-word column masks, the vote bytes, per-pair window / changed
    DevBuf      cs_cnt, cs_words, cs_mask, cs_votes, cs_trim, cs_len, cs_changed;
    bool        cs_valid = false;                  // the buffers hold the consensus of the unitig result at hand
    bool        cs_has_votes = false;
    // the final contig set (engine_final.hip): counters, the rank sort, the marks of the end reads, the two lists of undecided pairs, the accepted
    // flags and their scan, the result arrays, the windows of the accepted pairs, and for the trim: the capped rows, their lengths, trim by id
    DevBuf      fc_cnt, fc_keys[2], fc_vals, fc_first, fc_min, fc_list[2], fc_flag, fc_ids, fc_verdict, fc_rank, fc_id, fc_new, fc_trim, fc_begin, fc_len,
                fc_order, fc_wbegin, fc_wlen, fc_rows, fc_rlen, fc_tid;
    bool        fc_valid = false;                  // the buffers hold the final set of the unitig result and consensus at hand
    uint64_t    fc_n_accepted = 0;
    int         opt_consensus_max_blocks = 0;      // option "consensus_max_blocks": cap on the grids of the consensus kernels (0: their own); tests lower it to make small inputs stride
    // read error correction (engine_correct.hip): counters, the per-block tables of the histogram / run-head / fix kernels, the column sums, a slice's
    // keys before and after the sort, its solid flags and their scan, the solid keys of all slices, their directory
    DevBuf      cr_cnt, cr_table, cr_hist, cr_keys[2], cr_flag, cr_pos, cr_solid, cr_dir;
    int64_t     opt_correct_slice_keys = 1ll << 28;   // option "correct_slice_keys": occurrences a slice of the k-mer count holds (a single bin above it is a slice of its own)
    int         opt_correct_dir_bits = 0;             // option "correct_dir_bits": bits of the solid keys' directory, 0 = about two keys per bucket (tests force long and empty buckets)
    // the seed index of the call at hand (seed_index.hip; the placement, the grow and the merge build theirs here, and none reads an earlier
    // call's): the (k-mer, column) pairs before and after the sort, the directory, the per-wave usable-seed masks of the kernel that seeds from it
    DevBuf      seed_keys[2], seed_vals[2], seed_dir, seed_ub;
    // reads placed on sequences (engine_place.hip).  Workspaces: counters, the targets of a final result, the lengths' scan, the column array, the
    // difference array.  The result: per read target / pos / mm / hits / state, col_off, the scan of the differences (the cover is its entries
    // from 1 on), the per-target sums, the histogram
    DevBuf      pl_cnt, pl_fbegin, pl_flen, pl_scan, pl_cols, pl_diff;
    DevBuf      pl_target, pl_pos, pl_mm, pl_hits, pl_state, pl_coloff, pl_cover, pl_tstat, pl_hist;
    bool        pl_valid = false;                  // the result buffers hold a placement
    uint64_t    pl_targets = 0, pl_reads = 0;      // ... of this many reads on this many targets
    uint64_t    pl_ncolumns = 0, pl_nhist = 0;      // ... its col_off[pl_targets] and the bins of its insert histogram (max_insert + 1)
    uint64_t    pl_final_epoch = 0;                // ... made on the final result of this epoch (0: on caller's targets)
    alga_placements pl_out{};                      // ... the handle that was handed out for it (stage_common.h: alga_placement_is_current)
    uint64_t    fc_epoch = 0;                      // counts the alga_final_contigs_device calls that wrote a result
    int         opt_place_dir_bits = 0;            // option "place_dir_bits": bits of the seed index's directory, 0 = about two positions per bucket
    // the placed targets voted again (engine_polish.hip).  Workspaces: counters, the (first column, node) pairs before and after the sort, the
    // per-word masks, their popcounts and the scan.  The result: its own copy of col_off, the polished column array, the change list, the
    // per-target sums (changed, ambiguous), the optional counts
    DevBuf      po_cnt, po_keys[2], po_vals[2], po_marks, po_pop, po_scan;
    DevBuf      po_coloff, po_words, po_ccols, po_cbases, po_tstat, po_counts;
    bool        po_valid = false;                  // the result buffers hold a polish
    uint64_t    po_targets = 0, po_columns = 0;    // ... of this many targets and columns
    uint64_t    po_final_epoch = 0;                // ... of a placement on the final result of this epoch (0: on caller's targets)
    alga_polished po_out{};                        // ... the handle that was handed out for it (alga_polished_is_current)
    uint64_t    pl_serial = 0, po_pl_serial = 0;   // counts the placement results written; the one the polish at hand was made from
    // the chain workspace of the call at hand (chain_kernels.hip: alga_chain_work carves it for the scaffolder, the merge and the stitch stage): the
    // two sets of lists over the 2T states, the join of every end, head / first / members and their scans.  Nothing in it outlives a call and no
    // result handle points into it; a stage call ends with the wait for its stream (AlgaStageCall), so the stages take it in turn
    DevBuf      chain_work;
    // scaffolds from split pairs (engine_scaffold.hip).  Workspaces: counters, the link keys / judging reads before and after the sort, the spans,
    // the heads and their scan, the first link of every bundle, best / second / choice / partner / join bundle per end.  The result: the bundle
    // arrays, the end states, the per-contig and per-scaffold arrays
    DevBuf      sc_cnt, sc_keys[2], sc_vals[2], sc_span, sc_heads, sc_pos, sc_bstart, sc_best, sc_choice, sc_partner;
    DevBuf      sc_ba, sc_bb, sc_blinks, sc_bspan, sc_bgap, sc_bstate, sc_estate, sc_scaffold, sc_rank, sc_orient, sc_start, sc_gapafter, sc_jlinks, sc_soff,
                sc_smembers, sc_slen;
    int         opt_scaffold_max_blocks = 8192;    // option "scaffold_max_blocks": the cap of the k_sc_* grids (tests make every grid-stride loop take further passes)
    bool        sc_valid = false;                  // the result buffers hold scaffolds
    uint64_t    sc_targets = 0, sc_scaffolds = 0, sc_longest = 0;   // ... of this many targets, this many of them, the longest with its gaps
    uint64_t    sc_pl_serial = 0;                  // ... made from this placement result
    // contigs broken where no proper pair spans them (engine_break.hip).  Workspaces: counters, the difference array, the run starts and their
    // scan, the marks per column, first / last / closed per run and the scan of the closed ones.  The result: the span (entry g + 1 of the scan
    // of the differences), the cuts, the cuts per target, the piece arrays, the result's own copy of the bases
    DevBuf      br_cnt, br_diff, br_starts, br_rpos, br_marks, br_rfirst, br_rlast, br_closed, br_cpos;
    DevBuf      br_span, br_ccols, br_cfirst, br_clast, br_tcuts, br_poff, br_begin, br_len, br_ptarget, br_pstart, br_words;
    bool        br_valid = false;                  // the result buffers hold a break result
    uint64_t    br_targets = 0, br_pieces = 0, br_cuts = 0, br_columns = 0, br_longest = 0;   // ... of this many targets, pieces, cuts, columns; the longest piece
    // contig ends grown with the reads that hang over them (engine_grow.hip).  Workspaces: counters, the candidate flags, their scan and the
    // list, the end lengths and their scan, the end sequences, the growth per end and its bases.  The result, twice: a call writes the set
    // that is not the current one and swaps it in at its end, so a call that fails anywhere leaves the earlier result as it was
    DevBuf      gr_cnt, gr_flag, gr_pos, gr_cand, gr_elen, gr_eoff, gr_ecols, gr_x, gr_g;
    struct GrowSet { DevBuf end, over, mm, hits, state, count, estop, evoters, left, right, len, coloff, begin, words; } gr_set[2];
    int         gr_cur = 0;                        // the set that holds the result
    int         opt_grow_max_blocks = 8192;        // option "grow_max_blocks": the cap of the k_gr_* grids, k_gr_place's and the FASTA write grid's included (tests make every grid-stride and wave-stride loop take further passes)
    bool        gr_valid = false;
    uint64_t    gr_reads = 0, gr_targets = 0, gr_columns = 0, gr_longest = 0;   // ... of this many reads, targets and columns; the longest grown target
    // contigs whose ends overlap merged into one sequence (engine_merge.hip).  Workspaces: counters, the end lengths, their padded lengths and
    // the scan, the end sequences and their reverse complements.  The result, twice, as for the grow
    DevBuf      mg_cnt, mg_elen, mg_epad, mg_eoff, mg_ecols, mg_pcols;
    struct MergeSet { DevBuf partner, olen, mm, hits, estate, merged, rank, orient, start, ovafter, moff, mmembers, len, coloff, begin, words; } mg_set[2];
    int         mg_cur = 0;                        // the set that holds the result
    int         opt_merge_max_blocks = 8192;       // option "merge_max_blocks": the cap of the k_mg_* grids (tests make every grid-stride loop take further passes)
    bool        mg_valid = false;
    uint64_t    mg_targets = 0, mg_merged = 0, mg_columns = 0, mg_longest = 0;   // ... of this many targets, merged contigs and columns; the longest merged contig
    // contigs contained in another contig dropped (engine_contain.hip).  Workspaces: counters, the padded lengths and their scan, the targets and
    // their reverse complements in a column space of their own, what k_ct_contain leaves per (c, s), the kept flags and their scan.  The
    // result, twice, as for the grow (the roots in both buffers of the pointer jumping: the handle names the one the last round wrote)
    DevBuf      cn_cnt, cn_pad, cn_off, cn_cols, cn_rcols, cn_qmm, cn_qhits, cn_qhost, cn_qpos, cn_keep, cn_keepscan;
    struct ContainSet { DevBuf host, hostpos, hostorient, mm, hits, state, root[2], rootpos[2], rootorient[2], absorbed, newid, old, len, coloff, begin, words; } cn_set[2];
    int         cn_cur = 0;                        // the set that holds the result
    int         opt_contain_max_blocks = 8192;     // option "contain_max_blocks": the cap of the k_ct_* grids but k_ct_contain's and the FASTA kernels' (tests make every grid-stride loop take further passes)
    bool        cn_valid = false;
    uint64_t    cn_targets = 0, cn_kept = 0, cn_columns = 0, cn_longest = 0;   // ... of this many targets, kept targets and columns; the longest kept target
    // scaffold joins whose contig ends overlap stitched into one sequence (engine_stitch.hip).  Workspaces of its own: counters, the per-end
    // count, the per-end arrays the merge stage's launchers take (partner, olen, mm, hits, state), begin / len of a placement's targets.  The
    // result, twice, as for the grow
    DevBuf      st_cnt, st_endcnt, st_epartner, st_eolen, st_emm, st_ehits, st_estate, st_tbegin, st_tlen;
    struct StitchSet { DevBuf jolen, jmm, jhits, jstate, endentry, stitched, rank, orient, start, ovafter, soff, smembers, len, coloff, begin, words; } st_set[2];
    int         st_cur = 0;                        // the set that holds the result
    int         opt_stitch_max_blocks = 8192;      // option "stitch_max_blocks": the cap of the k_st_* grids and of the merge stage's kernels launched from the stitch (tests make every grid-stride loop take further passes)
    bool        st_valid = false;
    uint64_t    st_targets = 0, st_entries = 0, st_stitched = 0, st_columns = 0, st_longest = 0;   // ... of this many targets, entries, stitched contigs and columns; the longest stitched contig
    // the unplaced reads laid with indels (engine_gapped.hip).  Workspaces: counters, the participation flags, their scan and the list, this
    // stage's column array, the best key per participating read, the strided runs and their numbers, the difference array and its scan.  The
    // result: per read target / pos / end / edits / state, the CIGAR offsets and runs, the cover, the per-target sums
    DevBuf      gp_cnt, gp_flag, gp_pos, gp_list, gp_cols, gp_best, gp_runs, gp_nruns, gp_diff, gp_scan;
    DevBuf      gp_target, gp_rpos, gp_end, gp_edits, gp_state, gp_cigoff, gp_cigar, gp_cover, gp_tstat;
    bool        gp_valid = false;                  // the result buffers hold a gapped placement
    uint64_t    gp_reads = 0, gp_targets = 0, gp_columns = 0, gp_ncigar = 0;   // ... of this many reads, targets and columns; its runs
    uint64_t    gp_pl_serial = 0;                  // ... made from this placement result
    uint64_t    gp_serial = 0;                     // counts the gapped results written
    alga_gapped gp_out{};                          // the handle that was handed out for the gapped result at hand (alga_gapped_is_current)
    // the pair calls over both passes (engine_sam.hip).  Workspace: counters.  The result: FLAG and TLEN per read, the insert histogram
    DevBuf      sj_cnt, sj_flag, sj_tlen, sj_hist;
    bool        sj_valid = false;                  // the result buffers hold pair calls
    uint64_t    sj_reads = 0, sj_nhist = 0;        // ... of this many reads, with this many bins
    uint64_t    sj_pl_serial = 0, sj_gp_serial = 0;   // ... made from this placement and this gapped result (0: without one)
    int         opt_sam_max_blocks = 0;            // option "sam_max_blocks": the cap of the k_sam_* grids, 0 = the launches' own (tests make the loops take further passes)
    // the placed targets voted by the Hamming-placed and the gapped reads together (engine_ipolish.hip).  Workspaces: counters, the H voters'
    // (first column, node) pairs before and after the sort and what the polish's vote kernels write beside their counts, the four counts and the
    // `-` votes per column, the difference array of the span and its scan, the insertion votes (key, slot) before and after their two sorts, the
    // winner / its votes / all votes per slot, width / events / verdict per old column and the scan of the events.  The result, twice, as for
    // the grow
    DevBuf      ip_cnt, ip_keys[2], ip_vals[2], ip_marks, ip_pop, ip_pwords, ip_ptstat, ip_counts4, ip_del, ip_diff, ip_scan, ip_ikey[2], ip_islot[2], ip_winkey,
                ip_winvotes, ip_insall, ip_width, ip_evn, ip_evoff, ip_code;
    struct IpolishSet { DevBuf len, coloff, begin, words, newcol, evcol, evkind, evlen, evbases, evvotes, evcover, tstat, counts, span, oldoff; } ip_set[2];
    int         ip_cur = 0;                        // the set that holds the result
    int         opt_ipolish_max_blocks = 8192;     // option "ipolish_max_blocks": the cap of the k_ip_* grids (tests make every grid-stride loop take further passes)
    bool        ip_valid = false;
    uint64_t    ip_targets = 0, ip_columns = 0, ip_columns_before = 0, ip_events = 0, ip_longest = 0;   // ... of this many targets, new and old columns, events; the longest new target
    // seed-bucket-sharded N-GPU build (engine_shard.hip): state between its phases (the exchanges in between are the caller's)
    DevBuf      sh_keys[2], sh_vals[2], sh_store, sh_dir, sh_desc_out, sh_dkey[2], sh_dval[2], sh_small_top, sh_pending, sh_bitmap, sh_small_out,
                sh_ssrc[2], sh_skey[2], sh_edges_out, sh_deg, sh_rowptr, sh_cursor, sh_edges, sh_flagged, sh_cnt, sh_gflag, sh_gpos, sh_gstart;
    struct {
        int      phase = 0;                    // 0 none, 1 indexed, 2 joined, 3 small keys listed, 4 resolved
        int      rank = 0, n_ranks = 1, eq = 0, uniform_len = 0;
        int32_t  n = 0;
        const void *words = nullptr;
        alga::PrefSufCfg cfg{};
        alga::ClusterCfg cc{};
        uint32_t bucket_base = 0, bpr = 0;
        uint64_t n_targets = 0, n_desc = 0, n_rec = 0;
        uint32_t *d_keys_sorted = nullptr;     // descriptors of the last join, sorted by bucket
        unsigned long long *d_vals_sorted = nullptr;
    } sh;
    alga_shard_stats shard_stats{};
    // the approximate supplement between its phases (engine_pkb.hip: begin / round / merge / end)
    struct {
        int      phase = 0;                    // 0 none, 1 between rounds, 2 a round's additions are out, their merge pending
        int      rounds = 0, round = 0, rank = 0, n_ranks = 1, cur = 0, key_bits = 0;
        int32_t  prio[4] = {0, 1, 2, 3};
        uint64_t E = 0, nk = 0;
        uint32_t n_tips = 0;
        int      pre_set = 0, cur_set = 0;     // which of the two sets (engine_pkb.hip: PkbSet) the look-ahead fills / the round at hand works on
        bool     no_look_ahead = false;        // the look-ahead's buffers did not fit: this sequence runs its rounds one after the other
        int      pre_round = -1;               // the round whose sort -> repair -> heads were sent ahead on side_stream (their counts: h_counters + H_PRE), -1 none
        bool     kmers_all = false;            // the k-mer entries of every round are in pk_keys_all / pk_vals_all (made in round 0), kmers_stride entries apart
        size_t   kmers_stride = 0;
        int      kmers_sort_bits = 0;
        alga_nodes dn{};
        alga::PkbCfg cfg{};
    } pkb;
    unsigned long long *h_counters = nullptr;  // pinned, CNT_TOTAL + 2 entries + H_EXTRA more (supplement: the class bounds of a round, 257 x u32)
    static constexpr int H_EXTRA = 132 + 16, H_PRE = alga::CNT_TOTAL + 2 + 132;       // (H_PRE: 13 counts of the look-ahead, in 64-bit words from the block's start)
    uint32_t *h_counters_dev = nullptr;         // the same block by its device address (launch_mail writes it from a kernel)
    uint64_t    rec_cap_hint = 0, rec_cap_hint_local = 0;
    alga_prefsuf_stats stats;
    double      stats_host[2] = {0.0, 0.0};   // upload_nodes_impl: wall ms of its checks / of the upload (the host entry points copy them into stats)
    alga_pkb_stats pkb_stats;
};

// what prepare() (engine.hip) derives from a build's arguments and the node statistics
struct AlgaPrepared {
    alga::NodesDev   nd;
    alga::PrefSufCfg cfg;
    int        max_len = 0;
    int        uniform_len = 0;      // > 0: every live node has this length and there is no alignFrom mask
    uint64_t   live = 0;
    bool       local_ok = false;     // the source-side reduction is exact for this input
    int        local_sw = 1;         // ... with one or two 64-bit words per offset mask / uint4 per overhang
    int        cluster_eq = 0;       // clustered minimizer probe: 16-byte pieces per entry (0 = that probe does not take this input)
    alga::ClusterCfg cluster{};
    int        reduction = ALGA_REDUCTION_AUTO;
    int        keys_shared = 0;      // 1: the per-node keys come from alga_prefsuf_keys_device + the caller's all-gather; 2: the whole
                                     // entry array of the previous build of this node set is reused
};

// the upload of a host node set in two phases (engine.hip: upload_nodes_impl; mode 1 = my slice of the rows + all lengths, 2 = finish once the raw
// buffer is complete): what alga_multi_prefsuf_build_host shards over the ranks
extern "C" int alga_upload_nodes_phase(alga_engine *e, const alga_nodes *nodes, bool twin_rows, int mode, uint64_t row_begin, uint64_t row_end, uint64_t raw_rows_cap, alga_nodes *dev,
                            uint32_t **d_raw);
int alga_prepare(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, hipStream_t s, AlgaPrepared &out);
int alga_cluster_alloc(alga_engine *e, const AlgaPrepared &pp);

inline int alga_fail(alga_engine *e, int code, const char *what, hipError_t herr = hipSuccess) {
    char buf[512];
    if (herr != hipSuccess) snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(herr));
    else snprintf(buf, sizeof(buf), "%s", what);
    e->err = buf;
    return code;
}

#define HIP_TRY(e, call)                                                                     \
    do {                                                                                     \
        hipError_t _err = (call);                                                            \
        if (_err != hipSuccess) return alga_fail((e), _err == hipErrorOutOfMemory ? ALGA_ERR_OUT_OF_MEMORY : ALGA_ERR_HIP, #call, _err); \
    } while (0)

// Every device buffer of an engine is allocated here, and remembered: alga_engine_destroy releases what this function handed out
// (a hand-written list of the members missed the buffers later rounds added).
inline int alga_ensure(alga_engine *e, DevBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return ALGA_OK;
    if (b.p) { HIP_TRY(e, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    else if (std::find(e->owned.begin(), e->owned.end(), &b) == e->owned.end()) e->owned.push_back(&b);
    HIP_TRY(e, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return ALGA_OK;
}

// Engine-owned node storage (uploads, the output of the device input stage) is about to be rewritten: nothing derived from the
// node set that lived there -- key pass, entry array, node statistics -- may be reused by a later build (they are matched on
// addresses and sizes, which a rewrite does not change).
inline void alga_forget_node_set(alga_engine *e) {
    e->keyed_n = -1; e->store_n = -1; e->pile_n = -1;
    e->stat_len = nullptr; e->stat_from = nullptr; e->stat_to = nullptr;
}

// the largest length l such that the sequences of length >= l hold at least half of all bases
inline uint64_t n50_of(std::vector<uint64_t> v) {
    std::sort(v.begin(), v.end(), [](uint64_t a, uint64_t b) { return a > b; });
    unsigned __int128 total = 0, cum = 0;
    for (uint64_t x : v) total += x;
    if (total == 0) return 0;
    for (uint64_t x : v) { cum += x; if (2 * cum >= total) return x; }
    return 0;
}

inline void alga_release(DevBuf &b) {
    if (b.p) (void) hipFree(b.p);
    b.p = nullptr; b.cap = 0;
}

#include <chrono>
#include <functional>
typedef std::function<void(void * /* pinned chunk */, size_t /* byte offset of the chunk */, size_t /* bytes */)> AlgaStageFill;
int  alga_staged_h2d(alga_engine *e, void *d_dst, const void *h_src, size_t bytes);   // staging.hip: blocking
int  alga_staged_h2d_fill(alga_engine *e, void *d_dst, size_t bytes, const AlgaStageFill &fill);
int  alga_staged_d2h(alga_engine *e, void *h_dst, const void *d_src, size_t bytes);
void alga_staging_release(alga_engine *e);
void *alga_host_list_take(alga_engine *e, size_t bytes);
void alga_host_list_give(alga_engine *e, void *p);

// engine_unitig.hip, shared with engine_contig.hip: the device's verdict on a node set and edge list (unitig step 1), E* with its row pointers
// (step 2, into ut_estar / ut_rowptr), and the list ranking along nxt[] in both forms with the cycle-minimum jump (records: ut_rank[cur]).
// cnt: UT_COUNTERS + ALGA_UT_MAX_ROUNDS zeroed 64-bit words; a ranking uses one word per jump round from cnt[UT_COUNTERS + rounds] on.
constexpr int ALGA_UT_MAX_ROUNDS = 112;            // three ranking phases (rulers, nodes, nodes after the cuts) of at most 34 rounds each
int alga_ut_check(alga_engine *e, const alga_nodes *nodes, const alga::alga_edge_dev *d_in, uint64_t m, unsigned long long *cnt, hipStream_t s);
int alga_ut_estar(alga_engine *e, const alga_nodes *nodes, const alga::alga_edge_dev *d_in, uint64_t m, unsigned long long *cnt, hipStream_t s, uint64_t *ms_out);
int alga_ut_rank(alga_engine *e, const int32_t *len, int32_t n, int32_t *nxt, const int32_t *noff, int32_t *prv, unsigned long long *cnt, uint32_t *p_flag,
                 int &cur, int &rounds, hipStream_t s);

// engine_gfa.hip: the chunk pipeline of every text output (sizes -> 64-bit scan -> chunks formatted on the device, copied down and written by a
// host thread) over items that another file sizes and formats.  sizes: fill sizes[0 .. items) and counters[GFA_SEGMENTS] / [GFA_MAX_LINE] (zeroed);
// format: the text of items [i0, i1) into buf, item i at byte off[i] - off[i0].  An error removes the partial file.
struct AlgaTextJob {
    uint64_t items;
    std::function<void(uint32_t *sizes, unsigned long long *counters, hipStream_t s)> sizes;
    std::function<void(const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s)> format;
    const char *kind = "FASTA";       // what the I/O error messages call the file
    const char *head = "";            // the text before the first item
    // optional: what has to hold or exist before the sizes (the device's verdict on the input, tables); an error code ends the job
    std::function<int(unsigned long long *counters, hipStream_t s)> prepare;
    // optional: the verdict on the counters the sizes pass left, as they came back (host copy); an error code ends the job before the file is touched
    std::function<int(const unsigned long long *h_counters)> verdict;
};
int alga_text_job_run(alga_engine *e, const AlgaTextJob &job, const char *path, alga_gfa_info *info,
                      std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now());

// the job of records that a launch_*_sizes / launch_*_write pair formats from one struct `f` (f.n items)
template <class F> int alga_text_records(alga_engine *e, const F &f, void (*sizes)(const F &, uint32_t *, unsigned long long *, hipStream_t),
                                         void (*write)(const F &, const unsigned long long *, uint64_t, uint64_t, char *, hipStream_t), const char *path,
                                         alga_gfa_info *info, std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now()) {
    AlgaTextJob job;
    job.items = f.n;
    job.sizes = [f, sizes](uint32_t *out, unsigned long long *counters, hipStream_t s) { sizes(f, out, counters, s); };
    job.format = [f, write](const unsigned long long *off, uint64_t i0, uint64_t i1, char *buf, hipStream_t s) { write(f, off, i0, i1, buf, s); };
    return alga_text_job_run(e, job, path, info, t0);
}

// engine_correct.hip: the correction of device-resident rows in the parser's layout, in place (what alga_correct_reads_device and the corrected
// ingest share); the parameters are checked by the callers (alga_correct_check_params)
int alga_correct_check_params(alga_engine *e, const alga_correct_params *p);
int alga_correct_impl(alga_engine *e, uint32_t *d_rows, int32_t stride, const int32_t *d_len, int64_t n_nodes, const alga_correct_params *p, hipStream_t s,
                      alga_correct_info *info);

// engine_final.hip: `u` / `cons` / `fin` are the engine's current unitig, consensus and final results (else *why says which is not)
bool alga_final_is_current(const alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, const alga_final_contigs *fin, const char **why);

inline int alga_check_launch(alga_engine *e, const char *what) {
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return alga_fail(e, ALGA_ERR_HIP, what, err);
    return ALGA_OK;
}

#include "stage_common.h"
