/*
 * include/alga_amd.h -- C ABI of the MI355X (gfx950) overlap-graph engine for the ALGA assembler.
 *
 * This is the drop-in boundary for ONE path of swacisko/ALGA: the overlap-graph construction that
 * sits behind `class GraphCreator` (reference include/GraphCreators/GraphCreator.h:12-62) and is
 * selected in src/main.cpp:246-250.  Plain pointers and sizes only; no C++/torch types.
 * The reference-side bindings (GraphCreator subclasses that marshal to these calls) are
 * the headers under alga_amd/host/adapter/, described in INTEGRATION.md.  Paths below are relative to the reference root.
 *
 * Conventions
 *   - every call returns 0 on success or a negative alga_status; alga_last_error() gives the text.
 *     (the reference's convention is cerr + exit(1), e.g. src/DataStructures/Read.cpp:146-149; the
 *     adapter maps a non-zero status to that.)
 *   - the engine borrows caller memory and never frees it (GraphCreator::~GraphCreator only nulls
 *     its pointers, src/GraphCreators/GraphCreator.cpp:15-18); buffers the engine returns are
 *     released with alga_free_edges().
 *   - calls block until the result is complete (the reference joins its worker threads before
 *     returning, src/GraphCreators/GraphCreatorPrefSuf.cpp:147-161); one engine handle must not be
 *     used from two threads at once, different handles are independent.
 *   - there is NO CPU fallback: without a usable HIP device every compute call fails.
 */
#ifndef ALGA_AMD_H
#define ALGA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALGA_AMD_ABI_VERSION 7

typedef enum {
    ALGA_OK = 0,
    ALGA_ERR_INVALID_ARGUMENT = -1,
    ALGA_ERR_NO_DEVICE = -2,        /* no HIP device / HIP runtime failure at start-up        */
    ALGA_ERR_HIP = -3,              /* a HIP call or kernel failed                            */
    ALGA_ERR_OUT_OF_MEMORY = -4,
    ALGA_ERR_CAPACITY = -5,         /* an internal 32-bit index space would overflow; shard   */
    ALGA_ERR_IO = -6,
    ALGA_ERR_UNSUPPORTED = -7       /* the requested reduction form is not exact for this input: use the other one */
} alga_status;

/* Where the transitive reduction of GraphCreatorPrefSuf.cpp:397-483 is evaluated (same result either way):
 *   PER_TARGET  : the literal replay of the reference's push order per target node (any input);
 *   SOURCE_SIDE : per source node inside the probing wave, from the source's own raw overlaps;
 *                 exact when max_len <= max_len_cap, max_len - min_overlap <= 127, min_overlap <= rsoe_min_overlap <=
 *                 min(max_len, max_len_cap) + 1 and no live node has alignFrom without alignTo -- everything ALGA's
 *                 command line can produce for reads up to ~280 nt after trimming with the default scale.
 *   AUTO        : SOURCE_SIDE when those conditions hold (checked on the device), else PER_TARGET. */
typedef enum { ALGA_REDUCTION_AUTO = 0, ALGA_REDUCTION_PER_TARGET = 1, ALGA_REDUCTION_SOURCE_SIDE = 2 } alga_reduction;

/* Which probe finds the raw overlaps of the SOURCE_SIDE form (same result either way):
 *   TABLE   : bucketised seed table, one probe per (source, overlap length) -- takes any input;
 *   CLUSTER : clustered minimizer join -- targets sorted by the minimizer of their min_overlap-long prefix, ~3 contiguous
 *             lookups per source; takes max_len - min_overlap <= 127 and reads of up to 272 nt (round 4: 250-bp reads too, in the
 *             two-word form of the source-side reduction through its general kernel; up to 63 / 208 nt through k_probe_stream),
 *             anything else uses TABLE;
 *   AUTO    : CLUSTER whenever it takes the input (1.8x faster at 1.7 M nodes, 2.9x at 90 M) -- for the wide shapes (span > 63 or
 *             reads > 208 nt) from 4 M live nodes on (below, table and rows are cache-resident and TABLE is faster) --, else TABLE. */
typedef enum { ALGA_PROBE_AUTO = 0, ALGA_PROBE_TABLE = 1, ALGA_PROBE_CLUSTER = 2 } alga_probe;

typedef struct alga_engine alga_engine; /* opaque */

/* Directed overlap edge src -> dst: "dst starts at position `offset` of src"
 * == one (neighbor, offset) pair of Graph::V[src] (include/DataStructures/Graph.h:54,97). */
typedef struct { int32_t src, dst, offset; } alga_edge;

/* Node set = what GraphCreator's constructor receives as `vector<Read*>* reads`:
 * 2-bit packed reads, nucleotide i in bits (2i, 2i+1) of a little-endian bit string held in
 * uint32 blocks, A0 C1 G2 T3, unused tail bits zero (include/DataStructures/Bitset.h:41-50,
 * src/DataStructures/Read.cpp:40-68).  len[i] == 0 means READS[i] == nullptr. */
typedef struct {
    const uint32_t *words;   /* n rows of `stride_words` uint32                                  */
    int32_t         stride_words; /* >= ceil(2*max_len/32)                                       */
    const int32_t  *len;     /* n lengths in nucleotides                                         */
    int32_t         n;       /* number of nodes == Graph::size()                                 */
    const uint8_t  *align_from; /* n bytes or NULL (= all 1): GraphCreator::alignFrom            */
    const uint8_t  *align_to;   /* n bytes or NULL (= all 1): GraphCreator::alignTo              */
} alga_nodes;

/* Parameters GraphCreatorPrefSuf reads from Params:: globals. */
typedef struct {
    int32_t min_overlap;      /* Params::MIN_OVERLAP_PREF_SUF                                    */
    int32_t rsoe_min_overlap; /* Params::REMOVE_SMALL_OVERLAP_EDGES_MIN_OVERLAP                   */
    int32_t soes;             /* small-overlap edges kept per source; the reference hard-codes 3
                                 (include/GraphCreators/GraphCreatorPrefSuf.h:62)                 */
    int32_t max_len_cap;      /* 500 (src/GraphCreators/GraphCreatorPrefSuf.cpp:92)               */
    int32_t collect_stats;    /* != 0: fill the work counters of alga_prefsuf_stats               */
    int32_t reduction;        /* alga_reduction; SOURCE_SIDE fails with ALGA_ERR_UNSUPPORTED when not exact */
    int32_t keys_shared;      /* sharded form only.  1: the per-node keys were made by alga_prefsuf_keys_device and
                                 all-gathered by the caller; the build skips its own key pass.  2: this build follows
                                 another build of the SAME node set on this engine (nothing else in between) and reuses
                                 its index: only the probe of [src_begin, src_end) runs.  A previous build that the pile path
                                 KEPT (reads of one length, no masks, the sample found the buckets regular: option "pile")
                                 has no entry array: the piece goes through its piles (k_pile_probe over the piece's ids;
                                 with option "pile_range" 0 it is refused with ALGA_ERR_INVALID_ARGUMENT, as until round 5);
                                 after a build the pile path declined the entry array serves the piece as before        */
    int32_t twin_rows;        /* host entry points only.  1: nodes->words holds the rows of the ODD nodes alone (row k = node 2k + 1,
                                 n / 2 rows): node 2k is the reverse complement of node 2k + 1 -- ALGA's layout (src/IO/InputReader.cpp:
                                 78-80,363-377; the duplicate removal deletes twins together, src/main.cpp:150-232) -- and its row is
                                 rebuilt on the device from len[2k] (0 = removed, else == len[2k + 1]); half of the PCIe upload.  len and
                                 the masks keep all n entries                                                                           */
} alga_prefsuf_params;

/* Work counters; the first four mirror GATHER_STATISTICS of the reference
 * (include/GraphCreators/GraphCreatorPrefSuf.h:112-118). */
typedef struct {
    uint64_t raw_overlaps;        /* goodPrefSufChecks: suffix==prefix pairs found               */
    uint64_t transitive_listed;   /* bitsetChecksCount: in-list entries visited by big overlaps  */
    uint64_t transitive_compares; /* goodBitsetChecksCount: 2-bit compares started               */
    uint64_t transitive_removed;  /* bitsetCheckEdgesRemoved                                     */
    uint64_t windows_probed;      /* (node, overlap length) seed-table probes                    */
    uint64_t slots_scanned;       /* seed-table slots read while probing                         */
    uint64_t records;             /* overlap records kept after the small-overlap cap            */
    uint64_t edges;               /* edges in the result                                         */
    uint64_t table_slots;         /* seed-table capacity                                         */
    uint64_t max_in_records;      /* largest per-target record list                              */
    double   ms_total;            /* device time of the last call, HIP events on the engine's stream */
    double   ms_seed, ms_probe, ms_group, ms_reduce, ms_emit;
    uint64_t nodes_live;          /* nodes with len>0                                            */
    uint64_t reduction_used;      /* alga_reduction of the last build (1 or 2)                   */
    uint64_t generic_sources;     /* SOURCE_SIDE: sources that needed the all-pairs path (collect_stats) */
    uint64_t big_sources;         /* SOURCE_SIDE: sources with more raw overlaps than a wave's LDS holds (second pass) */
    uint64_t probe_used;          /* alga_probe of the last build (1 or 2)                       */
    uint64_t deferred_sources;    /* CLUSTER probe: sources the first kernel handed to the general kernel (all of them when it was skipped) */
    double   ms_probe_pairs;      /* CLUSTER probe: the first kernel's (k_probe_stream) part of ms_probe (0: not run) */
    double   ms_keys, ms_sort, ms_gather, ms_dir; /* CLUSTER probe: the parts of ms_seed -- k_node_runs, radix sort of (key, id),
                                     k_tgt_gather, k_tgt_dir (0 for a build that reused them: keys_shared)         */
    uint64_t probe_rounds;        /* CLUSTER probe, k_probe_stream: rounds = wave iterations (collect_stats); sources / rounds = sources packed per round */
    double   ms_pile;             /* CLUSTER probe, option pile: k_pile_build (consensus records of the entry array), part of ms_seed; 0: not run  */
    uint64_t pile_buckets, pile_irregular;   /* ... non-empty buckets in a SAMPLE of the key order (its first 1/32; an eighth of the sample's entries where that
                                     is more: a bucket of a high-coverage read set stands for more pairwise work saved) / those of them the pile path does
                                     not take (a source with a run in such a bucket goes to the general kernel); more than 1 in
                                     ALGA_PILE_IRREGULAR_ONE_IN irregular: the pairwise kernel k_probe_stream took the build instead of k_pile_probe */
    uint64_t pile_list_checked, pile_list_mismatch;   /* option "pile_check" (tests): first-group members whose own run list was compared with their pile's
                                     consensus-derived list clipped to their windows / those for which the two differ (must be 0) */
    uint64_t pile_own_lists;      /* pile path (option pile_runs): entries of the key order that read a run list of their OWN -- outside a first group, or members of a
                                     pile whose consensus gave no list -- and got it from the list-driven key pass (0: every node's list was made up front) */
    double   host_ms_check, host_ms_upload, host_ms_build, host_ms_download;   /* host entry points (alga_prefsuf_build_host*): wall time of the argument / length
                                     checks, of the upload (staging, re-stride / twin expansion included), of the build, of the download of the edges */
    uint64_t pile_mixed;          /* 1: the pile path kept a build with more than 1 irregular bucket in ALGA_PILE_IRREGULAR_ONE_IN (but not more than 1 in
                                     ALGA_PILE_DECLINE_ONE_IN): the sources k_pile_probe handed on went through k_probe_stream first                       */
    uint64_t pile_deferred;       /* sources k_pile_probe handed on (deferred_sources: what reached the general kernel in the end)                          */
} alga_prefsuf_stats;
/* The pile path keeps a build iff  pile_irregular * ALGA_PILE_IRREGULAR_ONE_IN <= pile_buckets  (decided on the device; pile_buckets as reported: raised to
 * an eighth of the sample's entries at high coverage).  Every source with a run in an
 * irregular bucket goes to the general kernel -- eight times the buckets' share of the sources, at ~20 times the cost per source: above ~0.5 % of
 * irregular buckets the pairwise kernels are faster (reads with sequencing errors: 25 %; error-free reads of a genome of 1 Gb: 1.5 %, 250 Mb: 0.07 %). */
#define ALGA_PILE_IRREGULAR_ONE_IN 250
/* Round 5: above that share the pile path still keeps the build as long as  pile_irregular * ALGA_PILE_DECLINE_ONE_IN <= pile_buckets  -- the sources
 * it hands on then go through the pairwise stream kernel (k_probe_stream over the list; the entry array is built for it) and only what that cannot
 * finish reaches the general kernel: ~0.3 instead of ~2 ms per million sources handed on.  Beyond it (reads with sequencing errors) the pairwise
 * kernels take the whole build as before.  alga_prefsuf_stats.pile_mixed tells which form ran. */
#define ALGA_PILE_DECLINE_ONE_IN 20

/* ---- lifetime --------------------------------------------------------------------------- */
int         alga_abi_version(void);
int         alga_engine_create(int hip_device, alga_engine **out);
void        alga_engine_destroy(alga_engine *e);
const char *alga_last_error(const alga_engine *e);      /* valid until the next call on `e`     */
int         alga_engine_device_name(const alga_engine *e, char *buf, size_t buflen);

/* Engine switches.  None changes a result, only how it is computed; there are no environment variables.
 *   "probe"                      alga_probe (default AUTO)
 *   "cluster_bucket_bias"        -8..8: log2 factor on the bucket count of the CLUSTER probe's index (default 0: ~1 entry per bucket)
 *   "cluster_pairs"              0: the CLUSTER probe runs its general kernel only (one source per wave); default 1: k_probe_stream first
 *                                (the entries of consecutive sources packed densely onto the lanes), the general kernel on what it defers
 *   "pile"                       default 1: reads of one length without masks take the probe through PILES (alga_amd/csrc/prefsuf_pile.hip): one compare
 *                                of a source against the consensus of a minimizer's targets instead of one per target; 0: always the pairwise kernels;
 *                                2 (tests only): without the sample that leaves reads with errors to the pairwise kernels; 3 (tests only): without it, in
 *                                the MIXED form (ALGA_PILE_DECLINE_ONE_IN below): what the pile kernel hands on goes through k_probe_stream by list
 *   "pile_runs"                  default 1: the run list of a pile (what its members probe with) is computed from the pile's CONSENSUS, once per pile
 *                                (k_pile_runs_consensus), and the key pass of a build the pile path keeps makes the target keys alone -- own run lists
 *                                only for the entries outside a first group and the sources handed to the general kernel; 0: round 4's form (every
 *                                node its own list, a pile's list joined from its two outer members')
 *   "pile_runs_list"             default 1: k_pile_build lists the piles of each of its workgroups and k_pile_runs_consensus_list takes the piles from
 *                                those lists (four waves per SIMD); 0: k_pile_runs_consensus sweeps the side records for them (round 5; A/B and tests)
 *   "pile_dir"                   where the pile path takes a bucket's record {first entry, entries, class offsets} from.  0: k_pile_build reads the bucket
 *                                directory k_tgt_dir made (until round 7; A/B and tests).  1: k_pile_build (the sample and the build) takes bucket
 *                                starts, counts of at most 64 and the class offsets from the sorted keys of its tile and never reads the directory;
 *                                the sample then runs in front of the directory pass.  2 (default): ... and a build the pile path keeps in its PURE
 *                                form neither fills nor builds the directory (decided on the device, from the sample's counters): the pairwise
 *                                kernels behind the pile kernels read the bucket records from the piles' table.  Declined and mixed builds, "pile" 0,
 *                                a statistics build and "pile_skip_gather" 0 build the directory as before
 *   "pile_deg_fold"              default 1: the first pass of the out-degree scan moves the out-degrees k_pile_probe left in the sources' slots; 0: a
 *                                pass of its own (k_pile_deg) right behind the probe (A/B and tests)
 *   "emit_fused"                 default 1: the source-side emit makes its rows in two passes over the out-degrees and slots (k_emit_tile_sums sums the
 *                                out-degrees of a tile, k_emit_scan_tiles forms their prefix and writes row pointers and slot edges from it); an
 *                                out-degree k_pile_probe left in a slot is read there and never moved to the out-degree array; 0: the scan of the
 *                                out-degree array first, k_local_emit_first behind it (until round 8; A/B and tests)
 *   "pile_probe_lean"            default 1: k_pile_probe takes a source's row from its home run in slot 0 only and looks for the last mismatch
 *                                below position 64 only (a mismatch from 64 on clears the whole offset set); 0: the round-5 kernel (A/B and tests)
 *   "pile_probe_tail"            default 1 (with "pile_probe_lean" 1): the end of a tile of k_pile_probe asks for memory in batches -- the look-ups of a
 *                                source's one or two standing targets share two round trips (both bucket lines, then four candidates of both m_C
 *                                classes; further batches while a class has more), and the first entry of a further group's bucket is read an
 *                                iteration ahead of the group's record; 0: load by load, as until round 9 (A/B and tests).  Decides nothing
 *   "pile_runs_ahead"            1: k_pile_runs_consensus_list asks for the records of its next round of piles (and the list entries of the
 *                                round after) before it works on the round at hand; default 0: every round reads its piles, then works on them -- at the
 *                                north-star size the look-ahead changed the kernel's time by less than the spread of two runs.  Computes nothing else
 *   "pile_stream_by_id"          1: a build the pile path keeps in its PURE form sends the sources k_pile_probe hands on through k_probe_stream (list
 *                                mode) before the general kernel, as the mixed form does -- the entries taken by id from the sorted (key, id) pairs, since
 *                                the pure form has no entry array; alga_prefsuf_stats.pile_deferred is then what the pile kernel handed on and
 *                                deferred_sources what the general kernel was given; default 0 (until the pass has been measured on the GPU): the
 *                                general kernel takes them all
 *   "pile_check"                 tests only.  != 0: every node gets its own run list as well and every first-group member's is compared with its pile's list
 *                                clipped to the member's windows (alga_prefsuf_stats.pile_list_checked / pile_list_mismatch)
 *   "pile_skip_gather"           default 1: a build the pile path keeps has no entry array (the rows in key order, 48 bytes per node: its kernels
 *                                read the rows by id, and the copy alone costs 3 ms per 90 M nodes); 0: the entry array is always built
 *   "cluster_order"              default 1: k_probe_stream takes the sources in the order of the entry array (sources of one locus together:
 *                                shared look-ups, cache hits); 0: in id order (what a range of ids always gets)
 *   "local_big_max"              largest per-wave item slice of the SOURCE_SIDE second pass (default -1 = built-in 4096); beyond it
 *                                the build takes PER_TARGET
 *   "auto_reduction_per_target"  != 0: alga_prefsuf_params.reduction == AUTO resolves to PER_TARGET
 *   "correct_slice_keys"         1..2^31 (default 2^28): alga_correct_reads_device counts the k-mers in slices of the key space of at most this many
 *                                occurrences (a single histogram bin above it is a slice of its own); tests lower it to run many slices
 *   "correct_dir_bits"           0 (default: about two keys per bucket) or 1..28: bits of the directory over the solid k-mers; tests force long
 *                                buckets and empty ones
 *   "place_dir_bits"             0 (default: about two positions per bucket) or 1..26 (never more than 2k): bits of the directory over the index
 *                                of alga_place_reads_device; tests force long buckets and empty ones
 *   "gfa_chunk_mb"               1..4096 (default 256): alga_write_gfa_device formats the text in chunks of at most this many MB (one device buffer,
 *                                two pinned host buffers of that size; a chunk is never smaller than twice the longest line)
 *   "unitig_ruling"              default -1: the list ranking of alga_unitigs_device ranks a RULING SET first -- the heads and one node in 64 walk to the
 *                                next ruler, the rulers alone are ranked by pointer jumping, a second walk fills in the nodes between them: ~3 gathers
 *                                per node instead of one per node and round (5.5 x faster at 1.7 M nodes) -- from 2^16 nodes on (below, a handful of rounds
 *                                over a cache-resident array costs less than the extra launches); 1: always, 0: never (A/B and tests)
 *   "mst_mid_nodes"              8..2^20 (default 4096): nodes a state of the first overflow tier of alga_remove_short_parallel_paths_device holds (and twice
 *                                as many collected edges); a beg that needs more takes a state sized for the whole graph (tests lower it to reach that tier)
 *   "consensus_max_blocks"       0..2^20 (default 0 = the kernels' own caps): the largest grid of the kernels of alga_unitig_consensus_device; what does not
 *                                fit is done by grid stride (tests lower it to make small inputs stride)
 *   "scaffold_max_blocks"        1..8192 (default 8192): the largest grid of the kernels of alga_scaffold_placed_device and of the write kernel of
 *                                alga_write_scaffold_fasta_device; what does not fit is done by grid stride (tests lower it to make small inputs stride)
 *   "grow_max_blocks"            1..8192 (default 8192): the largest grid of the kernels of alga_grow_placed_device, the placement of the overhanging
 *                                reads (its per-wave scratch follows the grid) and the write kernel of alga_write_grown_fasta_device included; what does
 *                                not fit is done by grid or wave stride (tests lower it to make small inputs stride)
 *   "stitch_max_blocks"          1..8192 (default 8192): the largest grid of the kernels of alga_stitch_targets_device, k_st_overlap's (one wave per
 *                                entry) included; what does not fit is done by grid stride (tests lower it to make small inputs stride)
 *   "contain_max_blocks"         1..8192 (default 8192): the largest grid of the kernels of alga_drop_contained_device but k_ct_contain's (one wave per
 *                                query) and the FASTA kernels'; what does not fit is done by grid stride (tests lower it to make small inputs stride)
 *   "shard_bucket_max"           1..4096 (default 4096): run descriptors of ONE bucket the bucket-sharded join (alga_shard_join_device) takes; a
 *                                bucket with more makes the call answer ALGA_ERR_UNSUPPORTED (tests lower it to exercise that)
 *   "own_sort"                   default 1: the (key, id) sort of the index build and the descriptor sort of the bucket-sharded form are the engine's own
 *                                radix sort (alga_amd/csrc/radix_sort.hip: stable LSD, wave-match ranking, XCD-contiguous tiles); 0: rocPRIM's onesweep
 *                                sort (what rounds 2-4 used; kept for A/B and tests)
 *   "stream_slots"               default 4: k_probe_stream writes the edges of a source with up to four standing items itself (slots beside the source's
 *                                first: 16 B per node more; eight measured no better); 2: two, any other source goes to the general kernel (the form until
 *                                round 4; A/B and tests)
 *   "pile_range"                 default 1: the pile path also takes a build of a source id range (a rank's share of the strong-scaling N-GPU build: the
 *                                index as for all sources, the range's sources compacted for k_pile_probe); 0: all sources only (until round 5; A/B and tests)
 *   "pkb_legacy"                 default 0; A/B and tests: one bit per piece of the approximate supplement that round 5 reworked, set = round 4's form of it:
 *                                1 groups of 8..16 k-mers a wave each (now four per wave), 2 the library's sort of the k-mer entries (now the engine's),
 *                                4 group heads in three kernels (now one), 8 the replay of the 8..16 groups inside the pair kernel, 16 the library's sort /
 *                                unique of the additions and a row-pointer pass, 32 the k-mer walk on a 128-bit value, 64 every tip record's snapshot
 *                                half rewritten every round, 128 a k-mer walk per round (now all rounds in one), 256 a device-to-host copy per count the
 *                                host waits for (now one small kernel per wait writes them into the pinned block), 512 no look-ahead (now the next round's
 *                                k-mer entries are sorted and their groups listed on a second stream beside the round's group joins and merge)
 *   "test_presort_oom"           tests only.  != 0: the allocation of the supplement's look-ahead buffers (a second set of sorted k-mer entries and sort scratch,
 *                                ~50 B per entry) answers ALGA_ERR_OUT_OF_MEMORY: the sequence must give them back and run its rounds one after the other
 *   "test_pile_oom"              tests only.  != 0: the allocation of the pile path's own buffers (~180 B per node) answers ALGA_ERR_OUT_OF_MEMORY: the build
 *                                must give them back and finish on the pairwise kernels (what a real out-of-memory there does)
 *   "test_unsorted_index"        tests only.  != 0: the CLUSTER probe's entry directory is built over UNSORTED keys; the directory pass
 *                                flags it, the probe's reads are clamped to the entry array, and the build returns ALGA_ERR_HIP (no GPU fault) */
int         alga_engine_set_option(alga_engine *e, const char *name, int64_t value);

void        alga_prefsuf_default_params(alga_prefsuf_params *p);

/* ---- the drop-in: GraphCreatorPrefSuf ---------------------------------------------------- */
/* Host buffers in, edges out.  Replaces, for the caller at src/main.cpp:246-291,
 *   new GraphCreatorPrefSuf(READS, G, false); setAlignFrom/To(...); startAlignmentGraphCreation();
 *   G->retainOnlySmallestOffset();
 * The result is the graph the caller would hold at src/main.cpp:293: edges grouped by src,
 * each adjacency list sorted by (dst, offset) (src/DataStructures/Graph.cpp:367-387).
 * *edges is engine-owned host memory; release with alga_free_edges() on the SAME engine and BEFORE alga_engine_destroy():
 * the engine keeps track of the lists it handed out (one released list is kept as a spare for the next call), destroy frees
 * whatever is still outstanding, and a list must not be touched afterwards. */
int  alga_prefsuf_build_host(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p,
                             alga_edge **edges, uint64_t *n_edges);
void alga_free_edges(alga_engine *e, alga_edge *edges);

/* The same build with the graph handed back in COMPACT form -- what crosses PCIe on the way down is 5.1 bytes per edge instead of 12 (the host
 * entry point is PCIe-bound: 0.56 GB instead of 1.1 GB at the north-star size).  Lists in node order: node i owns the next degree[i] entries of
 * dst[] / offset[] (each list sorted by (dst, offset), as in alga_edge form: src/DataStructures/Graph.cpp:367-387).  ALGA_ERR_UNSUPPORTED where an
 * out-degree or an offset does not fit a byte (reads longer than min_overlap + 255): take alga_prefsuf_build_host.  One host block, released by
 * alga_free_compact_edges; alga_adapter::fill_graph_compact turns it into Graph::V. */
typedef struct {
    int32_t         n_nodes;
    uint64_t        n_edges;
    const uint8_t  *degree;   /* n_nodes */
    const uint32_t *dst;      /* n_edges */
    const uint8_t  *offset;   /* n_edges */
} alga_compact_edges;
int         alga_prefsuf_build_host_compact(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, alga_compact_edges *out);
/* ... and any edge list on the device (a build's result, the supplement's) brought down in that form: what alga_download_edges is to alga_edge triples */
int         alga_download_edges_compact(alga_engine *e, int32_t n_nodes, const alga_edge *d_edges, uint64_t n_edges, alga_compact_edges *out);
void        alga_free_compact_edges(alga_engine *e, alga_compact_edges *c);

/* Pinned host memory (hipHostMalloc): node arrays allocated here are read by the DMA engines as they are -- alga_prefsuf_build_host* and
 * alga_upload_*nodes then skip the copy through the engine's staging buffers (the pointer is recognised, nothing else changes).  Allocation is slow
 * (pages are mapped and locked): ask once, while the reads are still being parsed.  NULL on failure (alga_last_error). */
void       *alga_host_alloc(alga_engine *e, size_t bytes);
void        alga_host_free(alga_engine *e, void *p);

/* Allocates, ahead of time, every device buffer a build of the exact path needs for a node set of `n_nodes` rows of up to
 * `max_len` nucleotides (and, n_edges_hint > 0, for that many edges; 0 = one per node), and runs a miniature build of the same shape
 * (4096 random reads) so that the HIP runtime loads the kernels' code objects now: an assembler builds its graph ONCE, and what the
 * first build of a process pays on top of a warm one is mostly that loading (~20 ms; the allocations themselves ~1 ms at 90 M nodes).
 * Safe to call from a second host thread while the caller is still parsing or uploading the reads -- but not concurrently with
 * another call on the same engine.  Later builds allocate only what turns out larger. */
int  alga_engine_reserve(alga_engine *e, int32_t n_nodes, int32_t max_len, int32_t min_overlap, uint64_t n_edges_hint);

/* The two halves of alga_prefsuf_build_host for callers that keep the node set resident across several stages (exact graph ->
 * supplement -> ... on ONE upload): host node set -> the engine's upload buffers in the engine's row layout, `*dev` describes the
 * resident copy (valid until the next upload on this engine); device edge list -> engine-owned host list (alga_free_edges). */
int  alga_upload_nodes(alga_engine *e, const alga_nodes *nodes, alga_nodes *dev);
/* the same for a node set in ALGA's twin layout, given by the rows of its ODD nodes alone (alga_prefsuf_params.twin_rows): half the upload */
int  alga_upload_twin_nodes(alga_engine *e, const alga_nodes *nodes /* words: n / 2 rows */, alga_nodes *dev);
int  alga_download_edges(alga_engine *e, const alga_edge *d_edges, uint64_t n_edges, alga_edge **edges);

/* Same computation with the node set already resident in HBM (all pointers in `nodes` are device
 * pointers on the engine's device).  Work is enqueued on `hip_stream` (a hipStream_t).  NULL = the engine's own stream, a
 * NON-BLOCKING stream that orders with no other stream (not even the null stream): with NULL every input must be complete
 * before the call (synchronise the producing stream first); to chain behind work of another stream pass that stream.
 * The same holds for every call below that takes a `hip_stream`.  The edge list stays on the device:
 *   *d_edges : device pointer to alga_edge[*n_edges], owned by the engine, valid until the next
 *              build call on this engine or alga_engine_destroy(). */
int  alga_prefsuf_build_device(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p,
                               void *hip_stream, const alga_edge **d_edges, uint64_t *n_edges);

/* Copies `bytes` of engine-owned device memory (an edge list, a device node set) into host memory: for callers that
 * are plain C/C++ without the HIP headers. */
int  alga_copy_to_host(alga_engine *e, void *dst, const void *d_src, size_t bytes);

/* Plain device buffers for callers without the HIP headers (e.g. alignFrom / alignTo masks next to a device-resident node set). */
int  alga_device_alloc(alga_engine *e, size_t bytes, void **d_out);
void alga_device_free(alga_engine *e, void *d_ptr);
int  alga_copy_to_device(alga_engine *e, void *d_dst, const void *src, size_t bytes);

/* Counters and per-phase device times of the last build call on `e`. */
int  alga_prefsuf_last_stats(const alga_engine *e, alga_prefsuf_stats *out);

/* ---- sharded form (one process per GPU; the exchange between the two calls is the caller's) ----
 * Phase 1, on every rank: discover the overlaps whose SOURCE node id is in [src_begin, src_end)
 * against the full (replicated) node set, apply the per-source small-overlap cap (it is per source,
 * so it needs no exchange: GraphCreatorPrefSuf.cpp:397-401), and return the overlap records as two
 * device arrays of *n_records slots (engine-owned, valid until the next call on `e`):
 *   d_dst[i] : target node id, or 0xFFFFFFFF for an unused slot (skip it)
 *   d_val[i] : (ol << 32) | source node id,  ol = offset | (overlap_len << 22) | (small << 31)
 * Phase 2, on the rank that owns the target ids [dst_begin, dst_end): reduce records (any order,
 * every record of an owned target present) to edges.  Slots with d_dst outside the range are ignored. */
int  alga_prefsuf_discover_device(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p,
                                  int32_t src_begin, int32_t src_end, void *hip_stream,
                                  const uint32_t **d_dst, const uint64_t **d_val, uint64_t *n_records);
int  alga_prefsuf_reduce_device(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p,
                                const uint32_t *d_dst, const uint64_t *d_val, uint64_t n_records,
                                int32_t dst_begin, int32_t dst_end, void *hip_stream,
                                const alga_edge **d_edges, uint64_t *n_edges);

/* Sharded form without an exchange: the final edges whose SOURCE node id is in [src_begin, src_end), by the source-side
 * reduction (every rank holds the full node set; a source's edges depend on nothing another rank computes).  Returns
 * ALGA_ERR_UNSUPPORTED when that form is not exact for the input (see alga_reduction) -- every rank gets the same answer
 * for the same node set, except for the capacity case (more than 65 536 sources with over 160 raw overlaps each, or one with
 * over 4 096: repeat-rich input), so ranks agree on the
 * fallback with one flag all-reduce.  *d_edges: engine-owned, sorted by (src, dst), valid until the next call on `e`. */
int  alga_prefsuf_build_range_device(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p,
                                     int32_t src_begin, int32_t src_end, void *hip_stream,
                                     const alga_edge **d_edges, uint64_t *n_edges);

/* Sharding of the build step itself (CLUSTER probe).  Without it every rank computes the minimizer keys of ALL nodes before it
 * probes its own sources -- the part of a build that does not shrink with the rank count.  With it, rank r
 *   1. alga_prefsuf_keys_device(node range of r)   keys + runs of its own nodes (the nodes whose sources it will probe);
 *   2. all-gathers, IN PLACE, the two per-node arrays the call returns (uint32 d_keys[n], d_meta[n]: rank q's slice is
 *      [node_begin_q, node_end_q)) -- 8 bytes per node over RCCL;
 *   3. alga_prefsuf_build_range_device(params.keys_shared = 1, src range inside its node range): sorts the gathered keys into
 *      the bucket order, builds the entry array and probes.
 *   A rank may cut step 3 into pieces (first piece keys_shared = 1, the following ones keys_shared = 2 on consecutive source
 *   sub-ranges) so that the transfer of one piece's edges overlaps the probe of the next.
 *   Up to four ranks the drivers (engine_multi.hip, alga_amd.multigpu) skip steps 1-2: every rank's build (keys_shared = 0, its id range) computes
 *   the target keys of all nodes itself -- the key pass of a build the PILE path keeps makes no run lists, 1.5 ms at the north-star size -- and
 *   probes its range through the piles; the shared key pass pays from five ranks on.
 * out->eligible == 0: the CLUSTER probe does not take this input (every rank gets the same answer for the same node set and
 * options); skip steps 2-3's flag and call the build as before.  The arrays are engine-owned, valid until the next build, and
 * have room for n + ALGA_KEY_ARRAY_SLACK entries, so that equal-sized slices (ceil(n / ranks), the last one running past n) can be
 * gathered in place. */
#define ALGA_KEY_ARRAY_SLACK 1024
typedef struct { uint32_t *d_keys; uint32_t *d_meta; int32_t n; int32_t eligible;
                 int32_t meta_needed; /* 0: every live node has the same length and there is no alignFrom mask -- the build does not read d_meta, it need not be shared */
                 int32_t reserved; } alga_node_keys;
int  alga_prefsuf_keys_device(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p,
                              int32_t node_begin, int32_t node_end, void *hip_stream, alga_node_keys *out);

/* ---- sharded form with the INDEX sharded by seed bucket (alga_amd/csrc/prefsuf_shard.hip, engine_shard.hip) --------------------
 * The reference's one bucket table per overlap length (src/GraphCreators/GraphCreatorPrefSuf.cpp:247-280,317-332: every thread reads every
 * bucket) divided over N ranks: rank g owns the targets whose minimizer bucket lies in its 1 / N of the bucket space, builds THEIR
 * entries and directory only, receives the run descriptors (12 bytes: cluster key, source id, minimizer position and window range)
 * of every rank's sources that fall into its buckets, and decides the transitive reduction per TARGET from the target's complete
 * candidate list (tests/bucket_side_rule.py: the reference's per-target rule, GraphCreatorPrefSuf.cpp:403-483).  The per-source cap
 * of three small overlaps (:397-401) is the one decision that needs a source's other overlaps: surviving small overlaps are PENDING
 * until the top-3 small keys of their sources have been collected from the bucket owners.  Per build, on every rank r of N:
 *   1. alga_prefsuf_keys_device(own node range [b_r, b_r+1))          keys + runs of the rank's nodes
 *   2. all-gather, in place, of the key array (and meta if meta_needed) -- as for the replicated form above
 *   3. alga_shard_index_device       my slice of the entry array + directory; the descriptors of MY sources, grouped by owner rank
 *   4. all-to-all of the descriptors (12-byte records; counts / offsets per destination from step 3)
 *   5. alga_shard_join_device        verification + per-target reduction in my buckets; the sources of my pending edges
 *   6. all-gather of the pending source ids (u32, variable length)
 *   7. alga_shard_small_keys_device  {source, L, C} (3 x u32) of the small overlaps my descriptors of those sources saw (top 3 per run)
 *   8. all-gather of those lists
 *   9. alga_shard_resolve_device     pending edges that fail their source's cap are dropped; final edges grouped by the rank that owns
 *                                    the SOURCE id (ranges of alga_amd/multigpu.py: shard_chunk -- the same as for the key all-gather)
 *  10. all-to-all of the edges (12-byte alga_edge)
 *  11. alga_shard_place_device       adjacency lists of my source range, (src, dst)-ordered: ready for the gather to rank 0
 * A call answers ALGA_ERR_UNSUPPORTED when the form does not take the input (what the clustered probe declines; a bucket with more than
 * 4096 descriptors): all ranks then take the replicated form.  Every result is engine-owned and valid until the next shard call. */
typedef struct {
    uint64_t targets_owned, descriptors_out, descriptors_in, flagged_sources;   /* index phase / join phase                          */
    uint64_t records, pending, pending_sources, small_keys_out, small_keys_in, dropped;
    uint64_t edges_out, edges_in, edges;
    uint64_t join_passes, join_passes_serial;   /* wave passes of k_shard_join (whole buckets packed onto 64 lanes); those decided target by target */
    double   ms_index, ms_export, ms_sort, ms_join, ms_cap, ms_edges_out, ms_place;   /* device time of each phase (HIP events)  */
} alga_shard_stats;
/* desc_counts[q] descriptors for rank q start at descriptor desc_offsets[q] of *d_desc (3 x uint32 each) */
int  alga_shard_index_device(alga_engine *e, const alga_nodes *nodes, const alga_prefsuf_params *p, int32_t rank, int32_t n_ranks, void *hip_stream,
                             const uint32_t **d_desc, uint64_t *desc_counts /* n_ranks */, uint64_t *desc_offsets /* n_ranks */);
int  alga_shard_join_device(alga_engine *e, const alga_nodes *nodes, const uint32_t *d_desc_in, uint64_t n_desc, void *hip_stream,
                            const uint32_t **d_pending_src, uint64_t *n_pending_src);
int  alga_shard_small_keys_device(alga_engine *e, const uint32_t *d_pending_src_all, uint64_t n_all, void *hip_stream,
                                  const uint32_t **d_small /* 3 x uint32: source, L, C */, uint64_t *n_small);
int  alga_shard_resolve_device(alga_engine *e, const uint32_t *d_small_all, uint64_t n_small_all, void *hip_stream,
                               const alga_edge **d_edges_out, uint64_t *edge_counts /* n_ranks */, uint64_t *edge_offsets /* n_ranks */);
int  alga_shard_place_device(alga_engine *e, const alga_edge *d_edges_in, uint64_t n_in, int32_t src_begin, int32_t src_end, void *hip_stream,
                             const alga_edge **d_edges, uint64_t *n_edges);
int  alga_shard_last_stats(const alga_engine *e, alga_shard_stats *out);

/* ---- the N GPUs of one node behind one handle (alga_amd/csrc/engine_multi.hip) ------------------------------------
 * The reference's parallelism is --threads (src/Params.cpp:237-294; worker threads inside GraphCreatorPrefSuf,
 * src/GraphCreators/GraphCreatorPrefSuf.cpp:150-161); the counterpart: ONE process, one host thread and one engine per GPU.  Rank r
 * computes the minimizer keys of its node range, the key arrays are all-gathered in place (RCCL over xGMI), every rank builds the final
 * edges of its own sources (steps 1-3 above) and the lists are gathered on rank 0's GPU with their exact lengths (grouped
 * ncclSend / ncclRecv) -- the concatenation is the single-GPU byte order.  A rank declining the source-side form makes rank 0 build
 * the whole graph alone: the result never depends on the number of ranks.
 * transport: RCCL (dlopen of librccl.so.1; one GPU per rank) or COPY (hipMemcpyPeerAsync + host barriers; also takes several ranks on
 * ONE device, which is how the driver is tested on a one-GPU box); AUTO = RCCL when every rank has its own GPU and there is more
 * than one, else COPY.  Not yet run on more than one GPU: in particular the variable-length exchanges of the
 * BUCKET_SHARDED form have only ever run over COPY and gloo, never over RCCL.  A post inside an RCCL group that fails on one rank aborts
 * every communicator of the handle (ncclCommAbort: the peers' matching halves would otherwise wait for ever), the build returns an
 * error on all ranks, and the handle refuses further RCCL collectives: destroy it and create a new one. */
typedef struct alga_multi alga_multi; /* opaque */
typedef enum { ALGA_TRANSPORT_AUTO = 0, ALGA_TRANSPORT_RCCL = 1, ALGA_TRANSPORT_COPY = 2 } alga_transport;
/* How the N ranks divide a build (alga_multi_set_option "form"; same graph either way):
 *   REPLICATED      every rank builds the whole bucket-ordered entry array from the all-gathered keys and probes its own source ids
 *                   (round 3: nothing but keys and edges travels, but the index build does not shrink with N);
 *   BUCKET_SHARDED  the index itself is sharded by seed bucket (alga_shard_* above): 1 / N of the entry array per rank, run descriptors
 *                   travel to the bucket's owner, the reduction is decided per target there, edges return to the source's owner;
 *   AUTO            = REPLICATED: measured per rank on one GPU at the north-star size (tools/emulate_shard.py, tools/emulate_rank.py), the
 *                   sharded form costs a rank more device time than the replicated one up to eight ranks.
 *   A build the sharded form declines (ALGA_ERR_UNSUPPORTED on any rank) continues in the replicated form. */
typedef enum { ALGA_MULTI_FORM_AUTO = 0, ALGA_MULTI_FORM_REPLICATED = 1, ALGA_MULTI_FORM_BUCKET_SHARDED = 2 } alga_multi_form;
typedef struct {
    int32_t  n_ranks, transport;          /* alga_transport actually used                                        */
    int32_t  fell_back_to_one_gpu;        /* a rank declined the source-side form: rank 0 built the whole graph  */
    int32_t  form;                        /* alga_multi_form the last build ended in (1 or 2)                     */
    uint64_t edges;
    double   ms_upload, ms_download;      /* host entry point only: node set to every GPU (side by side), edges from the GPUs */
    double   ms_keys, ms_share, ms_build, ms_gather, ms_total;   /* rank 0's host clock: key pass of its nodes, key all-gather, build of its
                                             sources (waits for the slowest rank at its end), gather of the edge lists, all of it */
    /* what rank 0 SENT to other ranks in each exchange of the last build, bytes (the all-gathers: its own slice times N - 1) */
    uint64_t xbytes_keys, xbytes_descriptors, xbytes_pending, xbytes_small_keys, xbytes_edges, xbytes_gather;
    double   ms_shard_index, ms_shard_exchange, ms_shard_join, ms_shard_cap, ms_shard_place;   /* BUCKET_SHARDED, rank 0's host clock per phase */
} alga_multi_stats;
/* "form": alga_multi_form */
int         alga_multi_set_option(alga_multi *m, const char *name, int64_t value);
int         alga_multi_create(const int32_t *hip_devices, int32_t n_ranks, int32_t transport, alga_multi **out);
void        alga_multi_destroy(alga_multi *m);
const char *alga_multi_last_error(const alga_multi *m);
alga_engine *alga_multi_engine(alga_multi *m, int32_t rank);   /* rank's engine: input stage (alga_ingest_device) before, further stages (supplement ...) after, on rank 0's */
/* nodes_per_rank[r]: the node set resident on rank r's GPU (the same nodes on every rank).  *d_edges: the complete graph on rank 0's
 * GPU, owned by the handle, valid until its next build. */
int         alga_multi_prefsuf_build_device(alga_multi *m, const alga_nodes *nodes_per_rank, const alga_prefsuf_params *p,
                                            const alga_edge **d_edges, uint64_t *n_edges);
/* Host buffers in, edges out -- alga_prefsuf_build_host on N GPUs; release *edges with alga_multi_free_edges before alga_multi_destroy. */
int         alga_multi_prefsuf_build_host(alga_multi *m, const alga_nodes *nodes, const alga_prefsuf_params *p, alga_edge **edges, uint64_t *n_edges);
void        alga_multi_free_edges(alga_multi *m, alga_edge *edges);
int         alga_multi_last_stats(const alga_multi *m, alga_multi_stats *out, alga_prefsuf_stats *per_rank /* n_ranks entries, or NULL */);

/* Exchange helpers of the sharded form (device in, device out, engine-owned results):
 *   alga_sort_records_device  orders record slots by target id and drops the padding: the first *n_valid
 *                             entries of the outputs are the records, so the slice that belongs to the rank
 *                             owning targets [a, b) is contiguous (lower_bound of a and b in d_dst_sorted).
 *   alga_sort_edges_device    orders a gathered edge list by (src, dst): the byte order of the single-GPU result. */
int  alga_sort_records_device(alga_engine *e, const uint32_t *d_dst, const uint64_t *d_val, uint64_t n_records,
                              int32_t n_nodes, void *hip_stream, const uint32_t **d_dst_sorted,
                              const uint64_t **d_val_sorted, uint64_t *n_valid);
/* The (u32 key, u32 value) sort of the index build on its own (tests and tools): stable on the key bits [begin_bit, 32).  own != 0: the
 * engine's radix sort (alga_amd/csrc/radix_sort.hip), 0: rocPRIM's.  For n < 2^22 the library path sorts on all 32 bits (its merge-sort path
 * compares the wrong bits for a partial key); the engine's own sort looks at [begin_bit, 32) whatever n is.  The sorted arrays are engine-owned
 * (valid until the next call on e); *ms_best = the fastest of `repeat` runs by HIP events.  d_vals == NULL with own != 0: the values are the
 * positions 0, 1, 2, ... (how the index build, the final-contig filter and the supplement call the sort); with own == 0 a NULL value array is
 * ALGA_ERR_INVALID_ARGUMENT (rocPRIM needs values). */
int  alga_sort_u32_pairs_device(alga_engine *e, const uint32_t *d_keys, const uint32_t *d_vals, uint64_t n, int32_t begin_bit, int32_t own, int32_t repeat,
                                void *hip_stream, const uint32_t **d_keys_sorted, const uint32_t **d_vals_sorted, double *ms_best);
/* The (u64 key, u64 value) sort of the supplement's k-mer entries on its own (tests and tools): stable on the key bits [0, bits); own != 0: the
 * engine's radix sort (bits <= 50), 0: rocPRIM's.  Replaces the std::sort of the reference's k-mer buckets (src/GraphCreators/GraphCreatorKmerBased.cpp:94-106). */
int  alga_sort_u64_pairs_device(alga_engine *e, const uint64_t *d_keys, const uint64_t *d_vals, uint64_t n, int32_t bits, int32_t own, int32_t repeat,
                                void *hip_stream, const uint64_t **d_keys_sorted, const uint64_t **d_vals_sorted, double *ms_best);
/* The (u32 key, u64 value) sort of the bucket-sharded build's run descriptors on its own (tests and tools): stable on the key bits
 * [begin_bit, end_bit); a window that is not one (begin_bit < 0, end_bit > 32, end_bit <= begin_bit) is [0, 32).  own != 0: the engine's radix sort
 * (12-byte records, alga_amd/csrc/radix_sort.hip), 0: rocPRIM's, which for n < 2^22 sorts on all 32 bits (see alga_sort_u32_pairs_device).  The
 * inputs are left untouched; the sorted arrays are engine-owned (valid until the next call on e). */
int  alga_sort_desc_device(alga_engine *e, const uint32_t *d_keys, const uint64_t *d_vals, uint64_t n, int32_t begin_bit, int32_t end_bit, int32_t own,
                           int32_t repeat, void *hip_stream, const uint32_t **d_keys_sorted, const uint64_t **d_vals_sorted, double *ms_best);
int  alga_sort_edges_device(alga_engine *e, const alga_edge *d_edges, uint64_t n_edges, int32_t n_nodes,
                            void *hip_stream, const alga_edge **d_sorted);

/* ---- approximate supplement (error_rate > 0.01): GraphCreatorLI ---------------------------------
 * Replaces, for the caller at src/main.cpp:300-347,
 *   new GraphCreatorLI(READS, G); setAlignFrom/To from the degrees of G; startAlignmentGraphCreation();
 *   G->retainOnlySmallestOffset();
 * i.e. four rounds (rotated alphabet priorities, src/GraphCreators/GraphCreatorLI.cpp:18-28) of: LI minimizer
 * k-mers of the tip nodes (src/DataStructures/Read.cpp:145-226), groups of equal k-mer
 * (src/GraphCreators/GraphCreatorKmerBased.cpp:28-136), pairwise join with branch markers
 * (src/GraphCreators/GraphCreatorPairwiseKmerBranch.cpp:16-97) and the mismatch-budget check
 * AlignmentControllerHybrid::canAlign (src/AlignmentControllers/AlignmentControllerLowErrorRate.cpp:15-49).
 * Order dependence: the reference walks the groups of a round one after the other (and races between its threads when
 * --threads > 1) and leaves the order of equal k-mers to std::sort; the engine gives every group the graph as it was
 * when the round started and orders equal k-mers by node id.  DESIGN.md states the measured difference. */
typedef struct {
    int32_t min_overlap_area;   /* Params::MIN_OVERLAP_AREA        = int((1 + SCALE) * avg_len / 2)   (src/main.cpp:333) */
    int32_t max_offset_pct;     /* Params::MAX_OFFSET_CONSIDERED_FOR_ALIGNMENT = int((1 - SCALE) * avg_len / 2), %      */
    int32_t min_identity_pct;   /* Params::MINIMAL_OVERLAP_FOR_LCS_LOW_ERROR = 99 - int(100 * error_rate)             */
    int32_t same_ends;          /* Params::ALIGNMENT_CONTROLLER_SAME_ENDS_LENGTH, 3                                    */
    int32_t li_k;               /* Params::LI_KMER_LENGTH, 35 (src/main.cpp:340)                                       */
    int32_t li_intervals;       /* Params::LI_KMER_INTERVALS, 6 (src/main.cpp:339)                                     */
    int32_t rounds;             /* min(4, Params::LI_PRIORITIES_TO_CONSIDER) = 4                                       */
    int32_t kmer_length_bucket; /* Params::KMER_LENGTH_BUCKET = min(2L/3, 60): shorter reads give no k-mers            */
} alga_pkb_params;

typedef struct {
    uint64_t kmers[4];          /* k-mers per round                                                                    */
    uint64_t groups[4];         /* groups of >= 2 equal k-mers per round                                               */
    uint64_t can_align_calls[4];
    uint64_t edges_after[4];    /* edges in the graph after each round                                                 */
    uint64_t max_group;
    double   ms_total;
    uint64_t group_hist[4][8];  /* per round, groups of 2, 3, 4, 5-7, 8-15, 16-31, 32-64 and > 64 equal k-mers (this rank's)     */
} alga_pkb_stats;

/* (1 + SCALE) / (1 - SCALE) arithmetic of src/main.cpp:332-336 in float, truncating; error_rate as on the command line */
void alga_pkb_derive_params(double avg_len, float scale, double error_rate, int32_t kmer_length_bucket, alga_pkb_params *p);

/* canAlign on n (r1, r2, offset) int32 triples -> n bytes (host buffers in and out) */
int  alga_can_align_batch_host(alga_engine *e, const alga_nodes *nodes, const alga_pkb_params *p, const int32_t *triples,
                               uint64_t n, uint8_t *out);
/* LI k-mers of every node under the alphabet permutation prio[4]: hash[n*li_intervals], ind[n*li_intervals], count[n] */
int  alga_li_kmers_host(alga_engine *e, const alga_nodes *nodes, const alga_pkb_params *p, const int32_t prio[4],
                        uint64_t *hash, int32_t *ind, int32_t *count);
/* The supplement: edges_in = the graph of the exact path (sorted by (src, dst), one edge per pair), result in the same
 * form; host buffers (`nodes` as for alga_prefsuf_build_host).  Release *edges_out with alga_free_edges(). */
int  alga_pkb_supplement_host(alga_engine *e, const alga_nodes *nodes, const alga_pkb_params *p, const alga_edge *edges_in,
                              uint64_t n_edges_in, alga_edge **edges_out, uint64_t *n_edges_out);
/* Same with node set and edge list resident in HBM; the result stays on the device (engine-owned). */
int  alga_pkb_supplement_device(alga_engine *e, const alga_nodes *nodes, const alga_pkb_params *p, const alga_edge *d_edges_in,
                                uint64_t n_edges_in, void *hip_stream, const alga_edge **d_edges_out, uint64_t *n_edges_out);
int  alga_pkb_last_stats(const alga_engine *e, alga_pkb_stats *out);

/* The supplement on N ranks (one engine per GPU; SURVEY.md section 8(e): groups are keyed by k-mer hash, the reference spreads its k-mer buckets
 * over worker threads, src/GraphCreators/GraphCreatorKmerBased.cpp:108-136).  Every rank holds the node set and the COMPLETE exact graph; a group of
 * equal k-mers belongs to rank mix(k-mer key) mod n_ranks.  Per round (params->rounds of them) each rank joins its own groups against the graph as
 * it stood when the round began -> its additions (edge keys src << 36 | dst << 9 | offset, unsorted, engine-owned until the merge); the CALLER
 * brings the additions of all ranks together on every rank (an all-gather of variable length: RCCL, torch.distributed, peer copies) and every rank
 * merges them ALL: the graphs stay identical, and identical to the one-GPU supplement's -- every group of a round sees the round's start graph and
 * the merge orders by key, so nothing depends on how the groups were dealt out (tests/test_gpu_pkb.py: 2, 3 and 5 ranks on one GPU).
 *   begin -> { round -> [exchange] -> merge } x rounds -> end.   alga_pkb_supplement_device is exactly this with one rank.
 * k-mers and their sort are computed by every rank (the pairwise join and canAlign are what is shared out). */
int  alga_pkb_shard_begin(alga_engine *e, const alga_nodes *nodes, const alga_pkb_params *p, const alga_edge *d_edges_in, uint64_t n_edges_in, int32_t rank,
                          int32_t n_ranks, void *hip_stream);
int  alga_pkb_shard_round(alga_engine *e, void *hip_stream, const uint64_t **d_additions, uint64_t *n_additions);
int  alga_pkb_shard_merge(alga_engine *e, const uint64_t *d_all_additions, uint64_t n_all, void *hip_stream);
int  alga_pkb_shard_end(alga_engine *e, void *hip_stream, const alga_edge **d_edges_out, uint64_t *n_edges_out);
/* The approximate supplement (alga_pkb_shard_*) on the handle's N ranks: d_edges_rank0 = the exact graph on rank 0's GPU (what
 * alga_multi_prefsuf_build_device returned); it is sent to every rank, each round's additions are all-gathered over the handle's transport, and
 * rank 0's copy of the result -- identical on all ranks, and to the one-GPU supplement's -- is handed back (engine-owned, rank 0's GPU). */
int         alga_multi_pkb_supplement_device(alga_multi *m, const alga_nodes *nodes_per_rank, const alga_pkb_params *p, const alga_edge *d_edges_rank0,
                                             uint64_t n_edges, const alga_edge **d_edges_out, uint64_t *n_edges_out);

/* ---- input stages (host, multithreaded C++; no GPU involved) ---------------------------------
 * What the reference does between its command line and the GraphCreator constructor, in its
 * --threads=1 order: record parsing, end trimming, N / STR filters, 2-bit packing, reverse-complement
 * twins, pair interleave (src/IO/InputReader.cpp:44-139,272-391), parameter derivation
 * (src/main.cpp:93-115), duplicate / prefix read removal (src/IO/ReadPreprocess.cpp:13-152), id
 * compaction and removal of too-short reads (src/main.cpp:150-232,253-266). */
typedef struct {
    int32_t trim_left, trim_right;   /* Params::READ_END_TRIM_LEFT/RIGHT, default 3 / 3           */
    int32_t remove_reads_with_n;     /* default 1                                                  */
    int32_t rna;                     /* default 0                                                  */
    float   scale;                   /* Params::SCALE, default 0.55                                */
    int32_t min_overlap;             /* -l ; -1 = derive from the mean read length                 */
    int32_t rsoemo;                  /* --rsoemo ; -1 = derive                                     */
    int32_t remove_pref_reads;       /* 1 duplicates, 2 all prefix reads (default), 3 none         */
    int32_t threads;
} alga_ingest_params;

typedef struct {
    int32_t   n, stride_words;       /* stride_words is a multiple of 4 (16-byte aligned rows)     */
    uint32_t *words;                 /* n * stride_words                                           */
    int32_t  *len;                   /* 0 = removed node                                           */
    uint8_t  *pair_off;              /* Global::pairedReadOffset                                   */
    int32_t   LEN, min_overlap, rsoemo, li_kmer_length;
    int64_t   records;
    int32_t   removed_n, removed_str, removed_prefix, removed_short;
    double    avg_len;
} alga_node_set;

void alga_ingest_default_params(alga_ingest_params *p);
int  alga_ingest_files(const char *file1, const char *file2 /* may be NULL */, const alga_ingest_params *p,
                       alga_node_set *out, char *errbuf, size_t errlen);
void alga_free_node_set(alga_node_set *ns);

/* Stage 1 alone: files -> every record's two nodes in the reference's node order, before the removals that depend on other
 * reads (src/IO/InputReader.cpp:44-139,272-391, parameters of src/main.cpp:93-115).  Release with alga_free_parsed_reads. */
typedef struct {
    int64_t   n_nodes;               /* 2 x records                                                                     */
    int32_t   stride_words;
    uint32_t *rows;                  /* n_nodes x stride_words, node 2k = reverse complement, 2k+1 = forward of read k  */
    int32_t  *len;                   /* -1 = removed (N / STR)                                                          */
    int32_t   paired;
    int64_t   records;
    int32_t   removed_n, removed_str;
    int32_t   LEN, min_overlap, rsoemo, li_kmer_length;
    double    avg_len;
    void     *owner;                 /* internal                                                                        */
} alga_parsed_reads;

int  alga_parse_files(const char *file1, const char *file2 /* may be NULL */, const alga_ingest_params *p,
                      alga_parsed_reads *out, char *errbuf, size_t errlen);
void alga_free_parsed_reads(alga_parsed_reads *pr);

/* ---- duplicate / prefix-read removal and id compaction on the GPU ----------------------------
 * The stage between the parser and the GraphCreator constructor (src/IO/ReadPreprocess.cpp:13-152, src/main.cpp:150-232,
 * 253-266): every record's two nodes in the reference's node order come in from the host (as alga_amd/host/ingest.cpp
 * `parse` leaves them; len -1 = removed by the N / STR filters), the surviving node set stays on the device, ready for
 * alga_prefsuf_build_device.  Same result as the host statement of the stage behind alga_ingest_files. */
typedef struct {
    const uint32_t *rows;            /* host: n_nodes rows of stride_words uint32, zero padded, node 2k = reverse complement,
                                        2k+1 = forward strand of read k                                               */
    int32_t         stride_words;
    const int32_t  *len;             /* host: n_nodes lengths, -1 = removed                                             */
    int64_t         n_nodes;         /* even                                                                            */
    int32_t         remove_pref_reads; /* 1 duplicates, 2 all prefix reads (the reference's default), 3 none           */
    int32_t         min_keep_len;    /* nodes shorter than this are emptied (len 0): 3 + li_kmer_length                */
} alga_preprocess_input;

typedef struct {
    const uint32_t *d_words;         /* device, engine-owned until the next alga_preprocess_nodes call on the engine   */
    const int32_t  *d_len;
    const uint8_t  *d_pair_off;      /* Global::pairedReadOffset                                                        */
    int32_t         n, stride_words;
    int32_t         removed_prefix, removed_short, max_len;
    double          ms_device;       /* upload excluded: sort + mark + compaction                                       */
} alga_device_node_set;

int  alga_preprocess_nodes(alga_engine *e, const alga_preprocess_input *in, alga_device_node_set *out);

/* ---- the whole input stage on the GPU -----------------------------------------------------------
 * Files -> node set resident in HBM.  The host maps the files and moves their bytes; everything InputReader does per record
 * (src/IO/InputReader.cpp:142-180,272-391: sequence line, blanks, end trimming, letter check, N / STR filters, 2-bit packing,
 * reverse complement, [rc, r] node order, pair interleave) and the stage behind alga_preprocess_nodes run as HIP kernels.
 * Takes .fasta (two lines per record) and .fastq / .fq (four) with remove_reads_with_n = 1, the reference's default; anything
 * else answers ALGA_ERR_UNSUPPORTED (use alga_parse_files + alga_preprocess_nodes).  Same node set as alga_ingest_files. */
typedef struct {
    int64_t records;                 /* records read (both files)                                                       */
    int32_t removed_n, removed_str;  /* nodes removed by the N / STR filters                                             */
    int32_t LEN, min_overlap, rsoemo, li_kmer_length;   /* src/main.cpp:93-115                                          */
    int32_t paired;
    double  avg_len;
    double  ms_parse, ms_preprocess; /* wall: map + upload + parse kernels; duplicate / prefix removal + compaction     */
    double  ms_upload;               /* part of ms_parse: device buffer + file bytes to HBM                             */
} alga_ingest_info;

int  alga_ingest_device(alga_engine *e, const char *file1, const char *file2 /* may be NULL */, const alga_ingest_params *p,
                        alga_device_node_set *out, alga_ingest_info *info);

/* ---- first step of the graph simplifier ---------------------------------------------------------
 * What the caller does first with the graph on the PrefSuf path (GraphSimplifier::simplifyGraphOld,
 * src/GraphSimplifiers/GraphSimplifier.cpp:90-125): Graph::sortEdgesByIncreasingOffset (src/DataStructures/Graph.cpp:584-614) and
 * GraphSimplifier::cutNonAndWeaklyMetricTriangles (src/GraphSimplifiers/GraphSimplifier.cpp:228-348): an edge i -> b of weight
 * w <= max_offset_parallel_paths (Params::MAX_OFFSET_PARALLEL_PATHS = max(250, int(1.75 * LEN)), src/main.cpp:95) goes when the
 * shortest two-edge path i -> a -> b weighs exactly w.  In: edges grouped by src, lists sorted by (dst, offset) -- what the
 * builds above return.  Out: grouped by src, every list in the order the reference leaves it in (sorted by (offset, dst), then
 * Graph::removeDirectedEdge's swap-with-last removals, src/DataStructures/Graph.cpp:96-119), so a Graph::V filled from it is the
 * reference's graph after that step, entry for entry.  *d_edges_out: engine-owned, valid until the next call of this function. */
int  alga_cut_triangles_device(alga_engine *e, int32_t n_nodes, const alga_edge *d_edges, uint64_t n_edges, int32_t max_offset_parallel_paths,
                               void *hip_stream, const alga_edge **d_edges_out, uint64_t *n_edges_out, uint64_t *n_removed /* may be NULL */);
int  alga_cut_triangles_host(alga_engine *e, int32_t n_nodes, const alga_edge *edges, uint64_t n_edges, int32_t max_offset_parallel_paths,
                             alga_edge **edges_out, uint64_t *n_edges_out);     /* release with alga_free_edges() */

/* ---- short parallel paths: bubbles go between the cut and the clip (alga_amd/csrc/mst_kernels.hip, mst_walk.h, engine_simplify.hip) ----------
 * GraphSimplifier::removeShortParallelPaths, i.e. tryToRemoveShortPathsMST for every node with >= 2 out-edges
 * (src/GraphSimplifiers/GraphSimplifier.cpp:182, :351-518); tests/tips_checker.py restates it in Python (remove_short_parallel_paths, held to the
 * reference's own dumps at --threads=1) and the device result equals that, entry for entry.  A sequencing error in the middle of a read opens a
 * bubble: two paths between the same two nodes.  The step keeps, around every branching node, a tree of the lightest edges.
 * The pipeline on the device: build -> supplement -> cut -> PARALLEL PATHS -> clip -> unitigs -> GFA.
 *   In: `d_edges` grouped by src with src ascending, device memory, every list in the order alga_cut_triangles_device leaves it in: list order
 *   matters.  Ids outside [0, n_nodes), a negative offset or a src smaller than the one before it: ALGA_ERR_INVALID_ARGUMENT, checked on the
 *   device, nothing written, the previous result untouched.
 *   One beg: the nodes beg = 0, 1, ..., n - 1 in ascending order, each on the graph the earlier ones left; a node that has >= 2 out-edges at
 *   that moment does this:
 *     1. a queue neigh = [beg] is processed in order, dst[beg] = 0;
 *     2. a node a taken from the queue is expanded only if it has not been expanded before and dst[a] <= max_offset;
 *     3. expansion walks a's list in list order; an entry (b, o) is skipped if dst[b] is set and dst[b] < dst[a] + o; otherwise
 *        dst[b] = dst[a] + o, (a, b, o) is appended to `edges` and b to the queue;
 *     4. for every collected edge in collection order Graph::removeDirectedEdge(a, b): every entry a -> b goes, each swapped with the
 *        shrinking last position;
 *     5. `edges` is sorted by (o, a, b);
 *     6. in that order an edge is pushed to the back of a's list unless an edge into b has been pushed already for this beg.
 *   Out: grouped by src, every list in exactly the resulting order (a Graph::V filled from it is the reference's graph after the step, entry for
 *   entry); engine-owned device memory, valid until the next call of this function.  It can hold several edges per (src, dst): the clip
 *   applies Graph::retainOnlySmallestOffset itself.
 * `max_offset`: the reference passes int(double(MAX_OFFSET_PARALLEL_PATHS * AVG_READ_LENGTH) / 100.0f) (:182), AVG_READ_LENGTH as for the clip.
 * The schedule.  A beg reads and writes only the lists of the nodes it expands, and an expanded node has a path of weight <= max_offset from
 * beg in the graph of that moment.  The step only removes edges (what it pushes back is part of what it took out), so whenever beg runs, what
 * it expands lies in its ball B(beg): the nodes at shortest-path distance <= max_offset from beg in any EARLIER state of the graph.  Two begs
 * with disjoint balls commute.  Rounds: the nodes with >= 2 out-edges are pending (one whose degree has fallen below 2 is dropped: a degree
 * never rises); every pending beg computes its ball on the current graph and claims each node of it with the minimum of the claiming ids; a
 * beg that holds its whole ball wins -- no smaller pending id touches its ball, now or later -- and the winners run the literal step on the
 * live lists, in any order.  The smallest pending id always wins.  The host reads one pair of counts per round.  The result is the
 * sequential ascending-id run's, entry for entry (tests/mst_schedule.py states the schedule in Python; tests/test_mst_schedule_cpu.py).
 * The number of rounds is the longest chain of overlapping balls with ascending ids: tens of rounds when ids are in random order along the
 * genome (reads as a sequencer delivers them), proportional to the length of a contig when the reads are numbered in genome order.  That is a
 * property of the definition (a beg must see what every smaller id within its reach has left), not of this implementation; there is no cap
 * and no host fallback.  `rounds` reports it.  The ABI number stays 7: like the GFA, unitig and clip calls before it this one only adds to the ABI.
 * The walks: one wave per beg with the state in LDS (a map of 256 slots, 192 nodes, 256 collected edges); begs that need more (rows of hundreds of
 * edges, balls of several hundred nodes) take the overflow route with per-beg arrays in a device workspace: 1024 states of 4096 nodes and 8192
 * edges, and for what even those cannot hold states sized for the whole graph (as many as 1 GB holds, at least one).
 * Device memory of the engine for this call, kept until the engine goes: 24 bytes per edge and 28 per node for rows, lists and owner[]; 180 MB for
 * the first overflow tier; and for a graph that one of its states does not hold (more than 4096 nodes or 8192 edges) the second tier, allocated up
 * front because a round finds out on the device who needs it: one state is 8 * 2^ceil(log2(2 (n + 1))) + 4 (n + 1) + 12 (m + 1) bytes -- 1.1 GB for
 * 20 M nodes and 5.6 M edges, 16 GB of maps alone towards 2^30 nodes.  The states are filled once, not per call: a walk leaves its map empty. */
#define ALGA_MST_MAX_ROUNDS 64
typedef struct {
    uint64_t edges_in, edges_out;
    uint64_t branching_nodes;                    /* nodes with >= 2 out-edges in the input: the initially pending                  */
    uint64_t begs_run;                           /* nodes that ran the step (they still had >= 2 out-edges at their turn)          */
    uint64_t rounds;
    uint64_t winners[ALGA_MST_MAX_ROUNDS];       /* begs run per round (the first 64 rounds; begs_run counts all)                  */
    uint64_t overflow_begs;                      /* begs whose run took the overflow route                                         */
    uint64_t ball_max;                           /* nodes of the largest ball claimed                                              */
    double   ms_prepare, ms_rounds;              /* device time (HIP events): checks + rows + pending list; the rounds             */
    double   ms_total;                           /* wall time of the call                                                          */
} alga_mst_info;
int  alga_remove_short_parallel_paths_device(alga_engine *e, int32_t n_nodes, const alga_edge *d_edges, uint64_t n_edges, int32_t max_offset,
                                             void *hip_stream, const alga_edge **d_edges_out, uint64_t *n_edges_out, alga_mst_info *info /* may be NULL */);

/* ---- dangling-branch removal: tips are clipped before the unitigs (alga_amd/csrc/tip_kernels.hip, tip_walk.h, engine_simplify.hip) ----------
 * GraphSimplifier::removeDanglingBranches / removeDanglingUpperBranches as simplifyGraphOld iterates them
 * (src/GraphSimplifiers/GraphSimplifier.cpp:191-215, :577-820); tests/tips_checker.py restates it in Python and the device result equals that.
 * A read with a sequencing error near an end has an in-edge and no out-edge (its twin the other way round): every such tip turns a
 * non-branching path into a branch.  The pipeline on the device: build -> supplement -> cut -> CLIP -> unitigs -> GFA.
 *   In: `d_edges` in any order, device memory.  Ids outside [0, n_nodes) or a negative offset: ALGA_ERR_INVALID_ARGUMENT, checked on the
 *   device, nothing written.  First per (src, dst) the smallest offset is kept (Graph::retainOnlySmallestOffset, :191).
 *   One pass on a graph H whose lists are in ascending neighbour order: for every node `beg` with >= 2 out-edges, for each out-edge (v, o) in
 *   list order: par[v] = beg (an earlier par[v] is overwritten), v is marked, off = o; while v has exactly one out-edge (son, w): stop if son
 *   is marked for this beg, else mark it, par[son] = v, off += w, v = son, and stop after the step if off > max_offset.  If v now has no
 *   out-edge and off <= max_offset, (off, v) is an end.  If every out-edge of beg gave an end, the largest (off, v) is dropped.  From every
 *   other end up par[] to beg each edge (par[x], x) is to go.  Every beg reads the same unmodified H; the union goes afterwards.
 *   Iteration i = 0, 1, ...: a down pass on the graph, an up pass on its reverse; it goes on while an iteration removed something and
 *   stops early when i >= 15 and it removed <= 30 edges (:210-213).
 *   Out: the surviving edges sorted by (src, dst, offset), engine-owned device memory, valid until the next call of this function.
 * `max_offset`: the reference passes int(MAX_OFFSET_DANGLING_BRANCHES * AVG_READ_LENGTH / 100.0f) with MAX_OFFSET_DANGLING_BRANCHES =
 * max(250, int(1.75 * LEN)) and AVG_READ_LENGTH the integer mean length of the reads alive at that moment.
 * NOT reproduced: the reference removes the found edges through WorkloadManager::parallelBlockExecution(0, size - 1, 3 * threads, ...),
 * which leaves out the last element of its SHUFFLED removal list when (size - 1) % (3 * threads) == 0 and the only element when size == 1:
 * one randomly chosen edge then survives the pass and can steer later ones.  This function removes every edge a pass finds.
 * No host fallback: the walks run in k_tip_find (one thread per branching node, a short list in LDS), and the nodes whose list does not fit
 * (rows of hundreds of edges, zero-offset chains through many joins) in k_tip_find_overflow with per-node arrays on the device. */
#define ALGA_TIPS_MAX_PASSES 64
typedef struct {
    uint64_t edges_in, edges_unique, edges_out;  /* as given, one per (src, dst), surviving                                        */
    int32_t  iterations, passes;                 /* passes = 2 * iterations: down, up, down, up, ...                               */
    uint64_t removed[ALGA_TIPS_MAX_PASSES];      /* edges removed per pass (the first 64 passes; removed_total counts all)         */
    uint64_t removed_total;
    uint64_t branching_nodes, overflow_nodes;    /* summed over the passes: nodes walked from, those that took the overflow route   */
    double   ms_prepare, ms_passes;              /* device time (HIP events): checks + sorts + both CSR directions; the loop        */
    double   ms_total;                           /* wall time of the call                                                           */
} alga_tips_info;
int  alga_remove_dangling_branches_device(alga_engine *e, int32_t n_nodes, const alga_edge *d_edges, uint64_t n_edges, int32_t max_offset,
                                          void *hip_stream, const alga_edge **d_edges_out, uint64_t *n_edges_out, alga_tips_info *info /* may be NULL */);

/* ---- contig trimming: the second use of the PrefSuf creator ---------------------------------------
 * src/main.cpp:633-725: the contigs and their reverse complements become the "reads" of one more GraphCreatorPrefSuf run with
 * MIN_OVERLAP_PREF_SUF = REMOVE_SMALL_OVERLAP_EDGES_MIN_OVERLAP = 25 (overlap lengths stop at 501 as always); the longest
 * overlap of an edge between two forward contigs that ends in contig d is cut off the left end of d (:683-712).  This call
 * replaces :636-697: contigs in (2-bit rows as everywhere, any length up to 4 194 303 nt), trim_left[n_contigs] out; the string
 * surgery of :700-712 stays with the caller.  `threshold` = 25 in the reference. */
int  alga_contig_trim_host(alga_engine *e, const uint32_t *words, int32_t stride_words, const int32_t *len, int32_t n_contigs,
                           int32_t threshold, int32_t *trim_left);

/* ---- graph dump: the reference's own checkpoint format ------------------------------------ */
/* Graph::serializeGraph (src/DataStructures/Graph.cpp:269-297): u32 n; n x {i32 id; i32 deg;
 * deg x {i32 neighbour; i32 offset}}, native endian.  Stock ALGA loads it with
 * --deserialize_graph=1 (src/main.cpp:242).  `edges` must be sorted by (src, dst, offset). */
int  alga_write_graph(const char *path, int32_t n_nodes, const alga_edge *edges, uint64_t n_edges);

/* ---- graph export: GFA 1.0, formatted on the GPU (alga_amd/csrc/gfa_kernels.hip, engine_gfa.hip) ------------------------
 * The standard exchange format of assembly / overlap graphs (Bandage, gfatools, other layout tools).  Fields are separated by one tab,
 * every line ends with '\n':  the header `H VN:Z:1.0`, the segments in ascending order of their name, the links in edge-list order.
 *   ALGA_GFA_TWINS      ALGA's layout (node 2k+1 = read k, node 2k its reverse complement; every ingest entry point produces it): twin pair k
 *                       is segment k, written when len[2k+1] > 0 (`S k <ACGT of node 2k+1> LN:i:<len>`), node 2k+1 is orientation +, 2k is -.
 *                       The twin of edge (a -> b, o), (b^1 -> a^1, len[b] - len[a] + o), is the same link: an edge is written unless its exact
 *                       twin is in the list too and has the lexicographically smaller (src, dst) (a self-twin b == a^1 once, an edge whose
 *                       twin is missing on its own).  n odd or len[2k] != len[2k+1]: ALGA_ERR_INVALID_ARGUMENT.
 *   without it          every node i with len[i] > 0 is segment i, every orientation + and every edge one link.
 *   ALGA_GFA_SEQUENCES  the segment's sequence from its 2-bit row; without it the field is `*`.
 * Edge (a -> b, o) is `L <name a> <orient a> <name b> <orient b> <len[a] - o>M`.  `nodes` and `d_edges` are device memory (a build's or the
 * supplement's result, sorted by (src, dst, offset)); ids outside [0, n), an unsorted list or a negative length answer ALGA_ERR_INVALID_ARGUMENT
 * (checked on the device) and write no file.  The text is formatted on the device in chunks (option "gfa_chunk_mb") that go down into two
 * pinned buffers in turn while a host thread writes the previous one; on any error the partial file is removed (ALGA_ERR_IO for the file
 * system's errors).  Every input must be complete before the call (the engine's own stream runs it). */
#define ALGA_GFA_TWINS     1
#define ALGA_GFA_SEQUENCES 2
typedef struct {
    uint64_t segments, links;   /* lines written                                                                         */
    uint64_t links_merged;      /* edges not written because their twin's line stands for them                           */
    uint64_t bytes;             /* size of the file                                                                      */
    double   ms_format;         /* device time of the checks, sizes, scan and formatting kernels (HIP events)             */
    double   ms_total;          /* wall time of the call                                                                 */
} alga_gfa_info;
int  alga_write_gfa_device(alga_engine *e, const alga_nodes *nodes, const alga_edge *d_edges, uint64_t n_edges, const char *path, int32_t flags,
                           alga_gfa_info *info /* may be NULL */);

/* ---- unitig graph: the maximal non-branching paths of the overlap graph, merged (alga_amd/csrc/unitig_kernels.hip, engine_unitig.hip) ----------
 * The first half of what the reference does behind the graph (GraphSimplifier::contractPathNodes, Graph::contractPath,
 * ContigCreatorSinglePath::addContractedPathToString), in its order-free core.  `nodes` is a node set in ALGA's twin layout (node 2k+1 = read k,
 * 2k = its reverse complement, v^1 = the twin of v) and `d_edges` an edge list IN ANY ORDER, both device memory (a build's result, the supplement's,
 * alga_cut_triangles_device's).  The definition (tests/unitig_checker.py states it in Python; the device result equals it byte for byte):
 *   1. checks, on the device, nothing written on refusal (ALGA_ERR_INVALID_ARGUMENT): n even, len[2k] == len[2k+1], ids in range, both ends live
 *      (len > 0), every edge (a -> b, o) a dovetail: 0 <= o < len[a] and o + len[b] >= len[a].  Offset 0 is accepted.
 *   2. E*: every edge and its twin (b^1 -> a^1, len[b] - len[a] + o); per (src, dst) only the smallest offset; sorted by (src, dst).
 *   3. u -> v of E* is COMPACTABLE when outdeg(u) == 1, indeg(v) == 1, v != u, v != u^1.
 *   4. a cycle of compactable edges is cut: m = the smallest node id over the cycle and its twin cycle; in the cycle that holds m the edge
 *      p -> m is not compactable, nor is its twin m^1 -> p^1.
 *   5. oriented unitigs = the maximal paths of compactable edges (a live node with none: a unitig of one node); the twin of v0 .. vk is vk^1 .. v0^1.
 *   6. of a unitig and its twin the one whose first node has the smaller id is orientation `+`; pairs are numbered in ascending order of that
 *      id; oriented unitig 2k+1 = `+` of pair k, 2k = `-`.
 *   7. layout of pair k (`+`): the nodes in path order with pos[v0] = 0, pos[v(i+1)] = pos[v(i)] + offset(v(i) -> v(i+1)); length
 *      L = pos[vk] + len[vk]; L > 2^31 - 1: ALGA_ERR_CAPACITY.
 *   8. sequence of pair k: base j is base j - pos[vi] of node vi for the LAST i with pos[vi] <= j; 2-bit packed like every row, ragged: pair k
 *      occupies the words d_word_off[k] .. d_word_off[k+1], unused tail bits zero.
 *   9. every edge of E* that is not compactable runs from the last node of a unitig to the first of one: (U(u) -> U(v), pos[u] + o) over
 *      oriented unitig ids, sorted by (src, dst, offset); twin-symmetric by construction.
 *  10. ALGA_UNITIG_SKIP_ISOLATED: pairs of one node without any edge in E* are left out before the numbering (Global::removeIsolatedReads).
 * The result is engine-owned device memory, valid until the next alga_unitigs_device call on `e`; the input graph is not modified. */
#define ALGA_UNITIG_SKIP_ISOLATED 1
typedef struct {
    int32_t         n_pairs;       /* oriented unitig ids: 0 .. 2 * n_pairs                                                          */
    const uint32_t *d_words;       /* the packed sequences of the `+` orientations                                                   */
    const uint64_t *d_word_off;    /* n_pairs + 1                                                                                    */
    const int32_t  *d_len;         /* n_pairs: length in bases                                                                       */
    const int32_t  *d_path_node;   /* the nodes of the `+` orientations in path order ...                                            */
    const int32_t  *d_path_pos;    /* ... and the base position of each in its unitig                                                */
    const uint64_t *d_path_off;    /* n_pairs + 1: pair k owns the entries d_path_off[k] .. d_path_off[k+1]                          */
    const alga_edge *d_edges;      /* over oriented unitig ids, sorted by (src, dst, offset), twin-symmetric                         */
    uint64_t        n_edges;
} alga_unitigs;
typedef struct {
    uint64_t edges_in, edges_sym;  /* edges given / edges of E*                                                                      */
    uint64_t twins_added;          /* (src, dst) pairs of E* that the input did not hold                                             */
    uint64_t compactable;          /* edges of E* inside unitigs, after the cycle cuts (edges_sym - unitig edges)                    */
    uint64_t cycles_cut;           /* cycles of compactable edges, a cycle and its twin cycle counted once                           */
    uint64_t isolated_skipped;     /* pairs left out by ALGA_UNITIG_SKIP_ISOLATED                                                    */
    uint64_t longest_nodes, longest_bases, total_bases, total_nodes;   /* over the pairs                                             */
    int32_t  rank_rounds;          /* pointer-jumping rounds of the list ranking: over the ruling set, over the nodes, after cycle cuts */
    double   ms_sym, ms_rank, ms_layout, ms_seq, ms_edges, ms_total;   /* device time per stage (HIP events) / wall time of the call */
} alga_unitig_info;
int  alga_unitigs_device(alga_engine *e, const alga_nodes *nodes, const alga_edge *d_edges, uint64_t n_edges, int32_t flags, void *hip_stream,
                         alga_unitigs *out, alga_unitig_info *info /* may be NULL */);
/* The unitig graph as GFA 1.0 through the kernels of alga_write_gfa_device: pair k is segment k with its spelled sequence (flags:
 * ALGA_GFA_SEQUENCES or 0), a unitig edge and its twin are one link.  `u` must be the result of the last alga_unitigs_device call on `e`.
 * ALGA_GFA_CONSENSUS (with ALGA_GFA_SEQUENCES): the segments carry the untrimmed consensus of the last alga_unitig_consensus_device call on `e`
 * (made from `u`) instead of the spelled sequence; without the flag the file is what it was before that call existed. */
#define ALGA_GFA_CONSENSUS 4
int  alga_write_unitig_gfa_device(alga_engine *e, const alga_unitigs *u, const char *path, int32_t flags, alga_gfa_info *info /* may be NULL */);

/* ---- consensus sequences of the unitigs: every column decided by the reads laid over it (alga_amd/csrc/consensus_kernels.hip, engine_consensus.hip) ----
 * The second half of what the reference does with a contracted path (Contig::correctSnipsInContig, called from
 * ContigCreatorSinglePath::getAllContigs): step 8 above spells a unitig from one read per column and so carries that read's substitutions; here
 * every column is a majority vote of all the reads over it, and the two ends are cut back to the first and last well-supported column.  On the
 * reference's fixtures whose simplified graph is one path (f1_cfg1, f3_paired) the window below IS the reference's contig, byte for byte up to
 * strand.  The build -> supplement -> cut -> parallel paths -> clip -> unitigs -> CONSENSUS -> GFA / FASTA chain stays on the device.
 * `u` must be the result of the last alga_unitigs_device call on `e` and `nodes` the node set it was made from.  The definition
 * (tests/consensus_checker.py states it in Python, once line for line after the reference and once as a pile-up; the device result equals both
 * byte for byte), for pair k with length L, path entries i = 0 .. c-1, node v_i at position p_i:
 *   votes      cnt[b][j] = the number of entries i with p_i <= j < p_i + len[v_i] whose base j - p_i is b.  The dovetail check of the unitig
 *              call guarantees that every column is covered; even nodes vote with their own rows, as step 8 reads them.
 *   base       of column j: the smallest b with the largest cnt[b][j] (std::max_element over A, C, G, T = 0 .. 3); votes[j] = that count.
 *   window     first / last = the first / last column with votes[j] > min_votes (the reference: 3; 0: nothing is trimmed; negative:
 *              ALGA_ERR_INVALID_ARGUMENT): d_trim_left[k] = first, d_len[k] = last - first + 1; no such column: both 0.
 *   output     d_words: the UNTRIMMED consensus in exactly the ragged layout of u.d_words (same d_word_off, tail bits zero) -- the trimmed
 *              sequence is a window of it, there is no second copy, and the link overlaps of the unitig graph stay valid for it;
 *              d_changed[k]: the columns of the whole unitig where the consensus differs from the spelled base; with ALGA_CONSENSUS_VOTES
 *              d_votes: one byte per column at index 16 * d_word_off[k] + j, saturated at 255 (no count saturates before the vote: a word
 *              of 16 columns that more than 255 entries cover is counted by a second kernel with 32-bit counters, `wide_words`).
 * Checks, on the device, nothing written on refusal (ALGA_ERR_INVALID_ARGUMENT): `u` is not the engine's last unitig result, nodes->n is odd or
 * not the n of that call, a path node is >= n, a length does not fit the rows or the layout of `u`.
 * The result is engine-owned device memory, valid until the next alga_unitig_consensus_device or alga_unitigs_device call on `e`. */
#define ALGA_CONSENSUS_VOTES 1
typedef struct {
    int32_t         n_pairs;       /* u.n_pairs                                                                                      */
    const uint32_t *d_words;       /* the untrimmed consensus sequences, laid out by u.d_word_off                                    */
    const int32_t  *d_trim_left;   /* n_pairs: first column of the window                                                            */
    const int32_t  *d_len;         /* n_pairs: length of the window (0: no column has more than min_votes votes)                     */
    const int32_t  *d_changed;     /* n_pairs: columns that differ from the spelled sequence                                         */
    const uint8_t  *d_votes;       /* ALGA_CONSENSUS_VOTES: 16 * total words bytes, else NULL                                        */
} alga_consensus;
typedef struct {
    uint64_t pairs, pairs_kept;    /* pairs / pairs with d_len > 0                                                                   */
    uint64_t columns;              /* sum of the unitigs' lengths                                                                    */
    uint64_t trimmed_bases;        /* sum of d_len                                                                                   */
    uint64_t changed;              /* sum of d_changed                                                                               */
    uint64_t max_depth;            /* the largest number of path entries that cover (part of) one 16-column word                     */
    uint64_t wide_words;           /* words that more than 255 entries cover (counted with 32-bit counters)                          */
    double   ms_vote, ms_window, ms_total;   /* device time of the checks and votes / of the windows (HIP events), wall time of the call */
} alga_consensus_info;
int  alga_unitig_consensus_device(alga_engine *e, const alga_nodes *nodes, const alga_unitigs *u, int32_t min_votes, int32_t flags, void *hip_stream,
                                  alga_consensus *out, alga_consensus_info *info /* may be NULL */);
/* The windows as FASTA through the chunk pipeline of alga_write_gfa_device: in pair order, for every pair with d_len[k] >= min_length and
 * d_len[k] > 0, the record `>unitig_<k>_length=<d_len[k]>\n<ACGT of the window>\n` (the sequence on one line, as OutputWriterNew::writeContig
 * writes it).  `u` / `cons` must be the last unitig / consensus results on `e`.  info: segments = records written, bytes = size of the file.
 * No pair selected: an empty file.  On an error the partial file is removed. */
int  alga_write_consensus_fasta_device(alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, const char *path, int32_t min_length,
                                       alga_gfa_info *info /* may be NULL */);

/* ---- contigs: contract, cut the contracted graph, contract again (alga_amd/csrc/contig_kernels.hip, engine_contig.hip) -------------------------
 * What the reference does between the simplified graph and its contigs (src/main.cpp:416-419: GraphSimplifier::contractPathNodes, the triangle cut
 * on the contracted graph, contractPathNodes again; ContigCreatorSinglePath::getContigOmitShortCyclesFrom: one contig per contracted edge, with the
 * junction reads at both ends), in an order-free, twin-symmetric form.  Input as for alga_unitigs_device, plus `max_offset`: the bound of
 * alga_cut_triangles_device (the reference: MAX_OFFSET_PARALLEL_PATHS).  The definition (tests/contig_checker.py states it in Python; the device
 * result equals it array for array):
 *   1. the checks of unitig step 1; B = E* (unitig step 2).
 *   2. a round on B, repeated:
 *      a. P = the nodes with indeg = outdeg = 1 whose one successor and one predecessor are neither the node nor its twin.  A cycle made only of
 *         P nodes is opened as unitig step 4 chooses: m = the smallest id over the cycle and its twin cycle; m and m^1 count as not in P.
 *         `cycles_cut` counts a cycle and its twin once (those of the final B).
 *      b. for every edge a -> b with a not in P the CHAIN is a, b, then the successors while the current node is in P; its end c is the first
 *         node not in P, its weight w the sum of the offsets.  Every edge of B lies in exactly one chain.  A chain is CLOSED when c is a or a^1;
 *         closed chains take no part in c. and d.
 *      c. among the open chains with the same (a, c) the lightest is the REPRESENTATIVE; on a tie the chain whose interior (the nodes between a
 *         and c) holds the smallest read index v >> 1 wins, a chain without interior loses; if that ties too, all the tied chains are
 *         representatives.  Every other chain of the group with w <= max_offset is DROPPED; a heavier one stays (Graph::contractPath refuses it).
 *      d. H holds one edge (a, c, w of the representative) per group.  The survivors are what alga_cut_triangles_device leaves of H at max_offset.
 *         A group whose H edge goes, or whose twin group's (c^1, a^1) H edge goes, has its representatives DROPPED (with reads of several lengths
 *         w <= max_offset is not twin-symmetric; this keeps B so).
 *      e. dropping a chain removes its edges and their twins from B.  Nothing dropped: stop.  Else the next round; there is no cap on the rounds
 *         and no host fallback (a round that continues removes at least one edge).
 *   3. the contigs are the chains of the final B, closed ones included.  Of a chain and its twin (the reversed chain of the twin nodes) the one with
 *      the smaller (first node, second node) is `+`; a chain that is its own twin occurs once.  Pairs are numbered by ascending (first node,
 *      second node) of `+`; oriented contig 2k+1 = `+` of pair k, 2k = its twin.  Layout, length and spelled sequence follow unitig steps 7-8
 *      literally (a and c are the first and the last entry; a junction read is in every contig that ends or starts there).  A node without an edge
 *      in the final B is in no contig; `reads_dropped` counts the nodes that had an edge in E* and have none now.
 *   4. the contig graph: for oriented contigs X, Y with last node of X == first node of Y the edge (X -> Y, pos of that node in X), sorted by
 *      (src, dst, offset).  In the GFA the overlap of a link is then the junction read's length.
 * The result has the alga_unitigs layout and BECOMES the engine's current unitig result: valid until the next alga_unitigs_device or
 * alga_contigs_device call on `e`; alga_unitig_consensus_device, alga_write_unitig_gfa_device and alga_write_consensus_fasta_device accept it as `u`
 * (calls made with a real unitig result behave, and write bytes, as before).  The FASTA of a contig result names its records as
 * OutputWriterNew::writeContigsNoFilter does: `>contig_id=<j>_length=<len>`, j counting the records written; the length rule is unchanged.
 * `d_edges` may be the engine-owned result of the cut, the clip or the parallel-path step: the call reads it once, into E*, before anything else,
 * and invalidates no earlier result but the unitigs and their consensus (the cut of H runs the cut's kernel on buffers of this call).
 * Refusals (ALGA_ERR_INVALID_ARGUMENT, nothing written, the previous result stays valid): where alga_unitigs_device refuses, max_offset < 0, flags != 0.
 * filterContigs' share of new reads and the N4 trim of contig ends against each other follow in alga_final_contigs_device below.
 * The extension by paired connections (markReliablePredecessorsByPairedConnections) follows in alga_extend_contigs_device below.
 * NOT reproduced (out of scope): the reference's order-dependent replacement of parallel contracted
 * paths, and its skipped last block in WorkloadManager::parallelBlockExecution.  The ABI number stays 7: the call only adds to the ABI. */
#define ALGA_CONTIG_MAX_ROUNDS 64
typedef struct {
    uint64_t edges_in, edges_sym;  /* edges given / edges of E*                                                                      */
    uint64_t rounds;               /* rounds run, the last one (which drops nothing) included                                        */
    uint64_t chains[ALGA_CONTIG_MAX_ROUNDS];              /* per round, the first 64: chains of B (both orientations, closed included) */
    uint64_t parallel_drops[ALGA_CONTIG_MAX_ROUNDS];      /* ... chains dropped by 2c                                                  */
    uint64_t groups_cut[ALGA_CONTIG_MAX_ROUNDS];          /* ... groups whose own H edge the cut removed                               */
    uint64_t base_edges_dropped[ALGA_CONTIG_MAX_ROUNDS];  /* ... edges that left B                                                     */
    uint64_t final_edges;          /* edges of the final B                                                                           */
    uint64_t path_nodes, junction_nodes;   /* of the final B: nodes in P / nodes with an edge that are not                           */
    uint64_t cycles_cut, closed_chains;    /* of the final B; closed chains in both orientations                                     */
    uint64_t reads_dropped;        /* nodes with an edge in E* and none in the final B                                               */
    uint64_t longest_nodes, longest_bases, total_bases;   /* over the pairs                                                          */
    int32_t  rank_rounds;          /* pointer-jumping rounds of all the list rankings                                                */
    double   ms_sym, ms_rounds, ms_layout, ms_seq, ms_edges, ms_total;   /* device time per stage (HIP events) / wall time of the call */
} alga_contig_info;
int  alga_contigs_device(alga_engine *e, const alga_nodes *nodes, const alga_edge *d_edges, uint64_t n_edges, int32_t max_offset, int32_t flags /* 0 */,
                         void *hip_stream, alga_unitigs *out, alga_contig_info *info /* may be NULL */);

/* ---- contigs extended through junctions that paired reads support (alga_amd/csrc/extend_kernels.hip, engine_extend.hip) ---------------------------
 * What the reference does with the pairing between its contracted graph and its contigs (ContigCreatorSinglePath::
 * markReliablePredecessorsByPairedConnections with countPairedConnections, and the walk of getContigOmitShortCyclesFrom through reliable
 * predecessors), in an order-free, twin-symmetric form.  It is the only consumer of alga_device_node_set.d_pair_off.  Inputs: the node set (n, len),
 * `d_pair_off` (n bytes of device memory, Global::pairedReadOffset: mate(v) = v, v + 2, v - 2 for the values 0, 1, 2; NULL: all zero), `u` = the
 * engine's current result, which must come from alga_contigs_device, min_chain_weight (the reference: int(2 * mean length of the live reads)),
 * min_connections (the reference: 5), max_insert (the reference: 1000), flags = 0.  The definition (tests/extend_checker.py states it in Python; the
 * device result equals it array for array):
 *   0. checks, on the device, nothing written on refusal (ALGA_ERR_INVALID_ARGUMENT): `u` is the current result and a contig result (not an
 *      extended one); nodes->n is the n of that call; pair_off[v] <= 2 and pair_off[v] == pair_off[v ^ 1]; mate(v) is in range and points back
 *      (1 <-> 2 at distance 2); min_chain_weight >= 0, max_insert >= 0, min_connections >= 1; flags == 0.
 *   1. oriented contig c in [0, 2 P) (2k+1 = `+` of pair k, 2k = `-`) has the entries e_0 .. e_(k-1) at the positions p_0 = 0 .. p_(k-1); `-` is the
 *      reversed chain of the twins: the entry made from v_i stands at L - p_i - len[v_i].  Its weight is w(c) = p_(k-1).
 *   2. the head H(c) = the read indices e_i >> 1 for 1 <= i <= k-1 with p_(i-1) <= max_insert; the tail T(c) = the entries i with 1 <= i <= k-1 and
 *      w(c) - p_i <= max_insert.  Entry 0 is in neither (the loops of countPairedConnections; the comparison is on the read index because the
 *      reference asks for the mate or its twin).
 *   3. for X, Y with last(X) == first(Y) =: a, cnt(X, Y) = the number of i in T(X) with pair_off[e_i] != 0 and mate(e_i) >> 1 in H(Y).
 *   4. X -> Y is a DIRECT link when Y is the only oriented contig that starts at a, w(X) >= min_chain_weight, w(Y) >= min_chain_weight and
 *      cnt(X, Y) >= min_connections.  L* = the direct links and their twins Y^1 -> X^1.
 *   5. a link X -> Y of L* is JOINABLE when it is the only link of L* out of X, the only one into Y, Y != X and Y != X^1.  A cycle of joinable
 *      links is opened as unitig step 4 opens it, over oriented contig ids (m = the smallest id over the cycle and its twin cycle; the link into m
 *      and its twin go).  The extended contigs are the maximal paths of joinable links (an oriented contig without one: a path of one).  Of a path
 *      and its twin the one whose first oriented contig has the smaller key c ^ 1 is `+`, and the pairs are numbered in ascending order of that key
 *      (unitig step 6 over a key that puts `+` of a pair before its `-`: a contig that no link touches keeps its orientation and its place).
 *   6. layout of a path X_1 .. X_m: the entries concatenated, a seam node once; base_1 = 0, base_(j+1) = base_j + w(X_j), position = base_j + p_i;
 *      length = base_m + L(X_m), above 2^31 - 1: ALGA_ERR_CAPACITY.  Sequences follow unitig step 8 (ragged, tail bits zero).
 *   7. the graph follows contig step 4 over the new oriented ids.
 *   8. the seam list of pair k: the path indices of the first entry of every constituent chain, plus the last entry -- m + 1 indices,
 *      d_seam_entry[d_seam_off[k] .. d_seam_off[k+1]) (alga_extend_seams_get).  These are the entries other pairs can share.
 * With no link at all the arrays equal those of `u`.
 * The result has the alga_unitigs layout and BECOMES the engine's current unitig result, as a contig result does (its FASTA names the records
 * contig_id=<j>); `u` itself is no longer valid after a successful call.  alga_final_contigs_device keeps its marks per seam read for such a result.
 * NOT reproduced: the reference extends one orientation only, emits every contig that starts in the middle of an extension as well and leaves
 * those to the filter; where several predecessors of `a` qualify it emits one overlapping contig per predecessor and its filter drops the shorter
 * ones whole -- here none is joined, and info.ambiguous counts the oriented contigs with more than one link of L* into them; an unpaired read
 * does not count (the reference compares it with itself).  The ABI number stays 7: the calls only add. */
#define ALGA_EXTEND_HEAD_SLICE 1024   /* head entries one pass of the count holds in its table */
typedef struct {
    uint64_t candidates;           /* oriented contigs X whose last node starts exactly one oriented contig                           */
    uint64_t direct_links, links;  /* direct links / links of L*                                                                     */
    uint64_t joinable;             /* joinable links, after the cycle cuts                                                           */
    uint64_t ambiguous;            /* oriented contigs with more than one link of L* into them                                       */
    uint64_t cycles_cut;           /* cycles of joinable links, a cycle and its twin cycle counted once                              */
    uint64_t pairs_in, pairs_out;
    uint64_t head_max, head_passes;   /* the largest head of a candidate that passed the weight test (entries; also without pairs) and the
                                         passes over the tail it takes: ceil(head_max / ALGA_EXTEND_HEAD_SLICE)                       */
    uint64_t longest_nodes, longest_bases, total_bases;   /* over the new pairs                                                      */
    int32_t  rank_rounds;          /* pointer-jumping rounds of both list rankings                                                   */
    double   ms_count, ms_paths, ms_layout, ms_seq, ms_edges, ms_total;   /* device time per stage (HIP events) / wall time of the call */
} alga_extend_info;
typedef struct {
    const uint64_t *d_seam_off;    /* n_pairs + 1                                                                                    */
    const int32_t  *d_seam_entry;  /* indices into the pair's own path entries (0 = its first entry)                                 */
    uint64_t        n_seams;       /* d_seam_off[n_pairs]                                                                            */
} alga_extend_seams;
int  alga_extend_contigs_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off, const alga_unitigs *u, int32_t min_chain_weight,
                                int32_t min_connections, int32_t max_insert, int32_t flags /* 0 */, void *hip_stream, alga_unitigs *out,
                                alga_extend_info *info /* may be NULL */);
/* The seam list of `u`, which must be the engine's current result and come from alga_extend_contigs_device (else ALGA_ERR_INVALID_ARGUMENT). */
int  alga_extend_seams_get(alga_engine *e, const alga_unitigs *u, alga_extend_seams *out);

/* ---- the final contig set: new-read filter, numbering, end trim, FASTA (alga_amd/csrc/final_kernels.hip, engine_final.hip) ------------------------
 * What the reference does between ContigCreatorSinglePath::getAllContigs and its output file: OutputWriterNew::filterContigs
 * (src/IO/OutputWriterNew.cpp:93-125, 150-187), the trim of the contig ends against each other (src/main.cpp:633-725), writeContigsNoFilter.
 *
 * alga_contig_trim_device: alga_contig_trim_host on ragged sequences that are in device memory already.  Sequence i is the d_len[i] bases of the
 * 2-bit packed array `d_words` from base index d_begin[i] on (any index: it need not be word-aligned); nodes 0 .. n-1 are the sequences,
 * n .. 2n-1 their reverse complements, one PrefSuf build runs with min_overlap = rsoe_min_overlap = threshold (in [1, 501]) and the defaults
 * otherwise, and d_trim_left[d] (device memory, n entries) = the largest len[i] - offset over the edges i -> d with i, d < n.  Overlap lengths
 * stop at 501, so a sequence longer than 1002 nt enters the build as its first 501 nt followed by its last 501 nt: every overlap of up to 501 nt
 * between the true sequences is one of the same length between the capped ones and the other way round, and a capped node cannot be the middle
 * of a transitive triple (that needs len = ov1 + ov2 - ov3 <= 977).  The rows of the build are at most 63 words long whatever the lengths are:
 * there is no length limit but int32.  A negative length answers ALGA_ERR_INVALID_ARGUMENT (checked on the device, nothing written).
 * The call runs a build on the engine: it invalidates the engine's last build result (the edge list of alga_prefsuf_build_device and the like)
 * and whatever the engine derived from a node set it was given before (keys, entry arrays, node statistics), as alga_contig_trim_host does.  It
 * does not touch the engine's current unitig, consensus or final result.  `edges_out` (may be NULL): the edges of that build.
 *
 * alga_final_contigs_device: `u` is the engine's current unitig result (alga_unitigs_device or alga_contigs_device), `cons` its consensus.  The
 * definition (tests/final_checker.py states it in Python; the device result equals it array for array):
 *   order      the pairs are ranked by (cons.d_len[k] descending, k ascending); d_rank[k] = the rank.  (std::sort in the reference leaves the
 *              order inside one length undefined; this is the order-free choice.)
 *   verdict    the pairs in rank order, with an empty mark set over read indices v >> 1:
 *                ALGA_FINAL_SHORT     cons.d_len[k] < min_length or cons.d_len[k] == 0.
 *                otherwise            all = the path entries of k, new = those whose read index is unmarked (a read that occurs twice in a
 *                                     closed chain counts twice);
 *                ALGA_FINAL_REJECTED  100.0 * ((double) new / (double) all) < (double) new_reads_percent, in IEEE double as the reference
 *                                     computes it (no fused or fast-math form);
 *                ALGA_FINAL_ACCEPTED  else: all the pair's read indices become marked (so the read and its twin do).
 *              d_id[k] = the number of accepted pairs ranked before k (-1: not accepted); d_new_reads[k] = new (-1: short);
 *              d_order[id] = the pair.
 *   trim       trim_threshold > 0: alga_contig_trim_device on the windows of the accepted pairs in id order, `+` orientation.  With t the value of
 *              pair k: t + 10 < cons.d_len[k]: d_begin[k] = cons.d_trim_left[k] + t, d_len[k] = cons.d_len[k] - t; else the pair becomes
 *              ALGA_FINAL_TRIMMED_AWAY (the reference writes the placeholder CCCC for such a contig; this engine leaves the record out and
 *              counts it).  Ids keep the gap.  d_trim_left[k] = t.  trim_threshold == 0: no trim (t = 0).
 *              Pairs that are not ACCEPTED in the end have d_begin = d_len = 0.
 * n_accepted = ACCEPTED + TRIMMED_AWAY pairs (the ids), n_written = ACCEPTED pairs.
 * Only the first and the last path entry of a pair can be shared with another pair (the junction reads of a contig result; a unitig result
 * shares nothing); of an extended result (alga_extend_contigs_device) the entries of its seam list can, and "end reads" below are those.
 * A pair that is accepted even with all its end reads marked needs no order; the rest is decided in rounds: a pair is decidable
 * when each of its end reads either is marked by an accepted pair of smaller rank or has no undecided pair of smaller rank.  The undecided pair of
 * the smallest rank always is: there is no cap on the rounds and no host fallback.  `filter_rounds` counts them; one count is read back per round.
 * Refusals (ALGA_ERR_INVALID_ARGUMENT, nothing written, an earlier final result stays valid): `u` / `cons` are not the engine's current results,
 * new_reads_percent outside 0 .. 100, min_length < 0, trim_threshold outside {0} and [1, 501], flags != 0.
 * The result is engine-owned device memory, valid until the next alga_unitigs_device, alga_contigs_device, alga_unitig_consensus_device or
 * alga_final_contigs_device call on `e`.  With trim_threshold > 0 the call invalidates what alga_contig_trim_device invalidates.
 *
 * alga_write_final_fasta_device: in id order, for every ALGA_FINAL_ACCEPTED pair, `>contig_id=<id>_length=<d_len>\n<ACGT of the window>\n`
 * through the chunk pipeline of alga_write_gfa_device.  `fin` must be the engine's current final result.  info: segments = records written,
 * bytes = size of the file.  No record: an empty file.  On an error the partial file is removed.  The ABI number stays 7: the calls only add. */
#define ALGA_FINAL_SHORT        0
#define ALGA_FINAL_REJECTED     1
#define ALGA_FINAL_ACCEPTED     2
#define ALGA_FINAL_TRIMMED_AWAY 3
typedef struct {
    int32_t        n_pairs;        /* u.n_pairs                                                                                       */
    int32_t        n_accepted;     /* ids handed out: ACCEPTED + TRIMMED_AWAY pairs                                                   */
    int32_t        n_written;      /* ACCEPTED pairs: the records of the FASTA                                                        */
    int32_t        reserved;
    const uint8_t *d_verdict;      /* n_pairs: ALGA_FINAL_*                                                                           */
    const int32_t *d_rank;         /* n_pairs                                                                                         */
    const int32_t *d_id;           /* n_pairs: -1 when not accepted                                                                   */
    const int32_t *d_new_reads;    /* n_pairs: -1 when short                                                                          */
    const int32_t *d_trim_left;    /* n_pairs: what the trim cuts off the window's left end                                           */
    const int32_t *d_begin;        /* n_pairs: first column of the written window in the pair's consensus row                         */
    const int32_t *d_len;          /* n_pairs: its length                                                                             */
    const int32_t *d_order;        /* n_accepted: pair by id                                                                          */
} alga_final_contigs;
typedef struct {
    uint64_t pairs, n_short, rejected, accepted, trimmed_away;   /* pairs per final verdict                                           */
    uint64_t filter_rounds;        /* rounds of the filter's schedule                                                                 */
    uint64_t trim_edges;           /* edges of the trim's build                                                                       */
    double   ms_filter, ms_trim;   /* device time (HIP events)                                                                        */
    double   ms_total;             /* wall time of the call                                                                           */
} alga_final_info;
int  alga_contig_trim_device(alga_engine *e, const uint32_t *d_words, const uint64_t *d_begin, const int32_t *d_len, int32_t n, int32_t threshold,
                             void *hip_stream, int32_t *d_trim_left, uint64_t *edges_out /* may be NULL */);
int  alga_final_contigs_device(alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, int32_t min_length, int32_t new_reads_percent,
                               int32_t trim_threshold, int32_t flags /* 0 */, void *hip_stream, alga_final_contigs *out, alga_final_info *info /* may be NULL */);
int  alga_write_final_fasta_device(alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, const alga_final_contigs *fin, const char *path,
                                   alga_gfa_info *info /* may be NULL */);

/* ---- read error correction: k-mer spectrum, one substitution per weak run ---------------------------
 * The stage between the parser and the duplicate / prefix removal.  A read with one wrong base has no exact overlap through that base; a base
 * that a spectrum of the reads themselves decides is put right here, before anything is built on it.  (The reference's own corrector,
 * src/Corrector/ReadCorrector.cpp, cannot be reached from its command line and its ties follow a hash map's iteration: this is a definition of
 * its own, free of any order, and tests/correct_checker.py states it literally.)
 *
 * In: the parser's node layout (alga_parsed_reads): n_nodes (even) rows of 2-bit bases, LSB first, stride_words apart; node 2r + 1 is read r,
 * node 2r its reverse complement.  A pair with len < k (-1 and 0 included) takes no part and stays as it is.
 *   1. Spectrum.  The canonical form of a k-mer is the smaller of the k-mer and its reverse complement under any fixed injective encoding
 *      (nothing observable depends on which).  count[x] = occurrences of x over all k-mers of all forward reads (odd nodes) with len >= k;
 *      x is SOLID iff count[x] >= solid_min.  The spectrum is that of the reads as they came in: fixes do not feed back into it.
 *   2. Weak runs.  Of a forward read of length l, nk = l - k + 1; k-mer i (bases i .. i + k - 1) is weak iff its canonical form is not solid.
 *      Runs are the maximal intervals [a, b] of weak k-mers of the unmodified read, len = b - a + 1.
 *   3. The suspected base p of a run:
 *        whole read   a == 0 && b == nk - 1    skipped
 *        interior     a > 0  && b <  nk - 1    p = b, only if len == k; otherwise skipped
 *        left end     a == 0 && b <  nk - 1    p = b, only if b <= k - 1; otherwise skipped
 *        right end    a > 0  && b == nk - 1    p = a + k - 1, only if len <= k; otherwise skipped
 *      and len < min_run is skipped in every case.
 *   4. Candidates.  A base x != read[p] WORKS iff every k-mer a .. b of the read with read[p] := x (all other bases as they came in) is solid.
 *      Exactly one x works: fixed.  None: no_candidate.  Two or three: ambiguous.  Nothing is written for the last two.
 *   5. Output.  All fixes of a read are applied together, row 2r becomes the reverse complement of the new row 2r + 1; lengths, tail bits (zero)
 *      and every other node are untouched.
 *   6. Counters: alga_correct_info.
 * The rule is strand-symmetric (left-end and right-end runs map onto each other), and the runs of one read are independent: the k-mers of one
 * run never contain the p of another.  Two errors closer than k + 1 apart make one run longer than k and stay: one base per run is the only
 * fix a spectrum alone decides.
 *
 * Checked on the device before anything is written (ALGA_ERR_INVALID_ARGUMENT, rows untouched): row 2r is the reverse complement of row
 * 2r + 1, len[2r] == len[2r + 1], blocks of len <= stride_words.  k even or outside 5 .. 31, solid_min < 1, min_run < 1, n_nodes odd: the same
 * answer.  The k-mers are counted in slices of the (mixed) key space of at most "correct_slice_keys" occurrences each (alga_engine_set_option;
 * default 2^28; a single bin of the 4096 above that is a slice of its own and the buffers follow the largest slice); the solid keys are looked
 * up through a directory of "correct_dir_bits" bits (0 = about two keys per bucket).  Neither option changes a result. */
typedef struct {
    int32_t k;                       /* odd, 5 .. 31; default 21                                                                      */
    int32_t solid_min;               /* >= 1; default 3                                                                               */
    int32_t min_run;                 /* >= 1; default 1                                                                               */
    int32_t reserved;                /* 0                                                                                             */
} alga_correct_params;
typedef struct {
    uint64_t reads;                  /* forward reads with len >= k                                                                   */
    uint64_t kmers_total, kmers_distinct, kmers_solid;
    uint64_t runs, runs_fixed, runs_ambiguous, runs_no_candidate, runs_skipped;
    uint64_t reads_changed;
    uint64_t slices;                 /* slices the count ran in (depends on "correct_slice_keys" alone)                               */
    double   ms_count, ms_index, ms_fix;   /* device time (HIP events): histogram + slices, directory, k_cr_fix                       */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_correct_info;
void alga_correct_default_params(alga_correct_params *p);
/* in place on caller-owned device arrays */
int  alga_correct_reads_device(alga_engine *e, uint32_t *d_rows, int32_t stride_words, const int32_t *d_len, int64_t n_nodes, const alga_correct_params *p,
                               void *hip_stream, alga_correct_info *info /* may be NULL */);
/* host arrays up, corrected, down again: what sits between alga_parse_files and alga_preprocess_nodes.  On a refusal pr is untouched. */
int  alga_correct_parsed_reads(alga_engine *e, alga_parsed_reads *pr, const alga_correct_params *p, alga_correct_info *info /* may be NULL */);
/* alga_ingest_device with the correction between its parse kernels and the duplicate / prefix removal (fixes make new duplicates and prefix
 * reads: that is why the stage sits in front of their removal) */
int  alga_ingest_corrected_device(alga_engine *e, const char *file1, const char *file2 /* may be NULL */, const alga_ingest_params *p, const alga_correct_params *cp,
                                  alga_device_node_set *out, alga_ingest_info *info, alga_correct_info *cinfo /* may be NULL */);

/* ---- reads placed on sequences: depth, pairs, inserts (alga_amd/csrc/place_kernels.hip, engine_place.hip) -------------------------
 * Every input read laid over a set of target sequences (the final contigs, or any ragged set): where it lies, how many reads cover every
 * column, and what the pairs say about the library.  Substitutions only: no insertions, deletions or clipped ends.  The rule is free of any
 * order (thread, slice, hash); tests/place_checker.py states it in Python and the device result equals it array for array.
 *
 * Targets.  T sequences; target t is the d_len[t] bases of the 2-bit packed array `d_words` from base index d_begin[t] on (any index, it
 * need not be word-aligned: the form alga_contig_trim_device takes).  col_off[t] = the exclusive prefix sum of d_len (col_off[T] = the sum,
 * the number of columns).  A sum above 2^32 - 2 answers ALGA_ERR_CAPACITY (before anything of that size is allocated), a negative length
 * ALGA_ERR_INVALID_ARGUMENT (checked on the device, nothing written).
 * Reads.  A node set in twin layout: n even, rows stride_words apart, d_len; node 2r + 1 is read r, node 2r its reverse complement (the
 * parser's layout, where len -1 means removed, and alga_device_node_set).  d_pair_off: NULL (= all zero) or n bytes, mate(v) = v, v + 2,
 * v - 2 for the values 0, 1, 2 as in alga_extend_contigs_device.  Checked on the device before anything is written
 * (ALGA_ERR_INVALID_ARGUMENT): row 2r is the reverse complement of row 2r + 1, len[2r] == len[2r + 1], len <= 16 * stride_words;
 * pair_off[v] <= 2, pair_off[v] == pair_off[v ^ 1], the mate is in range and points back.  A read with len < k takes no part: its state is 0.
 * Parameters (alga_place_params; anything outside answers ALGA_ERR_INVALID_ARGUMENT): k 8 .. 31 (default 21), max_mismatches 0 .. 254 (4),
 * max_occ 1 .. 65535 (256), max_insert 1 .. 2^20 (1000), flags ALGA_PLACE_DEPTH_MULTI or 0 (0).
 *
 *   1. Index.  Position (t, q) is indexed for 0 <= q <= len[t] - k; no k-mer spans two targets, also where the targets abut in d_words.
 *      occ(x) = the number of indexed positions whose k-mer is x.
 *   2. Seeds.  Node v of length L has S = floor(L / k) seeds, seed j = bases jk .. jk + k - 1.  A seed is USABLE iff
 *      1 <= occ(its k-mer) <= max_occ.
 *   3. Placement.  (t, p) is a placement of node v iff 0 <= p <= len[t] - L, the Hamming distance mm between v and t[p .. p + L) is
 *      <= max_mismatches, and some usable seed j of v equals t[p + jk .. p + jk + k) exactly.  (With S > max_mismatches and no seed over
 *      max_occ the third condition follows from the second by pigeonhole: "all placements within the bound".)  Placements of node 2r + 1 are
 *      `+` placements of read r, those of node 2r `-` placements; p is always the leftmost column covered.  A placement is a distinct triple
 *      (t, p, strand): several seeds hitting the same triple make one placement.
 *   4. Per read.  best = the smallest (mm, t, p, strand) with + < -; hits = the number of placements with mm == best.mm, saturated at 255;
 *      state bits ALGA_PLACE_PLACED, ALGA_PLACE_UNIQUE (hits == 1), ALGA_PLACE_MINUS.  d_target (-1 if not placed), d_pos (-1), d_mm (0),
 *      d_hits (0), d_state (0), one entry per read.
 *   5. Depth.  A read COUNTS iff it is UNIQUE; with ALGA_PLACE_DEPTH_MULTI iff it is PLACED, at its best placement.
 *      d_cover[col_off[t] + j] = the number of counting reads whose best placement covers column j of t.  Per target: d_t_reads = the
 *      counting reads, d_t_bases = the sum of their lengths, d_t_mismatches = the sum of their mm, d_t_uncovered = the columns with cover 0.
 *   6. Pairs.  Each pair is judged once, from the mate with the smaller read index.  Not both UNIQUE: pairs_not_unique.  Both UNIQUE on
 *      different targets: pairs_split.  Both UNIQUE on the same target: with a, la the position and length of the `+` read and b, lb of the
 *      `-` read, the pair is PROPER iff the strands differ, a <= b, a + la <= b + lb and insert = b + lb - a <= max_insert; a proper pair
 *      does d_insert_hist[insert]++ (max_insert + 1 bins); anything else on the same target is pairs_improper.  insert_median = the smallest i
 *      whose cumulative count reaches (proper + 1) / 2 (computed on the host from the histogram; -1 without proper pairs);
 *      insert_mean_x100 = floor(100 * sum of the inserts / proper) (-1 without proper pairs).
 *   7. Counters (alga_place_info): reads = n / 2, placed, unique, multi = placed - unique, unplaced = reads - placed; hits_saturated = reads
 *      with more than 255 placements at best.mm; seeds = the seeds of all nodes with len >= k (both strands), seeds_over_max_occ = those with
 *      occ > max_occ; index_positions, index_distinct (distinct k-mers among them); pairs = pairs_proper + pairs_improper + pairs_split +
 *      pairs_not_unique.
 * The lookups go through a directory on the top "place_dir_bits" bits of the k-mer (alga_engine_set_option; 0 = about two positions per
 * bucket): the option changes no result.  Three read-backs: the refusal flags with the column count, the counters, the histogram.
 * The result is engine-owned device memory, valid until the next placement call on `e`; a refused call leaves an earlier result valid.
 *
 * alga_place_reads_on_final_device: target t is the window of the pair fin.d_order[t] (target id == contig id): it begins at base
 * 16 * u.d_word_off[k] + fin.d_begin[k] of cons.d_words and has length fin.d_len[k]; a TRIMMED_AWAY pair is a target of length 0.  `u`,
 * `cons` and `fin` must be the engine's current results (refused as alga_write_final_fasta_device refuses); the call does not invalidate them.
 * alga_write_final_fasta_depth_device: the records and sequences of alga_write_final_fasta_device with the header
 * `>contig_id=<id>_length=<len>_reads=<t_reads>_depth=<q>.<dd>`, <q>.<dd> = floor(100 * t_bases / len) in integers, two decimals, formatted on
 * the device.  `placements` must be the engine's current result of alga_place_reads_on_final_device on `fin`.  ABI stays 7: the calls add. */
#define ALGA_PLACE_DEPTH_MULTI 1     /* alga_place_params.flags                                                                       */
#define ALGA_PLACE_PLACED 1          /* bits of d_state                                                                               */
#define ALGA_PLACE_UNIQUE 2
#define ALGA_PLACE_MINUS  4
typedef struct {
    int32_t k, max_mismatches, max_occ, max_insert, flags;
    int32_t reserved[3];             /* 0                                                                                             */
} alga_place_params;
typedef struct {
    int64_t         n_reads;         /* n / 2                                                                                         */
    int64_t         n_targets;
    uint64_t        n_columns;       /* col_off[n_targets]                                                                            */
    int64_t         n_hist;          /* max_insert + 1                                                                                */
    const int32_t  *d_target, *d_pos;                /* n_reads                                                                       */
    const uint8_t  *d_mm, *d_hits, *d_state;         /* n_reads                                                                       */
    const uint32_t *d_col_off;       /* n_targets + 1                                                                                 */
    const uint32_t *d_cover;         /* n_columns                                                                                     */
    const uint64_t *d_t_reads, *d_t_bases, *d_t_mismatches, *d_t_uncovered;   /* n_targets                                            */
    const uint64_t *d_insert_hist;   /* n_hist                                                                                        */
} alga_placements;
typedef struct {
    uint64_t reads, placed, unique, multi, unplaced;
    uint64_t hits_saturated, seeds, seeds_over_max_occ;
    uint64_t index_positions, index_distinct;
    uint64_t pairs, pairs_proper, pairs_improper, pairs_split, pairs_not_unique;
    int64_t  insert_median, insert_mean_x100;
    double   ms_index, ms_place, ms_depth;           /* device time (HIP events): gather + index, the placement kernel, depth + pairs */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_place_info;
void alga_place_default_params(alga_place_params *p);
int  alga_place_reads_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off /* may be NULL */, const uint32_t *d_words,
                             const uint64_t *d_begin, const int32_t *d_len, int32_t n_targets, const alga_place_params *p, void *hip_stream,
                             alga_placements *out, alga_place_info *info /* may be NULL */);
int  alga_place_reads_on_final_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off /* may be NULL */, const alga_unitigs *u,
                                      const alga_consensus *cons, const alga_final_contigs *fin, const alga_place_params *p, void *hip_stream,
                                      alga_placements *out, alga_place_info *info /* may be NULL */);
int  alga_write_final_fasta_depth_device(alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, const alga_final_contigs *fin,
                                         const alga_placements *placements, const char *path, alga_gfa_info *info /* may be NULL */);

/* ---- the placed targets polished: every column voted again by every placed read (alga_amd/csrc/polish_kernels.hip, engine_polish.hip) ----
 * The consensus decides a column from the reads of the contig's PATH; after the placement every input read lies over the final sequences,
 * also those the graph stages dropped.  This stage lets them all vote.  Substitutions only, integers only, free of any order (thread, sort);
 * tests/polish_checker.py states the rule twice in Python and the device result equals it array for array.
 *
 * Inputs: the node set that was placed (twin layout), the engine's current placement result `pl` (from either placement call), and
 * alga_polish_params: min_cover 1 .. 2^31 - 1 (default 3), min_percent 1 .. 100 (60), flags ALGA_POLISH_MULTI | ALGA_POLISH_COUNTS (0);
 * anything else answers ALGA_ERR_INVALID_ARGUMENT.
 *
 *   1. Voters.  Read r votes iff its state has ALGA_PLACE_UNIQUE; with ALGA_POLISH_MULTI iff it has ALGA_PLACE_PLACED; at its best placement.
 *      Its voting node is v = 2r if ALGA_PLACE_MINUS, else 2r + 1.  With L = len[v] and g0 = col_off[target[r]] + pos[r], base i of v gives
 *      one vote for its code at column g0 + i, 0 <= i < L.
 *   2. Counts.  count[g][b] = the votes for base b at column g, exact up to 2^32 - 1; cover[g] = their sum over b.  (Where the placement's
 *      depth mode agrees with the flag, cover[g] == pl.d_cover[g].)
 *   3. Decision.  cur = the base of the placed target at column g, read from the column array the placement call kept (the caller does not
 *      pass the targets again).  w = the base with the largest count; a tie goes to cur if it is among the tied bases, else to the smallest
 *      code.  Column g CHANGES to w iff w != cur, cover[g] >= min_cover and 100 * count[g][w] >= min_percent * cover[g] (64-bit products);
 *      it is AMBIGUOUS iff w != cur, cover[g] >= min_cover and the percentage test fails; every other column keeps cur.
 *   4. Result (alga_polished; engine-owned, valid until the next polish call on `e`: a later placement call does not invalidate it, a refused
 *      call leaves an earlier result valid).  n_targets, n_columns, d_col_off (a copy of the placement's); d_words: the polished targets in
 *      column space, column g in word g >> 4 at bits 2 * (g & 15), (n_columns + 15) / 16 + 2 words, the bits past n_columns zero; n_changed,
 *      d_changed_cols (uint32, ascending), d_changed_bases (uint8, old | new << 2); d_t_changed, d_t_ambiguous (uint64 per target); with
 *      ALGA_POLISH_COUNTS d_counts, uint32 [4 * n_columns], the count of base b of column g at 4 * g + b, else NULL.
 *      (d_words, begin[t] = col_off[t], len[t] = col_off[t + 1] - col_off[t]) is a ragged target set as alga_place_reads_device takes it:
 *      a second round is place -> polish on the first round's output.  The polish reads cur from the placement's copy, so it may overwrite
 *      the buffer its own targets came from.
 *   5. Counters (alga_polish_info): columns, voters, votes (the sum of their lengths), voted_columns (cover >= min_cover), changed,
 *      ambiguous, max_cover; ms_sort, ms_vote (HIP events), ms_total (wall).
 *   6. Refusals, all checked on the device before anything of the result is written (ALGA_ERR_INVALID_ARGUMENT): `pl` is not the engine's
 *      current placement result; nodes->n / 2 != pl.n_reads; a voter with len < 1 or len > 16 * stride_words; a voter with its target
 *      outside [0, n_targets), pos < 0 or pos + len > len[target].  The last check is what keeps a wrong node set from writing outside the
 *      arrays: the vote kernel relies on it and on nothing else.  An allocation that fails answers ALGA_ERR_OUT_OF_MEMORY (d_counts takes
 *      16 bytes per column).
 * The voters are sorted by first column with the engine's radix sort; every output word is then GATHERED by one lane (no atomic per base),
 * bit-sliced counters up to a cover of 255 and 32-bit counters above.  One read-back for the checks, one for the counters.
 *
 * alga_write_polished_fasta_device: the records of alga_write_final_fasta_device (depth_header == 0) or of
 * alga_write_final_fasta_depth_device (!= 0) -- same ids, lengths and order -- with the sequence taken from pol.d_words.  `pl` must be the
 * engine's current result of alga_place_reads_on_final_device on `fin`, `pol` the current polish of it.  ABI stays 7: the calls add. */
#define ALGA_POLISH_MULTI  1         /* alga_polish_params.flags                                                                      */
#define ALGA_POLISH_COUNTS 2
typedef struct {
    int32_t min_cover, min_percent, flags;
    int32_t reserved[5];             /* 0                                                                                             */
} alga_polish_params;
typedef struct {
    int64_t         n_targets;
    uint64_t        n_columns;
    uint64_t        n_changed;
    const uint32_t *d_col_off;       /* n_targets + 1                                                                                 */
    const uint32_t *d_words;         /* (n_columns + 15) / 16 + 2                                                                     */
    const uint32_t *d_changed_cols;  /* n_changed                                                                                     */
    const uint8_t  *d_changed_bases; /* n_changed                                                                                     */
    const uint64_t *d_t_changed, *d_t_ambiguous;     /* n_targets                                                                     */
    const uint32_t *d_counts;        /* 4 * n_columns, or NULL                                                                        */
} alga_polished;
typedef struct {
    uint64_t columns, voters, votes, voted_columns, changed, ambiguous, max_cover;
    double   ms_sort, ms_vote;       /* device time (HIP events): keys + sort, the votes + the change list                            */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_polish_info;
void alga_polish_default_params(alga_polish_params *p);
int  alga_polish_placed_device(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_polish_params *p,
                               void *hip_stream, alga_polished *out, alga_polish_info *info /* may be NULL */);
int  alga_write_polished_fasta_device(alga_engine *e, const alga_unitigs *u, const alga_consensus *cons, const alga_final_contigs *fin,
                                      const alga_placements *pl, const alga_polished *pol, int32_t depth_header, const char *path,
                                      alga_gfa_info *info /* may be NULL */);

/* ---- scaffolds from split pairs: links, joins, order, gaps, FASTA (alga_amd/csrc/scaffold_kernels.hip, engine_scaffold.hip) ---------------
 * alga_extend_contigs_device joins contigs only through junctions of the overlap graph.  A pair whose mates are both uniquely placed on
 * DIFFERENT targets (the placement's pairs_split) says that two targets lie near each other although no edge joins them; this stage turns
 * those pairs into scaffolds.  Integers only, free of any order (thread, sort); tests/scaffold_checker.py states the rule twice in Python
 * and the device result equals it array for array.  The library is forward-reverse, as the placement's PROPER rule assumes.
 *
 * Inputs: the node set that was placed (twin layout), d_pair_off as alga_place_reads_device takes it (NULL = no pairs), the engine's
 * current placement result `pl` (from either placement call), and alga_scaffold_params: insert 0 .. 2^20 (no default: the library's insert
 * size, usually the placement's insert_median), max_insert 1 .. 2^20 (default 1000), min_links 1 .. 2^31 - 1 (5, the default of the
 * extension's min_connections), max_second_percent 1 .. 100 (50), min_gap 1 .. 2^20 (10), flags 0, reserved 0; anything else answers
 * ALGA_ERR_INVALID_ARGUMENT.
 *
 *   1. Ends and reach.  Target t has a left end x = 2t and a right end x = 2t + 1.  A UNIQUE read r lies on target t at p with length
 *      L = len[2r + 1].  A `+` placement (no ALGA_PLACE_MINUS) points out of the right end: e(r) = 1, d(r) = len[t] - p; a `-` placement
 *      out of the left end: e(r) = 0, d(r) = p + L.  The read's end is x(r) = 2t + e(r).
 *   2. Links.  Pairs are judged as in the placement: by the mate with the smaller read index (pair_off[2r + 1] == 1), its mate is r + 1.
 *      A pair takes part iff both mates are UNIQUE and on different targets (pairs_split: it equals the placement's).  span = d(r) +
 *      d(r + 1).  The pair is a LINK between x(r) and x(r + 1) iff span <= max_insert, else it counts in links_too_far.  A link's key is
 *      (a, b) = (min, max) of its two ends.
 *   3. Bundles.  A bundle is all the links of one key: n links, S the 64-bit sum of their spans, gap = insert - floor(S / n) (int32, may be
 *      negative).  It is SUPPORTED iff n >= min_links.  The bundles are listed in ascending (a, b).
 *   4. Choice per end.  Among the SUPPORTED bundles at end x, ordered by (n descending, partner end ascending), n1 is the first and n2 the
 *      second if there is one.  x is AMBIGUOUS iff a second exists and 100 * n2 >= max_second_percent * n1 (64-bit products).  choice(x) =
 *      the first bundle's partner iff x has a supported bundle and is not ambiguous; else x has no choice.
 *   5. Joins.  A bundle (a, b) is a JOIN iff choice(a) == b and choice(b) == a.  Every end then has at most one join: the targets form
 *      paths and cycles (two bundles between the same two contigs at different ends make a ring of two).
 *   6. Cycles.  A cycle is opened at its smallest contig id c: the join at end 2c is dropped.  Its bundle keeps SUPPORTED | JOIN and gets
 *      DROPPED_CYCLE; it counts in joins_dropped_cycle and not in joins, and its two ends are not JOINED.
 *   7. Scaffolds.  A target of length 0 belongs to no scaffold (scaffold = rank = -1, everything else 0).  Every other target belongs to
 *      exactly one scaffold, a path of at least one contig.  A path of one contig has orientation +.  A longer path starts at whichever
 *      of its two terminal contigs has the smaller id; the start contig is entered at its free end.  A contig entered at end e has
 *      orientation + (d_orient 0) iff e == 0, else - (1, reverse-complemented); it is left at e ^ 1, through that end's join, into the
 *      partner end's contig.  Scaffolds are numbered by ascending id of their first contig; rank counts from 0 along the path.
 *   8. Layout.  gap_after[c] = max(gap of the join by which c is left, min_gap), 0 for the last contig of a scaffold; join_links[c] = that
 *      join's n, 0 for the last.  start[c] = the uint64 sum of the lengths and gap_after of the contigs before c in its scaffold; s_len =
 *      the scaffold's length with its gaps.
 *   9. Result (alga_scaffolds; engine-owned, valid until the next scaffold call on `e`: a later placement or polish call does not
 *      invalidate it, a refused call leaves an earlier result valid).  d_s_off[j] .. d_s_off[j + 1] are the places of scaffold j's contigs
 *      in d_s_members (contig ids in scaffold order); n_members = the targets with a length.
 *  10. Counters (alga_scaffold_info): pairs_split, links, links_too_far; bundles, bundles_supported; ends_ambiguous; joins,
 *      joins_dropped_cycle; scaffolds, scaffolds_multi (more than one contig); longest (the largest s_len); n50_targets, n50_scaffolds
 *      (host, from the lengths read back: the N50, the largest length l such that the sequences of length >= l hold at least half of all
 *      bases, 0 for an empty set; the scaffolds with their gaps); ms_links (links + sort + bundles), ms_chain (choice, joins, ranking, layout)
 *      (HIP events), ms_total (wall).
 *  11. Refusals, all before anything of the result is written (ALGA_ERR_INVALID_ARGUMENT).  On the host: `pl` is not the engine's current
 *      placement result; nodes->n / 2 != pl.n_reads.  On the device (k_sc_check, one read-back): pair_off is malformed (the placement's
 *      check, repeated because the array is passed again); a UNIQUE read with len < 1 or len > 16 * stride_words, its target outside
 *      [0, n_targets), pos < 0 or pos + len > len[target].  An allocation that fails, on the device or for the host copies of the lengths,
 *      answers ALGA_ERR_OUT_OF_MEMORY.  "Current" is judged as the polish judges it, by the struct's buffers and sizes: a struct kept from
 *      an earlier placement call of the same shapes names the same engine buffers and is taken for the current one -- what is read is
 *      then the current placement's data.  (Which placement a scaffold or polish RESULT was made from is tracked by a serial number inside
 *      the engine, so alga_write_scaffold_fasta_device cannot be given a scaffold or polish of an earlier placement.)
 * The links are sorted by a << 32 | b with sort_u64_u32 (the value is the judging read); a scan over the heads numbers the bundles, whose
 * arrays are allocated at their size after the count comes back.  Contig c entered at end e is state 2c + e with succ = the partner of the
 * join at the other end: pointer jumping over the 2T states finds the cycles (the smallest id rides along), then ranks the paths and sums
 * their lengths and gaps in the same jumps.  Nothing walks on the host.
 *
 * alga_write_scaffold_fasta_device: one record per scaffold in id order, `>scaffold_id=<j>_length=<s_len>_contigs=<m>`, then its contigs
 * (reverse-complemented where d_orient is 1) with gap_after `N`s behind each but the last, on one line.  The bases come from the column
 * array the placement kept, or from pol->d_words.  `pl` must be the engine's current placement, `scaf` its current scaffold result and
 * made from `pl`, `pol` (may be NULL) the current polish of `pl`; otherwise the call is refused.  ABI stays 7: the calls add. */
#define ALGA_SCAFFOLD_BUNDLE_SUPPORTED     1   /* bits of d_b_state                                                                   */
#define ALGA_SCAFFOLD_BUNDLE_JOIN          2
#define ALGA_SCAFFOLD_BUNDLE_DROPPED_CYCLE 4
#define ALGA_SCAFFOLD_END_HAS_SUPPORTED    1   /* bits of d_end_state                                                                 */
#define ALGA_SCAFFOLD_END_AMBIGUOUS        2
#define ALGA_SCAFFOLD_END_JOINED           4
typedef struct {
    int32_t insert, max_insert, min_links, max_second_percent, min_gap, flags;
    int32_t reserved[2];             /* 0                                                                                             */
} alga_scaffold_params;
typedef struct {
    int64_t         n_targets, n_bundles, n_scaffolds, n_members;
    const uint32_t *d_b_a, *d_b_b, *d_b_links;       /* n_bundles                                                                     */
    const uint64_t *d_b_span;
    const int32_t  *d_b_gap;
    const uint8_t  *d_b_state;
    const uint8_t  *d_end_state;     /* 2 * n_targets                                                                                 */
    const int32_t  *d_scaffold, *d_rank;             /* n_targets                                                                     */
    const uint8_t  *d_orient;
    const uint64_t *d_start;
    const int32_t  *d_gap_after;
    const uint32_t *d_join_links;
    const uint32_t *d_s_off;         /* n_scaffolds + 1                                                                               */
    const int32_t  *d_s_members;     /* n_members                                                                                     */
    const uint64_t *d_s_len;         /* n_scaffolds                                                                                   */
} alga_scaffolds;
typedef struct {
    uint64_t pairs_split, links, links_too_far, bundles, bundles_supported, ends_ambiguous, joins, joins_dropped_cycle;
    uint64_t scaffolds, scaffolds_multi, longest, n50_targets, n50_scaffolds;
    double   ms_links, ms_chain;     /* device time (HIP events): links + sort + bundles; choice, joins, ranking, layout              */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_scaffold_info;
void alga_scaffold_default_params(alga_scaffold_params *p);   /* insert is left 0: the caller sets it                                 */
int  alga_scaffold_placed_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off /* may be NULL */, const alga_placements *pl,
                                 const alga_scaffold_params *p, void *hip_stream, alga_scaffolds *out, alga_scaffold_info *info /* may be NULL */);
int  alga_write_scaffold_fasta_device(alga_engine *e, const alga_placements *pl, const alga_scaffolds *scaf, const alga_polished *pol /* may be NULL */,
                                      const char *path, alga_gfa_info *info /* may be NULL */);

/* ---- contigs broken where no read pair spans them (alga_amd/csrc/break_kernels.hip, engine_break.hip) -------------------------------------
 * Every stage after the graph keeps a contig whole or joins contigs.  The placement holds the evidence against a contig: for every uniquely
 * placed pair the target, both positions and both strands.  A column that no proper pair's fragment spans, while columns on both sides of it
 * are spanned, is a join that no clone of the library supports; the contig is cut there.  Integers only, free of any order (thread, atomics);
 * tests/break_checker.py states the rule twice in Python and the device result equals it array for array.  place -> [polish] -> break ->
 * place on the pieces -> scaffold.
 *
 * Inputs: the node set that was placed (twin layout), d_pair_off as alga_place_reads_device takes it (NULL = no pairs), the engine's
 * current placement result `pl` (from either placement call), optionally the current polish `pol` of that placement, and alga_break_params:
 * min_span 1 .. 2^31 - 1 (default 1), inset 0 .. 2^20 (21), margin 0 .. 2^20 (no default: the caller sets it, usually the placement's
 * insert_median), flags 0, reserved 0; anything else answers ALGA_ERR_INVALID_ARGUMENT.
 *
 *   1. Proper pairs.  A pair is PROPER exactly as item 6 of the placement defines it, with max_insert = pl.n_hist - 1.  Each pair is judged
 *      once, from the mate with the smaller read index.  pairs_proper of this call equals the placement's.
 *   2. Span.  A proper pair has its `+` read at a and its `-` read at b, lengths la and lb.  It SPANS column j of its target iff
 *      a + inset <= j < b + lb - inset.  A pair with b + lb - a <= 2 * inset spans nothing (it still counts in pairs_proper); the pairs that
 *      span something count in pairs_spanning.  span[g] = the number of proper pairs that span column g, in column space, uint32.
 *      (inset is part of the rule: with up to max_mismatches substitutions tolerated, a read may overhang a misjoin by a few columns.)
 *   3. Candidates.  Column j of target t is a CANDIDATE iff margin <= j < len[t] - margin.  A candidate is WEAK iff span < min_span.
 *   4. Runs.  A run is a maximal stretch of consecutive weak candidates of one target; it never crosses a target boundary, also where
 *      targets abut.
 *   5. Closed and open.  A run s .. e is CLOSED iff columns s - 1 and e + 1 are both candidates of the same target (they are then not weak).
 *      Every other run is OPEN and cuts nothing: a whole target with no pair on it, single-end data, a run that touches the margin.
 *   6. Cuts.  Every closed run makes one cut, at column c = floor((s + e + 1) / 2): the pieces are [.., c) and [c, ..).  Nothing is removed.
 *   7. Pieces, numbered in column order; a target of length 0 stays one piece of length 0 in its place.  n_pieces = n_targets + n_cuts;
 *      piece j is the columns d_piece_off[j] .. d_piece_off[j + 1]; d_piece_target[j] its source target, d_piece_start[j] its offset there.
 *   8. Result (alga_broken; engine-owned, valid until the next break call on `e`: a later placement, polish or scaffold call does not
 *      invalidate it, a refused call leaves an earlier result valid).  d_span [n_columns]; d_cut_cols (ascending, column space), d_cut_first,
 *      d_cut_last (the run of each cut) [n_cuts]; d_t_cuts uint32 [n_targets]; d_piece_off [n_pieces + 1]; d_begin uint64, d_len int32,
 *      d_piece_target, d_piece_start [n_pieces]; d_words: the result's OWN copy of the bases in column space (the polish's layout,
 *      (n_columns + 15) / 16 + 2 words, the bits past n_columns zero), taken from the column array the placement kept or from pol->d_words.
 *      (d_words, d_begin, d_len, n_pieces) is a target set as alga_place_reads_device takes it; the copy is what lets the next placement,
 *      which overwrites its own column array, read it.
 *   9. Counters (alga_break_info): pairs_proper, pairs_spanning; candidate_columns, weak_columns; runs, runs_open; cuts, targets_cut, pieces;
 *      max_span (over all columns), longest_piece; n50_targets, n50_pieces (the scaffold's N50, on the host from lengths read back only when
 *      `info` is given); ms_span (the check, the pair pass, the scan), ms_cut (flags, compaction, pieces, the copy) (HIP events), ms_total (wall).
 *  10. Refusals, all before anything of the result is written (ALGA_ERR_INVALID_ARGUMENT).  On the host: `pl` is not the engine's current
 *      placement result, judged by its buffers and by ALL its sizes (n_reads, n_targets, n_columns, n_hist: a struct kept from an earlier
 *      placement of the same reads on other targets is refused, since n_columns sizes every column array and n_hist - 1 is max_insert);
 *      nodes->n / 2 != pl.n_reads; `pol` is given but is not the current polish of this placement.  On the device
 *      (k_br_check, one read-back): pl.n_columns != col_off[n_targets]; pair_off fails the placement's test; a UNIQUE read with len < 1 or len > 16 * stride_words, its target
 *      outside [0, n_targets), pos < 0 or pos + len > len[target].  The column check and the last read check are what the pair kernel's
 *      writes into the difference array rely on.
 * One pass over the reads (integer atomics on a difference array of n_columns + 1 entries), a scan, one pass over the columns, and two
 * compactions by scan: of the runs (the i-th start belongs to the i-th end), then of the closed ones.  Read-backs: the refusal flags, the run
 * count, the cut count (the run, cut and piece arrays are allocated at their size), the counters.
 *
 * alga_write_broken_fasta_device: one record per piece with a length, in piece order, `>contig_id=<j>_length=<len>_from=<t>_start=<s>`: j is
 * the piece id (the target id of a later placement on the pieces), t and s its source target and offset.  `brk` must be the engine's
 * current break result.  ABI stays 7: the calls add. */
typedef struct {
    int32_t min_span, inset, margin, flags;
    int32_t reserved[4];             /* 0                                                                                             */
} alga_break_params;
typedef struct {
    int64_t         n_targets, n_pieces, n_cuts;
    uint64_t        n_columns;
    const uint32_t *d_span;          /* n_columns                                                                                     */
    const uint32_t *d_cut_cols, *d_cut_first, *d_cut_last;   /* n_cuts                                                                */
    const uint32_t *d_t_cuts;        /* n_targets                                                                                     */
    const uint32_t *d_piece_off;     /* n_pieces + 1                                                                                  */
    const uint64_t *d_begin;         /* n_pieces                                                                                      */
    const int32_t  *d_len;
    const int32_t  *d_piece_target;
    const uint32_t *d_piece_start;
    const uint32_t *d_words;         /* (n_columns + 15) / 16 + 2                                                                     */
} alga_broken;
typedef struct {
    uint64_t pairs_proper, pairs_spanning, candidate_columns, weak_columns, runs, runs_open, cuts, targets_cut, pieces, max_span, longest_piece;
    uint64_t n50_targets, n50_pieces;
    double   ms_span, ms_cut;        /* device time (HIP events): check + pair pass + scan; flags, compaction, pieces, copy          */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_break_info;
void alga_break_default_params(alga_break_params *p);         /* margin is left 0: the caller sets it                                 */
int  alga_break_placed_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off /* may be NULL */, const alga_placements *pl,
                              const alga_polished *pol /* may be NULL */, const alga_break_params *p, void *hip_stream, alga_broken *out,
                              alga_break_info *info /* may be NULL */);
int  alga_write_broken_fasta_device(alga_engine *e, const alga_broken *brk, const char *path, alga_gfa_info *info /* may be NULL */);

/* ---- contig ends grown with the reads that hang over them (alga_amd/csrc/grow_kernels.hip, engine_grow.hip) ---------------------------------
 * Every stage after the consensus keeps, joins, cuts or orders contigs; none adds a base.  The placement rule has 0 <= p <= len[t] - L, so a
 * read that hangs over a contig end comes out unplaced.  Here the unplaced reads are laid over the contig ends, the columns beyond each end
 * are voted, and each end grows while the vote is clear.  No mates, no joining.  Integers only, free of any order (thread, atomics, sort);
 * tests/grow_checker.py states the rule twice in Python and the device result equals it array for array.  place -> [polish] -> [break ->
 * place] -> grow -> place on the grown targets -> scaffold; a further round is a further call.
 *
 * Inputs: the node set that was placed (twin layout: node 2r + 1 is read r, node 2r its reverse complement), the engine's current placement
 * result `pl` (from either placement call), optionally the current polish `pol` of that placement (the bases are then pol->d_words instead of
 * the column array the placement kept), and alga_grow_params: k 8 .. 31 (default 21), max_mismatches 0 .. 254 (2), max_occ 1 .. 65535 (256),
 * min_anchor k .. 2^20 (63 = k * (max_mismatches + 1): by pigeonhole the seed condition of item 4 then follows from the Hamming bound),
 * min_cover 1 .. 2^31 - 1 (3), min_percent 51 .. 100 (80: above 50, so the winning base is unique), max_grow 1 .. 4096 (64), flags 0,
 * reserved 0; anything else answers ALGA_ERR_INVALID_ARGUMENT.
 *
 *   1. End sequences.  Lmax is the largest len over all nodes (0 where none has a length).  Target t of length n has two ends, e = 2t (left)
 *      and e = 2t + 1 (right); W_e = max(0, min(n, Lmax - 1)).  E_{2t+1} is the last W_e bases of t, E_{2t} the reverse complement of the
 *      first W_e bases of t: in both the contig end is at the right.  A left overhang of a node is by definition the right overhang of its
 *      twin on E_{2t}; both nodes of every read are tried, so every physical alignment appears exactly once.
 *   2. Index.  Position q of E_e is indexed for 0 <= q <= W_e - k; no k-mer spans two end sequences.  occ(x) = the number of indexed
 *      positions over all ends whose k-mer is x.
 *   3. Candidates.  Read r is a CANDIDATE iff its state in `pl` lacks ALGA_PLACE_PLACED and len >= min_anchor + 1.
 *   4. Overhang placements.  For node v of a candidate, of length L, (e, h) is an overhang placement iff, with a = L - h: h >= 1 and
 *      min_anchor <= a <= W_e; mm, the Hamming distance between v[0 .. a) and the last a bases of E_e, is <= max_mismatches; some seed j of v
 *      (bases jk .. jk + k - 1) with (j + 1) k <= a is USABLE (1 <= occ <= max_occ) and equals the corresponding k-mer of E_e exactly.  A
 *      placement is a distinct triple (e, h, strand), strand 0 for node 2r + 1 and 1 for node 2r.
 *   5. Per read.  best = the smallest (mm, e, h, strand); hits = the number of placements with mm == best.mm, saturated at 255.  d_state:
 *      ALGA_GROW_OVERHANGS, ALGA_GROW_VOTES (iff hits == 1), ALGA_GROW_MINUS (best.strand); d_end (-1 where the read does not overhang),
 *      d_over (h, else 0), d_mm, d_hits.
 *   6. Votes.  A voting read with best (e, h) on node v gives base v[a + i] one vote at growth column i of end e, 0 <= i < min(h, max_grow):
 *      d_count[(e * max_grow + i) * 4 + b], uint32.  cover = the sum over b.
 *   7. Decision.  x_e = the number of leading columns i = 0, 1, .. that PASS: cover >= min_cover and 100 * count[w] >= min_percent * cover
 *      (64-bit products), w the base with the largest count; g_e[i] = w.  d_e_stop[e] says why column x_e failed: 0 = no further column or
 *      cover below min_cover (an end without any voter has 0), 1 = the percentage (a disagreement: a branch, a second haplotype),
 *      2 = x_e == max_grow.  d_e_voters[e] = the reads voting at end e.
 *   8. Grown targets.  Target t becomes the reverse complement of g_{2t}[0 .. x_{2t}), then t, then g_{2t+1}[0 .. x_{2t+1}).  A target
 *      shorter than min_anchor, an empty one too, never grows (item 4).  d_left[t] = x_{2t} (where old column 0 now lies), d_right[t] =
 *      x_{2t+1}, d_len[t] the new length, d_col_off [n_targets + 1] their exclusive scan, d_begin[t] = col_off[t], d_words the result's OWN
 *      copy in column space (the polish's layout, (n_columns + 15) / 16 + 2 words, the bits past n_columns zero).  (d_words, d_begin, d_len,
 *      n_targets) is a target set as alga_place_reads_device takes it.  ALGA_ERR_CAPACITY, before anything of that size is allocated: more
 *      than 2^32 - 2 new columns, a new length above 2^31 - 1, 2 * n_targets * max_grow > 2^30, more than 2^32 - 2 bases in the end sequences.
 *   9. Counters (alga_grow_info): candidates, overhanging, voting, multi (= overhanging - voting), hits_saturated; seeds (of the candidates'
 *      nodes: the j with (j + 1) k <= L - 1), seeds_over_max_occ, index_positions; ends_with_voters, ends_grown, bases_added, longest_growth;
 *      stops_cover, stops_percent, stops_max (the ends by d_e_stop: they sum to 2 * n_targets); columns_before, columns_after; n50_before,
 *      n50_after (the scaffold's N50, on the host from lengths read back only when `info` is given); ms_index (check, candidates, end
 *      sequences, keys, sort, directory), ms_place (k_gr_place), ms_build (votes, decision, scan, build) (HIP events), ms_total (wall).
 *  10. Result (alga_grown; engine-owned, valid until the next grow call on `e`: a later placement, polish, break or scaffold call does not
 *      invalidate it, a refused call leaves an earlier result valid: a call writes a second set of buffers and swaps it in at its end).
 *      Refusals, all before anything of the result is written.  On the host, as alga_break_placed_device: `pl` is not the engine's current
 *      placement result, judged by its buffers and all its sizes; nodes->n / 2 != pl.n_reads; `pol` is given but is not the current polish of
 *      this placement.  On the device (k_gr_check, one read-back): the twin property fails or a len > 16 * stride_words; pl.n_columns !=
 *      col_off[n_targets].  The write kernels rely on these checks and on nothing else.
 * Read-backs: the refusal flags with Lmax; the candidate count, the bases and indexed positions of the end sequences (the sort and the
 * directory are sized by them); the new column count (d_words is allocated at its size); the counters.
 *
 * alga_write_grown_fasta_device: one record per target with a length, in target order, `>contig_id=<t>_length=<len>_left=<xl>_right=<xr>`.
 * `grown` must be the engine's current grow result.  ABI stays 7: the calls add. */
#define ALGA_GROW_OVERHANGS 1
#define ALGA_GROW_VOTES     2
#define ALGA_GROW_MINUS     4
typedef struct {
    int32_t k, max_mismatches, max_occ, min_anchor, min_cover, min_percent, max_grow, flags;
    int32_t reserved[4];             /* 0                                                                                             */
} alga_grow_params;
typedef struct {
    int64_t         n_reads, n_targets, max_grow;
    uint64_t        n_columns;       /* of the grown targets: d_col_off[n_targets]                                                    */
    const int32_t  *d_end, *d_over;  /* n_reads                                                                                       */
    const uint8_t  *d_mm, *d_hits, *d_state;
    const uint32_t *d_count;         /* 2 * n_targets * max_grow * 4                                                                  */
    const uint8_t  *d_e_stop;        /* 2 * n_targets                                                                                 */
    const uint32_t *d_e_voters;
    const uint32_t *d_left, *d_right;   /* n_targets                                                                                  */
    const int32_t  *d_len;
    const uint32_t *d_col_off;       /* n_targets + 1                                                                                 */
    const uint64_t *d_begin;         /* n_targets                                                                                     */
    const uint32_t *d_words;         /* (n_columns + 15) / 16 + 2                                                                     */
} alga_grown;
typedef struct {
    uint64_t candidates, overhanging, voting, multi, hits_saturated, seeds, seeds_over_max_occ, index_positions, ends_with_voters, ends_grown, bases_added,
             longest_growth, stops_cover, stops_percent, stops_max, columns_before, columns_after;
    uint64_t n50_before, n50_after;
    double   ms_index, ms_place, ms_build;   /* device time (HIP events)                                                              */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_grow_info;
void alga_grow_default_params(alga_grow_params *p);
int  alga_grow_placed_device(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_polished *pol /* may be NULL */,
                             const alga_grow_params *p, void *hip_stream, alga_grown *out, alga_grow_info *info /* may be NULL */);
int  alga_write_grown_fasta_device(alga_engine *e, const alga_grown *grown, const char *path, alga_gfa_info *info /* may be NULL */);

/* ---- contigs whose ends overlap merged into one sequence (alga_amd/csrc/merge_kernels.hip, engine_merge.hip) ----------------------------------
 * The grow stage stops where two grown ends overlap: they stay two contigs, and the scaffolder can only put min_gap Ns between them.  Here the
 * ends of different targets are compared with each other, ends that choose each other unambiguously are joined, the paths are ordered and
 * oriented, and the merged contigs come out as a new target set with its own copy of the bases.  No reads, no placement, nothing of the
 * engine's state but the stage's own result.  Integers only, free of any order (thread, atomics, sort); tests/merge_checker.py states the rule
 * twice in Python and the device result equals it array for array.  place -> [polish] -> [break -> place] -> grow -> merge -> place on the
 * merged contigs -> scaffold; a further round is a further call.
 *
 * Inputs: a ragged target set as alga_place_reads_device takes it (d_words, d_begin uint64 base index, d_len int32, n_targets = T; a negative
 * length answers ALGA_ERR_INVALID_ARGUMENT, checked on the device before anything is written; a column sum above 2^32 - 2 or more than 2^30
 * targets answers ALGA_ERR_CAPACITY), and alga_merge_params: k 8 .. 31 (default 21), max_mismatches 0 .. 254 (1), max_occ 1 .. 65535 (256),
 * min_overlap k .. max_overlap (42 = k * (max_mismatches + 1): by pigeonhole the seed condition of item 3 then follows from the Hamming bound
 * wherever no seed is over max_occ), max_overlap min_overlap .. min(4096, 64 k) (512; an end has at most 64 seeds: one wave holds them all),
 * flags 0, reserved 0; anything else answers ALGA_ERR_INVALID_ARGUMENT.
 *
 *   1. Ends.  Target t of n bases has two ends, x = 2t (left) and x = 2t + 1 (right); W_x = min(n >> 1, max_overlap).  E_{2t+1} is the last
 *      W_x bases of t, E_{2t} the reverse complement of the first W_x bases: in both the contig end is at the right (the grow stage's
 *      convention).  P_x is the reverse complement of E_x: the first W_x bases read inward from end x.  Because W_x <= n / 2 the two windows of
 *      a target never share a column, an overlap never contains a whole target, and the two overlaps of a doubly joined target never exceed
 *      its length.
 *   2. Index.  Position q of E_x is indexed for 0 <= q <= W_x - k; no k-mer spans two end sequences.  occ(v) = the number of indexed
 *      positions over all ends whose k-mer is v.
 *   3. Overlaps.  (x, y, o) is an overlap at end x iff x and y are ends of DIFFERENT targets; min_overlap <= o <= min(W_x, W_y); mm, the
 *      Hamming distance between P_x[0 .. o) and the last o bases of E_y, is <= max_mismatches; some seed j of P_x (bases jk .. jk + k - 1) with
 *      (j + 1) k <= o is USABLE (1 <= occ <= max_occ) and equals E_y[W_y - o + jk ..) exactly.  mm is the same seen from y; the seed condition
 *      need not be, and that is part of the rule.  An overlap of a target's end with that target's own other end (a ring of one) is no
 *      overlap here and counts nowhere.
 *   4. Per end.  hits[x] = the number of distinct (y, o), saturated at 255; best = the smallest (mm, y, o descending).  d_partner[x] = best.y
 *      (-1 without an overlap), d_olen[x] = best.o, d_mm[x], d_hits[x]; d_end_state: ALGA_MERGE_END_HAS_OVERLAP, ALGA_MERGE_END_AMBIGUOUS
 *      (hits > 1), ALGA_MERGE_END_JOINED, ALGA_MERGE_END_DROPPED_CYCLE.
 *   5. Joins.  Ends x and y are joined iff hits[x] == 1 and hits[y] == 1, partner[x] == y and partner[y] == x, olen[x] == olen[y].  Any second
 *      overlap within the bound stops the join: another partner, or the same partner at another o (a periodic end).  An end has at most one
 *      join.
 *   6. Cycles, paths, orientation, numbering: items 6 and 7 of the scaffold definition.  A cycle is opened at its smallest contig id c: the
 *      join at end 2c is dropped, both of its ends get DROPPED_CYCLE and lose JOINED, it counts in joins_dropped_cycle.  A path starts at its
 *      terminal contig of smaller id, entered at its free end; a contig entered at end 0 has orientation + (d_orient 0), else - (1).  Merged
 *      contigs are numbered by the ascending id of their first contig.  A target of length 0 belongs to none (d_merged = d_rank = -1).
 *   7. Layout.  d_overlap_after[c] = the o of the join by which c is left, 0 for the last contig of a path; d_start[c] = the sum of
 *      len - overlap_after over the contigs before c; the merged length = start[last] + len[last].  A merged length above 2^31 - 1 answers
 *      ALGA_ERR_CAPACITY, before d_words is allocated.
 *   8. Bases.  Column p of merged contig j belongs to the member m of largest rank with start[m] <= p, unless m has a predecessor and
 *      p < start[prev] + len[prev]: then to the predecessor (the overlapped bases are the earlier contig's).  At most two members cover a
 *      column (item 1).  The base is that of the oriented contig at p - start.
 *   9. Result (alga_merged; engine-owned, valid until the next merge call on `e`: no other call invalidates it; kept twice and swapped at the
 *      end of a call, so a refused or failed call leaves the earlier result valid and a call may take its targets from the previous merge
 *      result).  Per end (2T): d_partner, d_olen, d_mm, d_hits, d_end_state.  Per target (T): d_merged, d_rank, d_orient, d_start,
 *      d_overlap_after.  d_m_off [n_merged + 1] and d_m_members [n_members]: the members in rank order.  d_len [n_merged], d_col_off
 *      [n_merged + 1], d_begin [n_merged] (= col_off), d_words: the result's OWN copy in column space (the polish's layout,
 *      (n_columns + 15) / 16 + 2 words, the bits past n_columns zero).  (d_words, d_begin, d_len, n_merged) is a target set as
 *      alga_place_reads_device takes it.
 *  10. Counters (alga_merge_info): ends (those with W_x >= min_overlap: no other can overlap), index_positions, seeds (of those ends: the j
 *      with (j + 1) k <= W_x), seeds_over_max_occ, ends_with_overlap, ends_ambiguous, hits_saturated; joins (the kept ones),
 *      joins_dropped_cycle, join_mismatches (the sum of mm over the kept joins), bases_removed (the sum of their o), longest_overlap (their
 *      largest o); merged, merged_multi, longest, columns_before, columns_after; n50_before, n50_after (the scaffold's N50, on the host from
 *      lengths read back only when `info` is given); ms_index (check, end sequences, keys, sort, directory), ms_overlap (k_mg_overlap),
 *      ms_build (joins, cycles, ranks, layout, scan, build) (HIP events), ms_total (wall).
 * Read-backs: the refusal flag with the column sum; the padded end columns and the indexed positions (the sort and the directory are sized by
 * them); the merged contigs, members and columns (d_words is allocated at its size); the lengths for the N50s.
 *
 * alga_write_merged_fasta_device: one record per merged contig, in id order, `>contig_id=<j>_length=<len>_contigs=<m>`.  `merged` must be the
 * engine's current merge result.  ABI stays 7: the calls add. */
#define ALGA_MERGE_END_HAS_OVERLAP   1
#define ALGA_MERGE_END_AMBIGUOUS     2
#define ALGA_MERGE_END_JOINED        4
#define ALGA_MERGE_END_DROPPED_CYCLE 8
typedef struct {
    int32_t k, max_mismatches, max_occ, min_overlap, max_overlap, flags;
    int32_t reserved[2];             /* 0                                                                                             */
} alga_merge_params;
typedef struct {
    int64_t         n_targets, n_merged, n_members;
    uint64_t        n_columns;       /* of the merged contigs: d_col_off[n_merged]                                                    */
    const int32_t  *d_partner, *d_olen;   /* 2 * n_targets                                                                            */
    const uint8_t  *d_mm, *d_hits, *d_end_state;
    const int32_t  *d_merged, *d_rank;    /* n_targets                                                                                */
    const uint8_t  *d_orient;
    const uint32_t *d_start;
    const int32_t  *d_overlap_after;
    const uint32_t *d_m_off;         /* n_merged + 1                                                                                  */
    const int32_t  *d_m_members;     /* n_members                                                                                     */
    const int32_t  *d_len;           /* n_merged                                                                                      */
    const uint32_t *d_col_off;       /* n_merged + 1                                                                                  */
    const uint64_t *d_begin;         /* n_merged                                                                                      */
    const uint32_t *d_words;         /* (n_columns + 15) / 16 + 2                                                                     */
} alga_merged;
typedef struct {
    uint64_t ends, index_positions, seeds, seeds_over_max_occ, ends_with_overlap, ends_ambiguous, hits_saturated, joins, joins_dropped_cycle, join_mismatches,
             bases_removed, longest_overlap, merged, merged_multi, longest, columns_before, columns_after;
    uint64_t n50_before, n50_after;
    double   ms_index, ms_overlap, ms_build;   /* device time (HIP events)                                                            */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_merge_info;
void alga_merge_default_params(alga_merge_params *p);
int  alga_merge_targets_device(alga_engine *e, const uint32_t *d_words, const uint64_t *d_begin, const int32_t *d_len, int32_t n_targets,
                               const alga_merge_params *p, void *hip_stream, alga_merged *out, alga_merge_info *info /* may be NULL */);
int  alga_write_merged_fasta_device(alga_engine *e, const alga_merged *merged, const char *path, alga_gfa_info *info /* may be NULL */);

/* ---- contigs contained in another contig dropped (alga_amd/csrc/contain_kernels.hip, engine_contain.hip) ---------------------------------------
 * Every stage behind the graph joins contigs or cuts them; none removes a contig that adds nothing: an exact duplicate, a haplotype bubble the
 * parallel-path pass kept, a repeat copy that became a contig of its own, a fragment the grow rounds overtook.  The merge stage cannot see it
 * (its windows are W_x <= n / 2: an overlap never contains a whole target).  Such a contig inflates the FASTA, and every read on the doubled
 * stretch is placed twice: PLACED but not UNIQUE, so it votes in no polish, makes no link and spans nothing.  Here every target is a query: a
 * target whose whole sequence, or its reverse complement, lies inside a longer target within a few substitutions is dropped, and the kept
 * targets come out as a new target set with its own copy of the bases.  No reads, no placement, nothing of the engine's state but the stage's
 * own result.  Integers only, free of any order (thread, atomics, sort); tests/contain_checker.py states the rule twice in Python and the
 * device result equals it array for array.  ... -> grow -> merge -> drop contained -> place on the kept contigs -> scaffold.
 *
 * Inputs: a ragged target set as alga_place_reads_device takes it (d_words, d_begin uint64 base index, any residue mod 16, d_len int32,
 * n_targets = T; a negative length answers ALGA_ERR_INVALID_ARGUMENT, found on the device before anything of the result is written; a column
 * sum above 2^32 - 2, also of the lengths rounded up to 16, or more than 2^30 targets answers ALGA_ERR_CAPACITY), and alga_contain_params: k
 * 8 .. 31 (default 21), max_permille 0 .. 100 (10), max_occ 1 .. 65535 (256), flags 0, reserved 0; anything else answers
 * ALGA_ERR_INVALID_ARGUMENT.
 *
 *   1. Queries.  Target c of n bases has two query strings: Q_c^0 = c and Q_c^1, its reverse complement.  M(n) = floor(n * max_permille /
 *      1000) in 64-bit arithmetic.
 *   2. Index.  Position q of target t is indexed for 0 <= q <= len[t] - k, forward strands only; no k-mer spans two targets.  occ(v) = the
 *      number of indexed positions over all targets whose k-mer is v.
 *   3. Containers.  (h, p, s) is a container of c iff h != c; len[h] > n, or len[h] == n and h < c; 0 <= p and p + n <= len[h]; mm, the
 *      Hamming distance between Q_c^s and h[p .. p + n), is <= M(n); some seed j < S = min(floor(n / k), 64) of Q_c^s (bases jk .. jk + k - 1)
 *      is USABLE (1 <= occ <= max_occ) and equals h[p + jk ..) exactly.  The seed condition is part of the rule, as in merge.  A target with
 *      n < k has no container.  (len descending, id ascending) is a strict order: containers form no cycle, and the first target of that
 *      order in any group of near-duplicates is never contained.
 *   4. Per target.  hits[c] = the number of distinct (h, p, s), saturated at 255; best = the smallest (mm, h, p, s).  d_host[c] = best.h (-1
 *      without a container), d_host_pos = best.p, d_host_orient = best.s, d_mm (uint32), d_hits (uint8), d_state: ALGA_CONTAIN_CONTAINED,
 *      ALGA_CONTAIN_MINUS (best.s == 1), ALGA_CONTAIN_AMBIGUOUS (hits > 1), ALGA_CONTAIN_DUPLICATE (len[host] == n), ALGA_CONTAIN_KEPT.  A
 *      target is KEPT iff n > 0 and it has no container.  A target of length 0 is neither kept nor contained (state 0, new id -1).
 *   5. Roots.  Following d_host from c ends at a kept target d_root[c]; a kept target is its own root at position 0 with orientation 0; a
 *      target of length 0 has d_root -1.  Position and orientation compose: let c lie in h at (p, s) and h in g at (p', s'); with s' = 0, c
 *      lies in g at p' + p with orientation s; with s' = 1, at p' + len[h] - p - n with orientation s xor 1.  d_root_pos and d_root_orient
 *      hold the result.  The Hamming distance against the ROOT's bases is NOT bounded by M: every step of the walk may add its own
 *      mismatches.  d_absorbed[r] (per input target) = the number of contained targets whose root is r.
 *   6. Result (alga_kept; engine-owned, valid until the next alga_drop_contained_device call on `e`: no other call invalidates it; kept
 *      twice and swapped at the end of a call, so a refused or failed call leaves the earlier result valid and a call may take its targets
 *      from the result before).  Kept targets are numbered by ascending old id: d_new[c] (T; -1 where the target is not kept), d_old[j]
 *      (n_kept).  d_len [n_kept], d_col_off [n_kept + 1], d_begin [n_kept] (= col_off), d_words: the result's OWN copy in column space (the
 *      polish's layout, (n_columns + 15) / 16 + 2 words, the bits past n_columns zero).  (d_words, d_begin, d_len, n_kept) is a target set as
 *      alga_place_reads_device takes it.
 *   7. Counters (alga_contain_info): queries (targets with n >= k), index_positions, seeds (S of every (c, s): twice per query),
 *      seeds_over_max_occ (of those), candidates (distinct (c, h, p, s) that pass item 3 except for the Hamming bound), contained,
 *      contained_minus, duplicates, ambiguous, hits_saturated (all four over the contained targets), kept, bases_removed (the bases of the
 *      contained targets), longest_contained, columns_before, columns_after; n50_before, n50_after (the scaffold's N50, on the host from
 *      lengths read back only when `info` is given); ms_index (check, column arrays, keys, sort, directory), ms_contain (k_ct_contain),
 *      ms_build (decision, roots, scans, build) (HIP events), ms_total (wall).
 * Read-backs: the refusal flag with the column sums and the indexed positions (the column arrays, the sort and the directory are sized by
 * them); the contained and kept targets and their columns (the jumps are skipped where nothing is contained, d_words is allocated at its
 * size); the lengths for the N50s.  The seed index is built in the engine's one index workspace (option "place_dir_bits" as for the
 * placement).
 *
 * alga_write_kept_fasta_device: one record per kept target, in new-id order, `>contig_id=<j>_length=<len>_absorbed=<m>`.  `kept` must be the
 * engine's current containment result.  ABI stays 7: the calls add. */
#define ALGA_CONTAIN_CONTAINED 1
#define ALGA_CONTAIN_MINUS     2
#define ALGA_CONTAIN_AMBIGUOUS 4
#define ALGA_CONTAIN_DUPLICATE 8
#define ALGA_CONTAIN_KEPT      16
typedef struct {
    int32_t k, max_permille, max_occ, flags;
    int32_t reserved[2];             /* 0                                                                                             */
} alga_contain_params;
typedef struct {
    int64_t         n_targets, n_kept;
    uint64_t        n_columns;       /* of the kept targets: d_col_off[n_kept]                                                        */
    const int32_t  *d_host, *d_host_pos;  /* n_targets                                                                                */
    const uint8_t  *d_host_orient;
    const uint32_t *d_mm;
    const uint8_t  *d_hits, *d_state;
    const int32_t  *d_root, *d_root_pos;
    const uint8_t  *d_root_orient;
    const uint32_t *d_absorbed;
    const int32_t  *d_new;
    const int32_t  *d_old;           /* n_kept                                                                                        */
    const int32_t  *d_len;           /* n_kept                                                                                        */
    const uint32_t *d_col_off;       /* n_kept + 1                                                                                    */
    const uint64_t *d_begin;         /* n_kept                                                                                        */
    const uint32_t *d_words;         /* (n_columns + 15) / 16 + 2                                                                     */
} alga_kept;
typedef struct {
    uint64_t queries, index_positions, seeds, seeds_over_max_occ, candidates, contained, contained_minus, duplicates, ambiguous, hits_saturated, kept, bases_removed,
             longest_contained, columns_before, columns_after;
    uint64_t n50_before, n50_after;
    double   ms_index, ms_contain, ms_build;   /* device time (HIP events)                                                            */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_contain_info;
void alga_contain_default_params(alga_contain_params *p);
int  alga_drop_contained_device(alga_engine *e, const uint32_t *d_words, const uint64_t *d_begin, const int32_t *d_len, int32_t n_targets,
                                const alga_contain_params *p, void *hip_stream, alga_kept *out, alga_contain_info *info /* may be NULL */);
int  alga_write_kept_fasta_device(alga_engine *e, const alga_kept *kept, const char *path, alga_gfa_info *info /* may be NULL */);

/* ---- scaffold joins whose contig ends overlap stitched into one sequence (alga_amd/csrc/stitch_kernels.hip, engine_stitch.hip) ---------------
 * The scaffolder bridges two contigs with max(gap, min_gap) Ns, also where the gap estimate is negative and the two ends share bases.  The
 * merge stage in front of it compares all ends at once through a seed index, so it refuses an overlap under k * (max_mismatches + 1) bases, an
 * end with two overlaps and an overlap with more than one mismatch.  After the scaffolder the mates have made that choice: a bundle with state
 * JOIN names exactly two ends and a gap.  Here those two ends alone are compared, at every overlap length, with no index and no seed
 * condition; the entries with exactly one admissible overlap are stitched, and everything behind that decision (cycles, ranking, layout, the
 * bases, FASTA) is the merge stage's.  No reads, no voting, nothing of the engine's state but the stage's own result.  Integers only, free
 * of any order (thread, atomics); tests/stitch_checker.py states the rule twice in Python and the device result equals it array for array.
 * ... -> place -> scaffold -> stitch -> place on the stitched contigs -> scaffold; a further round is a further call.
 *
 * Inputs: a ragged target set as alga_place_reads_device takes it (d_words, d_begin uint64 base index, d_len int32, n_targets = T); an entry
 * list of J entries: d_j_a, d_j_b (uint32 ends, x = 2t left, 2t + 1 right), d_j_gap (int32), d_j_state (uint8, may be NULL) -- exactly
 * alga_scaffolds.d_b_a / d_b_b / d_b_gap / d_b_state / n_bundles; and alga_stitch_params: max_mismatches 0 .. 254 (default 2), min_overlap
 * 8 .. max_overlap (16: with at most 2 mismatches a random pair of 16-mers matches with probability (1 + 48 + 1080) / 4^16 = 2.6e-7 per overlap
 * length, and the sum over the longer lengths is dominated by that term), max_overlap min_overlap .. 4096 (512), slack 0 .. 2^20 (2^20: excludes
 * nothing in practice), flags 0, reserved 0; anything else answers ALGA_ERR_INVALID_ARGUMENT.
 *
 *   1. Selected entries.  Entry j is SELECTED iff d_j_state is NULL, or state & ALGA_SCAFFOLD_BUNDLE_JOIN and not state &
 *      ALGA_SCAFFOLD_BUNDLE_DROPPED_CYCLE.  Nothing of an unselected entry is read or checked.
 *   2. Refusals, all decided on the device before anything of the result is written, with one read-back, ALGA_ERR_INVALID_ARGUMENT: a
 *      negative target length; a selected entry with a >= 2T or b >= 2T, or with a >> 1 == b >> 1; an end named by more than one selected
 *      entry.  ALGA_ERR_CAPACITY as in merge: a column sum above 2^32 - 2, more than 2^30 targets, a stitched length above 2^31 - 1; also
 *      J > 2^31 - 1.
 *   3. Ends.  Target t of n bases has two ends, x = 2t (left) and x = 2t + 1 (right); W_x = min(n >> 1, max_overlap).  E_{2t+1} is the last
 *      W_x bases of t, E_{2t} the reverse complement of the first W_x bases: in both the contig end is at the right.  P_x is the reverse
 *      complement of E_x: the first W_x bases read inward from end x.  (Item 1 of the merge definition.)
 *   4. Overlaps of a selected entry (a, b, gap).  o is a CANDIDATE iff min_overlap <= o <= min(W_a, W_b) and mm(o) <= max_mismatches, mm(o) the
 *      Hamming distance between P_a[0 .. o) and the last o bases of E_b; mm is the same with a and b exchanged.  No seed condition, no index:
 *      every o is compared.  A candidate is ADMISSIBLE iff |gap + o| <= slack, in 64-bit arithmetic.  hits = the number of admissible
 *      candidates, saturated at 255; best = the smallest (mm, o descending) among them.  Per entry: d_j_olen = best.o (0 without), d_j_mm,
 *      d_j_hits, d_j_state: ALGA_STITCH_SELECTED, ALGA_STITCH_HAS_OVERLAP, ALGA_STITCH_AMBIGUOUS (hits > 1), ALGA_STITCH_STITCHED,
 *      ALGA_STITCH_DROPPED_CYCLE.  Unselected entries are all 0.
 *   5. Stitches.  A selected entry is STITCHED iff hits == 1.  A second admissible overlap length (a periodic end) stops it; a smaller slack
 *      is the caller's way to decide such an end.
 *   6. Cycles, paths, orientation, numbering, layout, bases: items 6, 7 and 8 of the merge definition with "join" read as "stitched entry".
 *      A raw entry list may hold a ring (the scaffolder's own joins cannot: it drops them).  A cycle is opened at its smallest contig id c:
 *      the stitch at end 2c is dropped, its entry gets DROPPED_CYCLE and loses STITCHED.  The overlapped bases are the earlier contig's.
 *   7. Result (alga_stitched; engine-owned, valid until the next stitch call on `e`: no other call invalidates it; kept twice and swapped at
 *      the end of a call, so a refused or failed call leaves the earlier result valid and a call may take its targets from the previous
 *      result).  Per entry (J): d_j_olen, d_j_mm, d_j_hits, d_j_state.  Per end (2T): d_end_entry, the selected entry that names the end, -1
 *      without.  Per target (T): d_stitched, d_rank, d_orient, d_start, d_overlap_after.  d_s_off [n_stitched + 1] and d_s_members
 *      [n_members].  d_len [n_stitched], d_col_off [n_stitched + 1], d_begin [n_stitched] (= col_off), d_words: the result's OWN copy in column
 *      space (the polish's layout, (n_columns + 15) / 16 + 2 words, the bits past n_columns zero).  (d_words, d_begin, d_len, n_stitched) is a
 *      target set as the placement and the merge take it.
 *   8. Counters (alga_stitch_info): entries, selected, with_overlap, ambiguous, hits_saturated, candidates_outside_slack (the (j, o) that are
 *      candidates but not admissible), stitched (the kept ones), dropped_cycle, join_mismatches, bases_removed, longest_overlap (over the kept
 *      ones); contigs, contigs_multi, longest, columns_before, columns_after; n50_before, n50_after (on the host from lengths read back only
 *      when `info` is given); ms_overlap (k_st_overlap), ms_build (joins, cycles, ranks, layout, scan, build) (HIP events), ms_total (wall).
 * Read-backs: the refusal flags with the column sum; the stitched contigs, members and columns (d_words is allocated at its size); the lengths
 * for the N50s.
 *
 * alga_stitch_scaffolds_device: the same on the engine's current placement and scaffold result.  The bases come from where
 * alga_write_scaffold_fasta_device takes them (the column array the placement kept, or pol->d_words), begin = col_off, the lengths from
 * col_off, the entries are the scaffold result's bundles; it refuses exactly what alga_write_scaffold_fasta_device refuses.
 * alga_write_stitched_fasta_device: one record per stitched contig, in id order, `>contig_id=<j>_length=<len>_contigs=<m>`.  `stitched` must be
 * the engine's current stitch result.  ABI stays 7: the calls add. */
#define ALGA_STITCH_SELECTED      1    /* bits of d_j_state                                                                           */
#define ALGA_STITCH_HAS_OVERLAP   2
#define ALGA_STITCH_AMBIGUOUS     4
#define ALGA_STITCH_STITCHED      8
#define ALGA_STITCH_DROPPED_CYCLE 16
typedef struct {
    int32_t max_mismatches, min_overlap, max_overlap, slack, flags;
    int32_t reserved[3];             /* 0                                                                                             */
} alga_stitch_params;
typedef struct {
    int64_t         n_targets, n_entries, n_stitched, n_members;
    uint64_t        n_columns;       /* of the stitched contigs: d_col_off[n_stitched]                                                */
    const int32_t  *d_j_olen;        /* n_entries                                                                                     */
    const uint8_t  *d_j_mm, *d_j_hits, *d_j_state;
    const int32_t  *d_end_entry;     /* 2 * n_targets                                                                                 */
    const int32_t  *d_stitched, *d_rank;  /* n_targets                                                                                */
    const uint8_t  *d_orient;
    const uint32_t *d_start;
    const int32_t  *d_overlap_after;
    const uint32_t *d_s_off;         /* n_stitched + 1                                                                                */
    const int32_t  *d_s_members;     /* n_members                                                                                     */
    const int32_t  *d_len;           /* n_stitched                                                                                    */
    const uint32_t *d_col_off;       /* n_stitched + 1                                                                                */
    const uint64_t *d_begin;         /* n_stitched                                                                                    */
    const uint32_t *d_words;         /* (n_columns + 15) / 16 + 2                                                                     */
} alga_stitched;
typedef struct {
    uint64_t entries, selected, with_overlap, ambiguous, hits_saturated, candidates_outside_slack, stitched, dropped_cycle, join_mismatches,
             bases_removed, longest_overlap, contigs, contigs_multi, longest, columns_before, columns_after;
    uint64_t n50_before, n50_after;
    double   ms_overlap, ms_build;   /* device time (HIP events)                                                                      */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_stitch_info;
void alga_stitch_default_params(alga_stitch_params *p);
int  alga_stitch_targets_device(alga_engine *e, const uint32_t *d_words, const uint64_t *d_begin, const int32_t *d_len, int32_t n_targets,
                                const uint32_t *d_j_a, const uint32_t *d_j_b, const int32_t *d_j_gap, const uint8_t *d_j_state /* may be NULL */,
                                int64_t n_entries, const alga_stitch_params *p, void *hip_stream, alga_stitched *out,
                                alga_stitch_info *info /* may be NULL */);
int  alga_stitch_scaffolds_device(alga_engine *e, const alga_placements *pl, const alga_scaffolds *scaf, const alga_polished *pol /* may be NULL */,
                                  const alga_stitch_params *p, void *hip_stream, alga_stitched *out, alga_stitch_info *info /* may be NULL */);
int  alga_write_stitched_fasta_device(alga_engine *e, const alga_stitched *stitched, const char *path, alga_gfa_info *info /* may be NULL */);

/* ---- gapped placement: the unplaced reads laid with indels, CIGARs (alga_amd/csrc/gapped_kernels.hip, engine_gapped.hip) -----------------
 * alga_place_reads_device verifies by Hamming distance, so a read with one inserted or deleted base is unplaced.  This second pass lays the
 * reads the Hamming pass left unplaced onto the same targets by edit distance, reports where they lie and how, and adds their cover.  Integers
 * only, free of any order (thread, sort); tests/gapped_checker.py states the rule twice in Python and the device result equals it array for
 * array.
 *
 * Inputs: the node set in twin layout and the ragged target set exactly as alga_place_reads_device takes them; the engine's current placement
 * result `pl` on those targets; alga_gapped_params: k 8 .. 31 (default 21), max_edits E 1 .. 15 (6), max_occ 1 .. 65535 (256), flags 0;
 * anything else answers ALGA_ERR_INVALID_ARGUMENT.
 *
 *   1. Who takes part.  Read r takes part iff pl.d_state[r] lacks ALGA_PLACE_PLACED, len >= k and len <= ALGA_GAPPED_MAX_READ (1024).  A read
 *      above the cap is counted in skipped_long; a read the Hamming pass placed is never touched.
 *   2. Index and seeds: rules 1 and 2 of the placement.  Position (t, q) is indexed for q + k <= len[t]; node v of length L has
 *      S = floor(L / k) seeds, seed j = bases jk .. jk + k - 1, USABLE iff 1 <= occ <= max_occ.  Both nodes of the read (both strands) are tried.
 *   3. Candidates.  Usable seed j of node v equal to the k-mer at indexed position (t, q) is a candidate (j, t, q).  It COUNTS iff no usable
 *      seed j' < j of v equals t[q - (j - j') k .. + k) (the same diagonal, inside t).
 *   4. Distance.  Unit costs: substitution, insertion (a read base alone), deletion (a target base alone).  The alignment passes through the
 *      seed, is global in the read and free-ended in the target, inside target t only.  Right part: v[jk + k .. L) against t[q + k ..);
 *      left part: v[0 .. jk) reversed against t[0 .. q) reversed.  For a part with n read bases and avail target bases, D[i][c] is the usual
 *      edit-distance table from (0, 0) (D[0][c] = c, D[i][0] = i).  The part's end is the column c in [max(0, n - E), min(avail, n + E)]
 *      with the smallest D[n][c]; ties go to the smallest |c - n|, then the smaller c; no such c: not a placement.  d = d_left + d_right; the
 *      candidate is a gapped placement iff d <= E.  Its first column is p = q - c_left, its end (exclusive) e = q + k + c_right.  A read
 *      hanging over a target end by at most E bases is thereby placed with insertions at the edge; there are no clipped ends.
 *   5. Canonical script.  Each part is traced back from its end cell to (0, 0); at every cell it takes the first of diagonal, up (insertion),
 *      left (deletion) whose predecessor attains the value (row 0 goes left, column 0 goes up).  The CIGAR is the left part (reversed back),
 *      k M for the seed, the right part, equal neighbouring ops merged; ops ALGA_CIGAR_M (match or substitution), _I, _D; at most 2 E + 1
 *      runs.  Banding to |c - i| <= E changes no decision: a value <= E is exact inside the band (a path of cost <= E leaves diagonal 0 by at
 *      most E), a banded value > E says the true one is > E, the trace visits only cells <= d <= E, and a predecessor that attains such a
 *      value is itself <= E.  The checker asserts banded == full on every case.
 *   6. Per read.  best = the smallest (d, strand, t, p, e) over its counting candidates that are placements, with + < - (the strand before the
 *      position, so that uniqueness follows from a minimum and a maximum); among candidates equal in all five the one with the smallest
 *      (j, q) gives the script.  ALGA_GAPPED_UNIQUE iff every such candidate with d == best.d has best's strand and target and
 *      p <= best.p + E.  State bits ALGA_GAPPED_PLACED, _UNIQUE, _MINUS, _INDEL (the script has an I or a D).  Per read, with these defaults
 *      where it is not placed: d_target (-1), d_pos (-1), d_end (-1), d_edits (0), d_state (0).  d_cigar_off has n_reads + 1 entries (the
 *      exclusive scan of the run counts, 0 runs where not placed); d_cigar is uint32 len << 2 | op, n_cigar = d_cigar_off[n_reads] entries.
 *   7. Cover.  A gapped read COUNTS iff it is UNIQUE.  d_cover[c] = pl.d_cover[c] + the counting gapped reads whose [p, e) contains c: deleted
 *      columns count as covered, inserted bases cover nothing.  Per target, the gapped reads alone: d_t_reads, d_t_bases (the sum of
 *      e - p), d_t_edits.
 *   8. Counters (alga_gapped_info): tried (the reads that take part), skipped_long, placed, unique, with_indel, edits (the sum of d over the
 *      placed), insertions, deletions (inserted / deleted bases of their scripts), candidates (those that count, rule 3), seeds,
 *      seeds_over_max_occ (of the reads that take part, both strands); ms_index, ms_place, ms_trace, ms_depth (HIP events), ms_total (wall).
 *   9. Refusals, all before anything of the result is written (ALGA_ERR_INVALID_ARGUMENT): `pl` is not the engine's current placement result;
 *      nodes->n / 2 != pl.n_reads; n_targets != pl.n_targets; on the device: a target length that differs from pl's col_off (so n_columns
 *      agrees), the twin property of the node set.
 * The result (alga_gapped) is engine-owned, valid until the next gapped call on `e`; a refused call leaves an earlier result valid; `pl` and
 * every other result stay valid.  The seed index is built in the engine's one index workspace (option "place_dir_bits" as for the placement).
 * Read-backs: the refusal flags with the participating reads; the number of runs (d_cigar is allocated at its size); the counters.
 *
 * alga_write_gapped_tsv_device: one line per gapped-placed read in read order, `read target pos end strand edits unique cigar` separated by
 * tabs (strand + or -, unique 0 or 1, the CIGAR as text, for example 57M1D93M), formatted on the device.  `gapped` must be the engine's
 * current gapped result.  ABI stays 7: the calls add. */
#define ALGA_GAPPED_MAX_READ 1024
#define ALGA_GAPPED_PLACED 1         /* bits of alga_gapped.d_state                                                                    */
#define ALGA_GAPPED_UNIQUE 2
#define ALGA_GAPPED_MINUS  4
#define ALGA_GAPPED_INDEL  8
#define ALGA_CIGAR_M 0               /* the low two bits of a d_cigar entry                                                            */
#define ALGA_CIGAR_I 1
#define ALGA_CIGAR_D 2
typedef struct {
    int32_t k, max_edits, max_occ, flags;
    int32_t reserved[4];             /* 0                                                                                             */
} alga_gapped_params;
typedef struct {
    int64_t         n_reads;         /* n / 2                                                                                         */
    int64_t         n_targets;
    uint64_t        n_columns;       /* pl.n_columns                                                                                  */
    uint64_t        n_cigar;         /* d_cigar_off[n_reads]                                                                          */
    const int32_t  *d_target, *d_pos, *d_end;        /* n_reads                                                                       */
    const uint8_t  *d_edits, *d_state;               /* n_reads                                                                       */
    const uint32_t *d_cigar_off;     /* n_reads + 1                                                                                   */
    const uint32_t *d_cigar;         /* n_cigar                                                                                       */
    const uint32_t *d_cover;         /* n_columns                                                                                     */
    const uint64_t *d_t_reads, *d_t_bases, *d_t_edits;   /* n_targets                                                                 */
} alga_gapped;
typedef struct {
    uint64_t tried, skipped_long, placed, unique, with_indel, edits, insertions, deletions, candidates, seeds, seeds_over_max_occ;
    double   ms_index, ms_place, ms_trace, ms_depth; /* device time (HIP events): list + gather + index, the score kernel, trace + CIGAR, depth */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_gapped_info;
void alga_gapped_default_params(alga_gapped_params *p);
int  alga_place_gapped_device(alga_engine *e, const alga_nodes *nodes, const uint32_t *d_words, const uint64_t *d_begin, const int32_t *d_len,
                              int32_t n_targets, const alga_placements *pl, const alga_gapped_params *p, void *hip_stream, alga_gapped *out,
                              alga_gapped_info *info /* may be NULL */);
int  alga_write_gapped_tsv_device(alga_engine *e, const alga_gapped *gapped, const char *path, alga_gfa_info *info /* may be NULL */);

/* ---- polish with the gapped reads: indel votes, targets that change length (alga_amd/csrc/ipolish_kernels.hip, engine_ipolish.hip) --------
 * alga_polish_placed_device repairs substitutions only: at a column where a target has a base too many or too few the Hamming pass places no
 * read.  Here the Hamming-placed and the gapped reads vote together, on every column (a base, or "delete this column") and on every slot
 * between two columns ("insert these bases"); the result is a new target set whose lengths may differ.  Integers only, free of any order
 * (thread, sort); tests/ipolish_checker.py states the rule twice in Python and the device result equals it array for array.
 *
 * Inputs: the node set that was placed (twin layout); `pl`, the engine's current placement result; `gp`, the engine's current gapped result,
 * made from that placement; alga_ipolish_params: min_cover 1 .. 2^31 - 1 (default 3), min_percent 1 .. 100 (60), max_ins 1 .. 13 (6), flags
 * 0 or ALGA_IPOLISH_COUNTS, reserved 0; anything else answers ALGA_ERR_INVALID_ARGUMENT.  The current bases `t` come from the column array
 * the placement call kept (column g = col_off[target] + index), never from the caller.
 *
 *   1. Voters.  H voter: read r with ALGA_PLACE_UNIQUE in pl; node v = 2r if MINUS else 2r + 1; its script is one M run of len[v] columns
 *      from column col_off[target] + pos.  G voter: read r with ALGA_GAPPED_UNIQUE in gp; v = 2r if ALGA_GAPPED_MINUS else 2r + 1; its script
 *      is gp.d_cigar[d_cigar_off[r] .. d_cigar_off[r + 1]) from column col_off[gp.d_target[r]] + gp.d_pos[r] on, in target orientation over the
 *      bases of v.  The two sets are disjoint (the gapped pass touches only reads the Hamming pass left unplaced).
 *   2. Normalisation of a G script.  This is a DEFINITION of where a gap votes, not a claim that the result is the leftmost form.  Every gap
 *      run that is neither the first nor the last run of its script is shifted left; the shifts are found on the script's ORIGINAL runs.  m =
 *      the length of the M run directly in front of the gap, 0 if that run is not M.  A D run over columns [c, c + n) moves by the largest
 *      s <= m with t[c - j] == t[c + n - j] for all 1 <= j <= s.  An I run of read bases v[a .. a + n) before column c moves by the largest
 *      s <= m with v[a - j] == v[a + n - j] for all 1 <= j <= s and becomes v[a - s .. a - s + n) before column c - s (the string rotates).
 *      The M run in front shrinks by s; the s cells the gap passed over are M cells directly behind it (they join a following M run; behind
 *      a gap followed by another gap they stand between the two).  A gap never leaves its own M run, so the events keep their order; [p, e)
 *      and the read's bases are unchanged.
 *   3. Votes, after rule 2.  An M cell: one vote for the read base at its column, count[g][b].  A D cell: one vote into del[g].  An inner I run
 *      of n <= max_ins bases before column c: one vote for (n, string) at slot c, key n << 26 | string, the first base in the highest used
 *      bits.  An inner I run longer than max_ins adds only to long_ins[c].  An I run that is the first or last run of its script votes nothing
 *      (an overhang over a target end: the grow stage's business).  A voter over [p, e) adds one to span[c] for every slot c with p < c < e.
 *      Slot c is the place between columns c - 1 and c of one target; a target's first column has no slot.
 *      cover[g] = sum_b count[g][b] + del[g] (== gp.d_cover[g] where the placement's depth counts the UNIQUE reads).
 *   4. Column decision.  Candidates A, C, G, T and `-` (votes del[g]).  The winner w has the most votes; a tie goes to cur if it is among the
 *      tied, else to the smallest of A < C < G < T < `-`.  The column CHANGES iff w != cur, cover >= min_cover and 100 * votes[w] >=
 *      min_percent * cover (64-bit products): substituted if w is a base, deleted if w is `-`.  AMBIGUOUS iff w != cur, cover >= min_cover and
 *      the percentage test fails.  With no G voter this is rule 3 of the polish, bit for bit.
 *   5. Slot decision.  The winner w is the (n, string) with the most votes at the slot, a tie goes to the smallest key.  INSERTED iff
 *      span[c] >= min_cover and 100 * votes[w] >= min_percent * span[c].  AMBIGUOUS iff span[c] >= min_cover, not inserted, and 100 * (all
 *      insertion votes at c, the long ones included) >= min_percent * span[c].  Column and slot decisions are independent.
 *   6. New targets.  Target t from its columns in order: first the string of the column's slot if INSERTED, then the column unless DELETED,
 *      with its new base if substituted.  Result (alga_ipolished; engine-owned, double-buffered: a call writes the set that is not the current
 *      one and swaps it in at its end, so a call that fails anywhere leaves the earlier result valid): n_targets, n_columns_before,
 *      n_columns; d_len, d_col_off [T + 1], d_begin (== col_off), d_words (the result's own copy, 16 columns a word, two zero words of padding,
 *      the bits past n_columns zero) -- (d_words, d_begin, d_len, n_targets) is a target set as alga_place_reads_device takes it;
 *      d_new_col [n_columns_before + 1]: the new column of each old column (a deleted column: the index of the next kept one; the last entry
 *      n_columns); the events, n_events, ascending by old column, an insertion before the column's own event: d_ev_col, d_ev_kind (0 S, 1 I,
 *      2 D), d_ev_len (S 1, D 1, I n), d_ev_bases (S old | new << 2, D old, I the string), d_ev_votes, d_ev_cover (cover, for I span); per
 *      target d_t_subs, d_t_dels, d_t_ins_bases, d_t_ambiguous (columns and slots); with ALGA_IPOLISH_COUNTS d_counts uint32
 *      [5 * n_columns_before] (A C G T - per column) and d_span uint32 [n_columns_before], else both NULL.  ALGA_ERR_CAPACITY where the new
 *      targets hold more than 2^32 - 2 bases or one is longer than 2^31 - 1.
 *   7. Counters (alga_ipolish_info): columns, voters_hamming, voters_gapped, votes (M cells), del_votes (D cells), ins_votes (inner I runs
 *      that vote), ins_too_long, ins_edge (runs), shifted_runs, shifted_bases (sum of s), voted_columns (cover >= min_cover), substituted,
 *      deleted, inserted_slots, inserted_bases, ambiguous_columns, ambiguous_slots, columns_after, max_cover; ms_votes, ms_inserts, ms_build
 *      (HIP events), ms_total (wall).
 *   8. Refusals, all before anything of the result is written (ALGA_ERR_INVALID_ARGUMENT).  Host: `pl` is not the current placement; `gp` is
 *      not the engine's current gapped result or was made from an earlier placement; nodes->n / 2 != pl.n_reads; the parameters.  Device, one
 *      read-back: the twin property; an H voter's length above the stride, target out of range, pos < 0, pos + len > len[target]; a G
 *      voter whose script's read length differs from len[v], whose column length differs from end - pos, that does not lie inside its target,
 *      or that has no run, more than 31 runs or an op that is none of M, I, D.  The vote kernels rely on these checks and on nothing else.
 * Read-backs: the checks with the insertion votes; the new column and event counts; the counters.
 *
 * alga_write_ipolished_fasta_device: `>contig_id=<t>_length=<len>_subs=<s>_ins=<i>_dels=<d>` and the new sequence, one record per target with
 * a length.  alga_write_ipolish_events_tsv_device: one line per event, `contig pos kind len old new votes cover` separated by tabs; pos is the
 * OLD position inside the contig, kind S / I / D, old and new as letters with `-` where there is none (I: old `-`, new the string; D: new `-`).
 * Both are formatted on the device; `ipol` must be the engine's current result of this stage.  ABI stays 7: the calls add. */
#define ALGA_IPOLISH_COUNTS 1        /* alga_ipolish_params.flags                                                                      */
#define ALGA_IPOLISH_MAX_INS 13
typedef struct {
    int32_t min_cover, min_percent, max_ins, flags;
    int32_t reserved[4];             /* 0                                                                                             */
} alga_ipolish_params;
typedef struct {
    int64_t         n_targets;
    uint64_t        n_columns_before, n_columns, n_events;
    const int32_t  *d_len;           /* n_targets                                                                                     */
    const uint32_t *d_col_off;       /* n_targets + 1                                                                                 */
    const uint64_t *d_begin;         /* n_targets                                                                                     */
    const uint32_t *d_words;         /* (n_columns + 15) / 16 + 2                                                                     */
    const uint32_t *d_new_col;       /* n_columns_before + 1                                                                          */
    const uint32_t *d_ev_col;        /* n_events, as are the next five                                                                */
    const uint8_t  *d_ev_kind, *d_ev_len;
    const uint32_t *d_ev_bases, *d_ev_votes, *d_ev_cover;
    const uint64_t *d_t_subs, *d_t_dels, *d_t_ins_bases, *d_t_ambiguous;   /* n_targets                                               */
    const uint32_t *d_counts;        /* 5 * n_columns_before, or NULL                                                                 */
    const uint32_t *d_span;          /* n_columns_before, or NULL                                                                     */
} alga_ipolished;
typedef struct {
    uint64_t columns, voters_hamming, voters_gapped, votes, del_votes, ins_votes, ins_too_long, ins_edge, shifted_runs, shifted_bases, voted_columns, substituted,
             deleted, inserted_slots, inserted_bases, ambiguous_columns, ambiguous_slots, columns_after, max_cover;
    double   ms_votes, ms_inserts, ms_build;         /* device time (HIP events): checks' follow-up + all votes + span, the insertion votes' sorts and winners, decision + build */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_ipolish_info;
void alga_ipolish_default_params(alga_ipolish_params *p);
int  alga_polish_indels_device(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_gapped *gp, const alga_ipolish_params *p,
                               void *hip_stream, alga_ipolished *out, alga_ipolish_info *info /* may be NULL */);
int  alga_write_ipolished_fasta_device(alga_engine *e, const alga_ipolished *ipol, const char *path, alga_gfa_info *info /* may be NULL */);
int  alga_write_ipolish_events_tsv_device(alga_engine *e, const alga_ipolished *ipol, const char *path, alga_gfa_info *info /* may be NULL */);

/* ---- SAM output and pair calls over both placement passes (alga_amd/csrc/sam_kernels.hip, engine_sam.hip) ---------------------------------
 * The Hamming placement judges its pairs by pos + len; a pair with a gapped mate stays pairs_not_unique there.  alga_judge_pairs_device judges
 * every pair again over both passes, with the ends the gapped pass reports, and gives every read its SAM FLAG and TLEN;
 * alga_write_sam_device writes all reads as SAM, formatted on the device.  Integers only, free of any order; tests/sam_checker.py states both
 * in Python and the device result equals it array for array and byte for byte.  No other result is touched.
 *
 * Inputs: the node set that was placed (twin layout) and its pair_off (NULL = no pairs); `pl`, the engine's current placement result; `gp`,
 * the engine's current gapped result made from `pl`, or NULL: the Hamming pass alone.  alga_pair_params: max_insert 1 .. 2^20 (1000), flags 0,
 * reserved 0.
 *
 *   1. The combined view of read r, L = len[2r + 1].  H iff pl.d_state[r] has ALGA_PLACE_PLACED: target and pos from pl, end = pos + L, strand
 *      from ALGA_PLACE_MINUS, nm = d_mm, unique = ALGA_PLACE_UNIQUE, the script is the one run `L M`.  Otherwise G iff gp is given and
 *      gp.d_state[r] has ALGA_GAPPED_PLACED: target, pos, end, strand, nm = d_edits, unique and the runs from gp.  Otherwise unplaced.  A read
 *      is LIVE iff L >= 1 (a removed read, len -1, is not).
 *   2. Pairs.  The pair is (r, r + 1) where pair_off[2r + 1] == 1; the smaller index judges.  A pair is LIVE iff both reads are live; only live
 *      pairs are counted, a read of a pair that is not live is a single read.  Not both unique: pairs_not_unique.  Different targets:
 *      pairs_split.  Same strand: pairs_improper.  Otherwise with a, ea the pos and end of the `+` read and b, eb of the `-` read the pair is
 *      PROPER iff a <= b, ea <= eb and insert = eb - a <= max_insert; a proper pair does d_insert_hist[insert]++ (max_insert + 1 bins);
 *      anything else is pairs_improper.  insert_median and insert_mean_x100 as the placement computes them (rule 6 there; -1 without proper
 *      pairs).  For two H reads this is the placement's rule 6 word for word: with no gapped-placed read, every pair live and max_insert the
 *      placement's, the five pair counters, the histogram, the median and the mean equal those of `pl`.
 *   3. d_flag[r], the SAM FLAG: 0x1 r is in a live pair; 0x2 the pair is proper; 0x4 r is unplaced; 0x8 r is paired and its mate is
 *      unplaced; 0x10 r is placed on the minus strand; 0x20 r is paired and its mate is placed on the minus strand; 0x40 / 0x80 r is the
 *      smaller / the larger index of a live pair.  No other bit is ever set; a read that is not live gets 0.
 *   4. d_tlen[r]: both mates of a live pair placed on the same target: max(e1, e2) - min(p1, p2), positive for the mate with the smaller p,
 *      negative for the other, at equal p positive for the smaller read index; 0 in every other case.
 *   5. Counters (alga_pair_info): reads = n / 2, live, placed_h, placed_g, unplaced (of the live reads); pairs = pairs_proper + pairs_improper +
 *      pairs_split + pairs_not_unique; pairs_with_gapped = the live pairs with at least one G mate, proper_with_gapped the proper ones among
 *      them; ms_judge (HIP events), ms_total (wall).
 *   6. Refusals (ALGA_ERR_INVALID_ARGUMENT; nothing of the result is written, an earlier result stays valid).  Host: `pl` is not the current
 *      placement; `gp` is given but is not the current gapped result or was made from an earlier placement; nodes->n / 2 != pl.n_reads; the
 *      parameters.  Device, one read-back: pair_off[v] <= 2, pair_off[v] == pair_off[v ^ 1], the mate in range and pointing back.
 * The result (alga_pair_calls) is engine-owned, valid until the next judge call on `e`; it remembers the placement and the gapped result
 * (or that there was none) it was made from.  `pl`, `gp` and every other result stay valid.  Read-backs: the check; the counters and the
 * histogram.
 *
 * alga_write_sam_device.  `calls` must be the engine's current pair calls, made from this `pl` and this `gp` (NULL where they were made
 * without one); anything else is refused.  Target lengths come from pl.d_col_off; no target bases are needed.
 *   Header: `@HD VN:1.6 SO:unsorted GO:query`, one `@SQ SN:<name(t)> LN:<len[t]>` per target with len >= 1 in target order (SAM forbids LN:0;
 *   nothing lies on such a target), `@PG ID:alga_amd PN:alga_amd`, tab separated, formatted on the host from T lengths.  name(t) =
 *   `contig_id=<t>_length=<len>`, the first token of alga_write_final_fasta_device's header; with ALGA_SAM_NAMES_DEPTH that plus
 *   `_reads=<t_reads>_depth=<q>.<dd>` from pl, the token of alga_write_final_fasta_depth_device.
 *   Records: one per live read in read order (mates adjacent), eleven tab-separated fields and the tags.  QNAME `r<q>`, q the smaller read
 *   index of the live pair, for a single read its own (the engine keeps no read names).  FLAG d_flag[r].  RNAME, POS: placed: name(target),
 *   pos + 1; unplaced with a placed live mate: the mate's; otherwise `*`, 0.  MAPQ 60 if placed and unique, else 0 (there is no second-best
 *   score to grade with).  CIGAR: unplaced `*`; H `<L>M`; G the runs of gp.d_cigar, a leading and / or trailing I run written as S (a read
 *   hanging over a target end; the clipped bases stay in SEQ).  RNEXT, PNEXT: single read `*`, 0; in a live pair the RNAME and POS fields of
 *   the mate's record (borrowed values included), `=` where the names are equal; both unplaced `*`, 0.  TLEN d_tlen[r].  SEQ the bases of
 *   node 2r if placed on the minus strand, else of node 2r + 1.  QUAL `*` (the engine keeps no qualities).  Tags, placed reads only:
 *   `NM:i:<nm>` (G: edits minus the soft-clipped bases), `XP:A:H` or `XP:A:G`.
 *   ALGA_SAM_SKIP_UNPLACED: no records for unplaced reads; every other record byte for byte as without the flag.
 *   Refusals: as for the judge; on the device, in the read-back of the sizes pass, before the file is touched: a live read with
 *   len > 16 * stride_words; a G read whose script's query length differs from len or that has no run.
 *   Not written: MD tags, qualities and read names, BAM, secondary and supplementary records, graded MAPQ, coordinate order.
 * ABI stays 7: the calls add. */
#define ALGA_SAM_NAMES_DEPTH   1     /* alga_sam_params.flags: names as the depth FASTA's header token, else as the plain final FASTA's */
#define ALGA_SAM_SKIP_UNPLACED 2     /* no records for unplaced reads                                                                 */
typedef struct {
    int32_t max_insert, flags;
    int32_t reserved[6];             /* 0                                                                                             */
} alga_pair_params;
typedef struct {
    int64_t         n_reads, n_hist; /* n / 2, max_insert + 1                                                                         */
    const uint16_t *d_flag;          /* n_reads: the SAM FLAG of the read's record                                                    */
    const int32_t  *d_tlen;          /* n_reads                                                                                       */
    const uint64_t *d_insert_hist;   /* n_hist                                                                                        */
} alga_pair_calls;
typedef struct {
    uint64_t reads, live, placed_h, placed_g, unplaced;
    uint64_t pairs, pairs_proper, pairs_improper, pairs_split, pairs_not_unique;
    uint64_t pairs_with_gapped, proper_with_gapped;   /* pairs with >= 1 mate from the gapped pass, and the proper ones among them    */
    int64_t  insert_median, insert_mean_x100;
    double   ms_judge;               /* device time (HIP events)                                                                      */
    double   ms_total;               /* wall time of the call                                                                         */
} alga_pair_info;
typedef struct {
    int32_t flags;
    int32_t reserved[7];             /* 0                                                                                             */
} alga_sam_params;
void alga_pair_default_params(alga_pair_params *p);
int  alga_judge_pairs_device(alga_engine *e, const alga_nodes *nodes, const uint8_t *d_pair_off /* may be NULL */, const alga_placements *pl,
                             const alga_gapped *gp /* may be NULL: the Hamming pass alone */, const alga_pair_params *p, void *hip_stream,
                             alga_pair_calls *out, alga_pair_info *info /* may be NULL */);
int  alga_write_sam_device(alga_engine *e, const alga_nodes *nodes, const alga_placements *pl, const alga_gapped *gp /* may be NULL */,
                           const alga_pair_calls *calls, const alga_sam_params *p, const char *path, alga_gfa_info *info /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* ALGA_AMD_H */
