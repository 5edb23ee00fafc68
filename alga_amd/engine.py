"""ctypes binding of libalga_amd.so (include/alga_amd.h) + the host-side mirror of the reference's
GraphCreator interface for this path (include/GraphCreators/GraphCreator.h:12-62 of the reference).

Nothing here computes an overlap: every build call goes through the C ABI into the HIP kernels and
raises AlgaError when the library or the device is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

EDGE_DTYPE = np.dtype([("src", np.int32), ("dst", np.int32), ("offset", np.int32)])


class AlgaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("alga_amd error %d: %s" % (code, msg))
        self.code = code


class _Info(C.Structure):
    """base of the info and stats structs.  _PER_ROUND = {array field: (its count field, its capacity)}: as_dict() cuts that list at the count"""
    _PER_ROUND = {}

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        for k, (count, cap) in self._PER_ROUND.items():
            d[k] = [int(x) for x in d[k][: min(int(getattr(self, count)), cap)]]
        return d


class _Nodes(C.Structure):
    _fields_ = [("words", C.c_void_p), ("stride_words", C.c_int32), ("len", C.c_void_p), ("n", C.c_int32),
                ("align_from", C.c_void_p), ("align_to", C.c_void_p)]


class PrefSufParams(C.Structure):
    """alga_prefsuf_params"""
    _fields_ = [("min_overlap", C.c_int32), ("rsoe_min_overlap", C.c_int32), ("soes", C.c_int32),
                ("max_len_cap", C.c_int32), ("collect_stats", C.c_int32), ("reduction", C.c_int32),
                ("keys_shared", C.c_int32), ("twin_rows", C.c_int32)]


class CompactEdges(C.Structure):
    """alga_compact_edges"""
    _fields_ = [("n_nodes", C.c_int32), ("n_edges", C.c_uint64), ("degree", C.c_void_p), ("dst", C.c_void_p), ("offset", C.c_void_p)]


class PrefSufStats(_Info):
    """alga_prefsuf_stats"""
    _fields_ = [("raw_overlaps", C.c_uint64), ("transitive_listed", C.c_uint64), ("transitive_compares", C.c_uint64),
                ("transitive_removed", C.c_uint64), ("windows_probed", C.c_uint64), ("slots_scanned", C.c_uint64),
                ("records", C.c_uint64), ("edges", C.c_uint64), ("table_slots", C.c_uint64),
                ("max_in_records", C.c_uint64), ("ms_total", C.c_double), ("ms_seed", C.c_double),
                ("ms_probe", C.c_double), ("ms_group", C.c_double), ("ms_reduce", C.c_double), ("ms_emit", C.c_double),
                ("nodes_live", C.c_uint64), ("reduction_used", C.c_uint64), ("generic_sources", C.c_uint64),
                ("big_sources", C.c_uint64), ("probe_used", C.c_uint64), ("deferred_sources", C.c_uint64), ("ms_probe_pairs", C.c_double),
                ("ms_keys", C.c_double), ("ms_sort", C.c_double), ("ms_gather", C.c_double), ("ms_dir", C.c_double), ("probe_rounds", C.c_uint64), ("ms_pile", C.c_double),
                ("pile_buckets", C.c_uint64), ("pile_irregular", C.c_uint64), ("pile_list_checked", C.c_uint64), ("pile_list_mismatch", C.c_uint64),
                ("pile_own_lists", C.c_uint64), ("host_ms_check", C.c_double), ("host_ms_upload", C.c_double), ("host_ms_build", C.c_double),
                ("host_ms_download", C.c_double), ("pile_mixed", C.c_uint64), ("pile_deferred", C.c_uint64)]


class IngestParams(C.Structure):
    """alga_ingest_params"""
    _fields_ = [("trim_left", C.c_int32), ("trim_right", C.c_int32), ("remove_reads_with_n", C.c_int32), ("rna", C.c_int32),
                ("scale", C.c_float), ("min_overlap", C.c_int32), ("rsoemo", C.c_int32), ("remove_pref_reads", C.c_int32),
                ("threads", C.c_int32)]


class NodeSet(C.Structure):
    """alga_node_set"""
    _fields_ = [("n", C.c_int32), ("stride_words", C.c_int32), ("words", C.POINTER(C.c_uint32)), ("len", C.POINTER(C.c_int32)),
                ("pair_off", C.POINTER(C.c_uint8)), ("LEN", C.c_int32), ("min_overlap", C.c_int32), ("rsoemo", C.c_int32),
                ("li_kmer_length", C.c_int32), ("records", C.c_int64), ("removed_n", C.c_int32), ("removed_str", C.c_int32),
                ("removed_prefix", C.c_int32), ("removed_short", C.c_int32), ("avg_len", C.c_double)]


class ParsedReads(C.Structure):
    """alga_parsed_reads"""
    _fields_ = [("n_nodes", C.c_int64), ("stride_words", C.c_int32), ("rows", C.POINTER(C.c_uint32)), ("len", C.POINTER(C.c_int32)),
                ("paired", C.c_int32), ("records", C.c_int64), ("removed_n", C.c_int32), ("removed_str", C.c_int32), ("LEN", C.c_int32),
                ("min_overlap", C.c_int32), ("rsoemo", C.c_int32), ("li_kmer_length", C.c_int32), ("avg_len", C.c_double),
                ("owner", C.c_void_p)]


class PreprocessInput(C.Structure):
    """alga_preprocess_input"""
    _fields_ = [("rows", C.c_void_p), ("stride_words", C.c_int32), ("len", C.c_void_p), ("n_nodes", C.c_int64),
                ("remove_pref_reads", C.c_int32), ("min_keep_len", C.c_int32)]


class DeviceNodeSet(C.Structure):
    """alga_device_node_set"""
    _fields_ = [("d_words", C.c_void_p), ("d_len", C.c_void_p), ("d_pair_off", C.c_void_p), ("n", C.c_int32), ("stride_words", C.c_int32),
                ("removed_prefix", C.c_int32), ("removed_short", C.c_int32), ("max_len", C.c_int32), ("ms_device", C.c_double)]


class IngestInfo(C.Structure):
    """alga_ingest_info"""
    _fields_ = [("records", C.c_int64), ("removed_n", C.c_int32), ("removed_str", C.c_int32), ("LEN", C.c_int32), ("min_overlap", C.c_int32),
                ("rsoemo", C.c_int32), ("li_kmer_length", C.c_int32), ("paired", C.c_int32), ("avg_len", C.c_double), ("ms_parse", C.c_double),
                ("ms_preprocess", C.c_double), ("ms_upload", C.c_double)]


class CorrectParams(C.Structure):
    """alga_correct_params"""
    _fields_ = [("k", C.c_int32), ("solid_min", C.c_int32), ("min_run", C.c_int32), ("reserved", C.c_int32)]


class CorrectInfo(_Info):
    """alga_correct_info"""
    _fields_ = [(k, C.c_uint64) for k in ("reads", "kmers_total", "kmers_distinct", "kmers_solid", "runs", "runs_fixed", "runs_ambiguous",
                                          "runs_no_candidate", "runs_skipped", "reads_changed", "slices")] + \
               [(k, C.c_double) for k in ("ms_count", "ms_index", "ms_fix", "ms_total")]


class PkbParams(C.Structure):
    """alga_pkb_params"""
    _fields_ = [("min_overlap_area", C.c_int32), ("max_offset_pct", C.c_int32), ("min_identity_pct", C.c_int32),
                ("same_ends", C.c_int32), ("li_k", C.c_int32), ("li_intervals", C.c_int32), ("rounds", C.c_int32),
                ("kmer_length_bucket", C.c_int32)]


class PkbStats(C.Structure):
    """alga_pkb_stats"""
    _fields_ = [("kmers", C.c_uint64 * 4), ("groups", C.c_uint64 * 4), ("can_align_calls", C.c_uint64 * 4),
                ("edges_after", C.c_uint64 * 4), ("max_group", C.c_uint64), ("ms_total", C.c_double), ("group_hist", (C.c_uint64 * 8) * 4)]


PROBE = {"auto": 0, "table": 1, "cluster": 2}                  # alga_probe
PILE_DECLINE_ONE_IN = 20                                       # ALGA_PILE_DECLINE_ONE_IN: the pile path keeps a build iff pile_irregular * this <= pile_buckets (round 5; between the two: the mixed form)
PILE_IRREGULAR_ONE_IN = 250                                    # ALGA_PILE_IRREGULAR_ONE_IN (include/alga_amd.h): the pile path keeps a build iff pile_irregular * this <= pile_buckets

class MultiStats(C.Structure):
    """alga_multi_stats"""
    _fields_ = [("n_ranks", C.c_int32), ("transport", C.c_int32), ("fell_back_to_one_gpu", C.c_int32), ("form", C.c_int32), ("edges", C.c_uint64),
                ("ms_upload", C.c_double), ("ms_download", C.c_double), ("ms_keys", C.c_double), ("ms_share", C.c_double), ("ms_build", C.c_double),
                ("ms_gather", C.c_double), ("ms_total", C.c_double),
                ("xbytes_keys", C.c_uint64), ("xbytes_descriptors", C.c_uint64), ("xbytes_pending", C.c_uint64), ("xbytes_small_keys", C.c_uint64),
                ("xbytes_edges", C.c_uint64), ("xbytes_gather", C.c_uint64),
                ("ms_shard_index", C.c_double), ("ms_shard_exchange", C.c_double), ("ms_shard_join", C.c_double), ("ms_shard_cap", C.c_double),
                ("ms_shard_place", C.c_double)]


class ShardStats(_Info):
    """alga_shard_stats"""
    _fields_ = [(k, C.c_uint64) for k in ("targets_owned", "descriptors_out", "descriptors_in", "flagged_sources", "records", "pending", "pending_sources",
                                          "small_keys_out", "small_keys_in", "dropped", "edges_out", "edges_in", "edges", "join_passes", "join_passes_serial")] + \
               [(k, C.c_double) for k in ("ms_index", "ms_export", "ms_sort", "ms_join", "ms_cap", "ms_edges_out", "ms_place")]


MULTI_FORM = {"auto": 0, "replicated": 1, "bucket_sharded": 2}   # alga_multi_form


TRANSPORT = {"auto": 0, "rccl": 1, "copy": 2}                  # alga_transport


class NodeKeys(C.Structure):
    _fields_ = [("d_keys", C.c_void_p), ("d_meta", C.c_void_p), ("n", C.c_int32), ("eligible", C.c_int32), ("meta_needed", C.c_int32), ("reserved", C.c_int32)]


EXPORTS = ["alga_abi_version", "alga_engine_set_option", "alga_engine_create", "alga_engine_destroy", "alga_last_error",
           "alga_engine_device_name", "alga_prefsuf_default_params", "alga_prefsuf_build_host", "alga_free_edges",
           "alga_prefsuf_build_device", "alga_prefsuf_last_stats", "alga_prefsuf_discover_device",
           "alga_prefsuf_reduce_device", "alga_prefsuf_build_range_device", "alga_prefsuf_keys_device", "alga_write_graph", "alga_ingest_default_params", "alga_ingest_files",
           "alga_free_node_set", "alga_sort_records_device", "alga_sort_edges_device", "alga_pkb_derive_params",
           "alga_can_align_batch_host", "alga_li_kmers_host", "alga_pkb_supplement_host", "alga_pkb_supplement_device",
           "alga_pkb_last_stats", "alga_parse_files", "alga_free_parsed_reads", "alga_preprocess_nodes", "alga_copy_to_host", "alga_device_alloc", "alga_device_free", "alga_copy_to_device", "alga_cut_triangles_device", "alga_cut_triangles_host", "alga_ingest_device", "alga_contig_trim_host", "alga_engine_reserve", "alga_upload_nodes", "alga_download_edges",
           "alga_multi_create", "alga_multi_destroy", "alga_multi_last_error", "alga_multi_engine", "alga_multi_prefsuf_build_host", "alga_multi_prefsuf_build_device",
           "alga_multi_free_edges", "alga_multi_last_stats", "alga_multi_set_option", "alga_upload_twin_nodes",
           "alga_shard_index_device", "alga_shard_join_device", "alga_shard_small_keys_device", "alga_shard_resolve_device", "alga_shard_place_device",
           "alga_shard_last_stats", "alga_sort_u32_pairs_device", "alga_sort_u64_pairs_device", "alga_sort_desc_device", "alga_multi_pkb_supplement_device", "alga_pkb_shard_begin", "alga_pkb_shard_round", "alga_pkb_shard_merge", "alga_pkb_shard_end",
           "alga_prefsuf_build_host_compact", "alga_download_edges_compact", "alga_free_compact_edges", "alga_host_alloc", "alga_host_free",
           "alga_write_gfa_device", "alga_unitigs_device", "alga_write_unitig_gfa_device", "alga_remove_dangling_branches_device",
           "alga_remove_short_parallel_paths_device", "alga_unitig_consensus_device", "alga_write_consensus_fasta_device",
           "alga_contigs_device", "alga_contig_trim_device", "alga_final_contigs_device", "alga_write_final_fasta_device",
           "alga_extend_contigs_device", "alga_extend_seams_get",
           "alga_correct_default_params", "alga_correct_reads_device", "alga_correct_parsed_reads", "alga_ingest_corrected_device",
           "alga_place_default_params", "alga_place_reads_device", "alga_place_reads_on_final_device", "alga_write_final_fasta_depth_device",
           "alga_polish_default_params", "alga_polish_placed_device", "alga_write_polished_fasta_device",
           "alga_scaffold_default_params", "alga_scaffold_placed_device", "alga_write_scaffold_fasta_device",
           "alga_break_default_params", "alga_break_placed_device", "alga_write_broken_fasta_device",
           "alga_grow_default_params", "alga_grow_placed_device", "alga_write_grown_fasta_device",
           "alga_merge_default_params", "alga_merge_targets_device", "alga_write_merged_fasta_device",
           "alga_contain_default_params", "alga_drop_contained_device", "alga_write_kept_fasta_device",
           "alga_stitch_default_params", "alga_stitch_targets_device", "alga_stitch_scaffolds_device", "alga_write_stitched_fasta_device",
           "alga_gapped_default_params", "alga_place_gapped_device", "alga_write_gapped_tsv_device",
           "alga_ipolish_default_params", "alga_polish_indels_device", "alga_write_ipolished_fasta_device", "alga_write_ipolish_events_tsv_device",
           "alga_pair_default_params", "alga_judge_pairs_device", "alga_write_sam_device"]

GFA_TWINS, GFA_SEQUENCES = 1, 2                                 # alga_write_gfa_device flags
GFA_CONSENSUS = 4                                                # alga_write_unitig_gfa_device: segments carry the consensus


class GfaInfo(_Info):
    """alga_gfa_info"""
    _fields_ = [("segments", C.c_uint64), ("links", C.c_uint64), ("links_merged", C.c_uint64), ("bytes", C.c_uint64),
                ("ms_format", C.c_double), ("ms_total", C.c_double)]


TIPS_MAX_PASSES = 64                                             # ALGA_TIPS_MAX_PASSES


class TipsInfo(_Info):
    """alga_tips_info"""
    _PER_ROUND = {"removed": ("passes", TIPS_MAX_PASSES)}
    _fields_ = [("edges_in", C.c_uint64), ("edges_unique", C.c_uint64), ("edges_out", C.c_uint64), ("iterations", C.c_int32), ("passes", C.c_int32),
                ("removed", C.c_uint64 * TIPS_MAX_PASSES), ("removed_total", C.c_uint64), ("branching_nodes", C.c_uint64), ("overflow_nodes", C.c_uint64),
                ("ms_prepare", C.c_double), ("ms_passes", C.c_double), ("ms_total", C.c_double)]


MST_MAX_ROUNDS = 64                                              # ALGA_MST_MAX_ROUNDS


class MstInfo(_Info):
    """alga_mst_info"""
    _PER_ROUND = {"winners": ("rounds", MST_MAX_ROUNDS)}
    _fields_ = [("edges_in", C.c_uint64), ("edges_out", C.c_uint64), ("branching_nodes", C.c_uint64), ("begs_run", C.c_uint64), ("rounds", C.c_uint64),
                ("winners", C.c_uint64 * MST_MAX_ROUNDS), ("overflow_begs", C.c_uint64), ("ball_max", C.c_uint64),
                ("ms_prepare", C.c_double), ("ms_rounds", C.c_double), ("ms_total", C.c_double)]


UNITIG_SKIP_ISOLATED = 1                                         # alga_unitigs_device flag


class UnitigsC(C.Structure):
    """alga_unitigs"""
    _fields_ = [("n_pairs", C.c_int32), ("d_words", C.c_void_p), ("d_word_off", C.c_void_p), ("d_len", C.c_void_p), ("d_path_node", C.c_void_p),
                ("d_path_pos", C.c_void_p), ("d_path_off", C.c_void_p), ("d_edges", C.c_void_p), ("n_edges", C.c_uint64)]


class UnitigInfo(_Info):
    """alga_unitig_info"""
    _fields_ = [(k, C.c_uint64) for k in ("edges_in", "edges_sym", "twins_added", "compactable", "cycles_cut", "isolated_skipped", "longest_nodes",
                                          "longest_bases", "total_bases", "total_nodes")] + [("rank_rounds", C.c_int32)] + \
               [(k, C.c_double) for k in ("ms_sym", "ms_rank", "ms_layout", "ms_seq", "ms_edges", "ms_total")]


CONTIG_MAX_ROUNDS = 64


class ContigInfo(_Info):
    """alga_contig_info"""
    _PER_ROUND = {k: ("rounds", CONTIG_MAX_ROUNDS) for k in ("chains", "parallel_drops", "groups_cut", "base_edges_dropped")}
    _fields_ = [(k, C.c_uint64) for k in ("edges_in", "edges_sym", "rounds")] + [(k, C.c_uint64 * CONTIG_MAX_ROUNDS) for k in _PER_ROUND] + \
               [(k, C.c_uint64) for k in ("final_edges", "path_nodes", "junction_nodes", "cycles_cut", "closed_chains", "reads_dropped", "longest_nodes",
                                          "longest_bases", "total_bases")] + [("rank_rounds", C.c_int32)] + \
               [(k, C.c_double) for k in ("ms_sym", "ms_rounds", "ms_layout", "ms_seq", "ms_edges", "ms_total")]


EXTEND_HEAD_SLICE = 1024                                          # ALGA_EXTEND_HEAD_SLICE


class ExtendInfo(_Info):
    """alga_extend_info"""
    _fields_ = [(k, C.c_uint64) for k in ("candidates", "direct_links", "links", "joinable", "ambiguous", "cycles_cut", "pairs_in", "pairs_out", "head_max",
                                          "head_passes", "longest_nodes", "longest_bases", "total_bases")] + [("rank_rounds", C.c_int32)] + \
               [(k, C.c_double) for k in ("ms_count", "ms_paths", "ms_layout", "ms_seq", "ms_edges", "ms_total")]


class ExtendSeamsC(C.Structure):
    """alga_extend_seams"""
    _fields_ = [("d_seam_off", C.c_void_p), ("d_seam_entry", C.c_void_p), ("n_seams", C.c_uint64)]


class Unitigs:
    """Result of Engine.unitigs: zero-copy torch views of the engine's device memory (valid until the next Engine.unitigs call on
    that engine; clone what has to live longer) -- words int32 [total words], word_off / path_off int64 [n_pairs + 1], len int32
    [n_pairs], path_node / path_pos int32 [total nodes], edges int32 [n_edges, 3] -- and .info (dict of alga_unitig_info)."""

    def __init__(self, c, info, device):
        self._c, self.info, self.n_pairs, self.n_edges = c, info, int(c.n_pairs), int(c.n_edges)
        P = self.n_pairs
        dev = "cuda:%d" % device
        self.word_off = device_view(c.d_word_off, (P + 1,), dev, "<i8")
        self.path_off = device_view(c.d_path_off, (P + 1,), dev, "<i8")
        self.len = device_view(c.d_len, (P,), dev)
        self.words = device_view(c.d_words, (int(self.word_off[-1]),), dev)
        total_nodes = int(self.path_off[-1])
        self.path_node = device_view(c.d_path_node, (total_nodes,), dev)
        self.path_pos = device_view(c.d_path_pos, (total_nodes,), dev)
        self.edges = device_view(c.d_edges, (self.n_edges, 3), dev)

    def to_host(self):
        """numpy copies, in the dtypes of tests/unitig_checker.py"""
        h = lambda t: t.cpu().numpy().copy()
        return dict(n_pairs=self.n_pairs, words=h(self.words).view(np.uint32), word_off=h(self.word_off).view(np.uint64), len=h(self.len),
                    path_node=h(self.path_node), path_pos=h(self.path_pos), path_off=h(self.path_off).view(np.uint64),
                    edges=h(self.edges).reshape(-1, 3), info=dict(self.info))


CONSENSUS_VOTES = 1                                              # alga_unitig_consensus_device flag


class ConsensusC(C.Structure):
    """alga_consensus"""
    _fields_ = [("n_pairs", C.c_int32), ("d_words", C.c_void_p), ("d_trim_left", C.c_void_p), ("d_len", C.c_void_p), ("d_changed", C.c_void_p),
                ("d_votes", C.c_void_p)]


class ConsensusInfo(_Info):
    """alga_consensus_info"""
    _fields_ = [(k, C.c_uint64) for k in ("pairs", "pairs_kept", "columns", "trimmed_bases", "changed", "max_depth", "wide_words")] + \
               [(k, C.c_double) for k in ("ms_vote", "ms_window", "ms_total")]


class Consensus:
    """Result of Engine.unitig_consensus: zero-copy torch views of the engine's device memory (valid until the next Engine.unitig_consensus or
    Engine.unitigs call on that engine; clone what has to live longer) -- words int32 [total words] (the untrimmed consensus in the layout of
    Unitigs.words), trim_left / len / changed int32 [n_pairs], votes uint8 [16 * total words] or None -- and .info (dict of
    alga_consensus_info)."""

    def __init__(self, c, info, unitigs, device):
        self._c, self.info, self.n_pairs = c, info, int(c.n_pairs)
        P = self.n_pairs
        dev = "cuda:%d" % device
        total_words = int(unitigs.words.shape[0])
        self.words = device_view(c.d_words, (total_words,), dev)
        self.trim_left = device_view(c.d_trim_left, (P,), dev)
        self.len = device_view(c.d_len, (P,), dev)
        self.changed = device_view(c.d_changed, (P,), dev)
        self.votes = device_view(c.d_votes, (16 * total_words,), dev, "|u1") if c.d_votes else None

    def to_host(self):
        """numpy copies, in the dtypes of tests/consensus_checker.py"""
        h = lambda t: t.cpu().numpy().copy()
        return dict(n_pairs=self.n_pairs, words=h(self.words).view(np.uint32), trim_left=h(self.trim_left), len=h(self.len), changed=h(self.changed),
                    votes=None if self.votes is None else h(self.votes), info=dict(self.info))


FINAL_SHORT, FINAL_REJECTED, FINAL_ACCEPTED, FINAL_TRIMMED_AWAY = 0, 1, 2, 3     # ALGA_FINAL_*: alga_final_contigs.d_verdict


class FinalContigsC(C.Structure):
    """alga_final_contigs"""
    _fields_ = [("n_pairs", C.c_int32), ("n_accepted", C.c_int32), ("n_written", C.c_int32), ("reserved", C.c_int32), ("d_verdict", C.c_void_p),
                ("d_rank", C.c_void_p), ("d_id", C.c_void_p), ("d_new_reads", C.c_void_p), ("d_trim_left", C.c_void_p), ("d_begin", C.c_void_p),
                ("d_len", C.c_void_p), ("d_order", C.c_void_p)]


class FinalInfo(_Info):
    """alga_final_info"""
    _fields_ = [(k, C.c_uint64) for k in ("pairs", "n_short", "rejected", "accepted", "trimmed_away", "filter_rounds", "trim_edges")] + \
               [(k, C.c_double) for k in ("ms_filter", "ms_trim", "ms_total")]


class FinalContigs:
    """Result of Engine.final_contigs: zero-copy torch views of the engine's device memory (valid until the next Engine.unitigs, contigs,
    unitig_consensus or final_contigs call on that engine; clone what has to live longer) -- verdict uint8 [n_pairs] (FINAL_*), rank / id /
    new_reads / trim_left / begin / len int32 [n_pairs], order int32 [n_accepted] -- the counts n_accepted / n_written and .info (dict of
    alga_final_info)."""
    KEYS = ("verdict", "rank", "id", "new_reads", "trim_left", "begin", "len", "order")

    def __init__(self, c, info, unitigs, consensus, device):
        self._c, self.info, self.n_pairs, self.n_accepted, self.n_written = c, info, int(c.n_pairs), int(c.n_accepted), int(c.n_written)
        self._unitigs, self._consensus = unitigs, consensus
        P = self.n_pairs
        dev = "cuda:%d" % device
        self.verdict = device_view(c.d_verdict, (P,), dev, "|u1")
        for k in self.KEYS[1:-1]:
            setattr(self, k, device_view(getattr(c, "d_" + k), (P,), dev))
        self.order = device_view(c.d_order, (self.n_accepted,), dev)

    def to_host(self):
        """numpy copies, in the dtypes of tests/final_checker.py"""
        d = {k: getattr(self, k).cpu().numpy().copy() for k in self.KEYS}
        d.update(n_pairs=self.n_pairs, n_accepted=self.n_accepted, n_written=self.n_written, info=dict(self.info))
        return d


class _Result:
    """base of the stages' result wrappers.  COUNTS: the integer fields of the C struct that become attributes; KEYS = ((name, typestr of the
    view, dtype of to_host(), size key), ...): attribute `name` is the zero-copy view of c.d_<name> with _sizes()[size key] entries (an entry
    without a size key: _sizes()[name], and n_targets where that has none); KEPT: the attribute that keeps what the result was made from alive"""
    COUNTS, KEYS, KEPT = (), (), "_source"

    def __init__(self, c, info, device, source=None):
        self._c, self.info = c, info
        setattr(self, self.KEPT, source)
        for k in self.COUNTS:
            setattr(self, k, int(getattr(c, k)))
        self._dev = "cuda:%d" % device
        size = self._sizes()
        for k, typestr, *rest in self.KEYS:
            setattr(self, k, device_view(getattr(c, "d_" + k), (size[rest[1]] if len(rest) > 1 else size.get(k, getattr(self, "n_targets", 0)),), self._dev, typestr))

    def to_host(self):
        """numpy copies of every array of KEYS, in the dtypes of the stage's checker under tests/, and info"""
        d = {k: getattr(self, k).cpu().numpy().copy().view(dt) for k, _, dt, *_ in self.KEYS}
        d["info"] = dict(self.info)
        return d


class _RaggedResult(_Result):
    """a result that carries sequences of its own: words, begin, len"""

    def targets(self):
        """(words, begin int64, len int32): the result's sequences as the ragged target set Engine.place_reads(targets=...) and Engine.merge_ends
        take; sequence j is target j of that call (the tensors are the engine's)"""
        return self.words, self.begin, self.len


PLACE_DEPTH_MULTI = 1                                            # alga_place_params.flags
PLACE_PLACED, PLACE_UNIQUE, PLACE_MINUS = 1, 2, 4                # bits of Placements.state


class PlaceParams(C.Structure):
    """alga_place_params"""
    _fields_ = [(k, C.c_int32) for k in ("k", "max_mismatches", "max_occ", "max_insert", "flags")] + [("reserved", C.c_int32 * 3)]


class PlaceInfo(_Info):
    """alga_place_info"""
    _fields_ = [(k, C.c_uint64) for k in ("reads", "placed", "unique", "multi", "unplaced", "hits_saturated", "seeds", "seeds_over_max_occ", "index_positions",
                                          "index_distinct", "pairs", "pairs_proper", "pairs_improper", "pairs_split", "pairs_not_unique")] + \
               [(k, C.c_int64) for k in ("insert_median", "insert_mean_x100")] + [(k, C.c_double) for k in ("ms_index", "ms_place", "ms_depth", "ms_total")]


class PlacementsC(C.Structure):
    """alga_placements"""
    _fields_ = [("n_reads", C.c_int64), ("n_targets", C.c_int64), ("n_columns", C.c_uint64), ("n_hist", C.c_int64)] + \
               [(k, C.c_void_p) for k in ("d_target", "d_pos", "d_mm", "d_hits", "d_state", "d_col_off", "d_cover", "d_t_reads", "d_t_bases", "d_t_mismatches",
                                          "d_t_uncovered", "d_insert_hist")]


class Placements(_Result):
    """Result of Engine.place_reads: zero-copy torch views of the engine's device memory (valid until the next Engine.place_reads call on that
    engine; clone what has to live longer) -- target / pos int32 [n_reads], mm / hits / state uint8 [n_reads], col_off int32 [n_targets + 1]
    and cover int32 [n_columns] (the bits of uint32), t_reads / t_bases / t_mismatches / t_uncovered int64 [n_targets], insert_hist int64
    [max_insert + 1] -- and .info (dict of alga_place_info)."""
    KEYS = (("target", "<i4", np.int32), ("pos", "<i4", np.int32), ("mm", "|u1", np.uint8), ("hits", "|u1", np.uint8), ("state", "|u1", np.uint8),
            ("col_off", "<i4", np.uint32), ("cover", "<i4", np.uint32), ("t_reads", "<i8", np.uint64), ("t_bases", "<i8", np.uint64),
            ("t_mismatches", "<i8", np.uint64), ("t_uncovered", "<i8", np.uint64), ("insert_hist", "<i8", np.uint64))
    COUNTS, KEPT = ("n_reads", "n_targets", "n_columns", "n_hist"), "_final"

    def _sizes(self):
        return dict(target=self.n_reads, pos=self.n_reads, mm=self.n_reads, hits=self.n_reads, state=self.n_reads, col_off=self.n_targets + 1,
                    cover=self.n_columns, insert_hist=self.n_hist)


POLISH_MULTI, POLISH_COUNTS = 1, 2                               # alga_polish_params.flags


class PolishParams(C.Structure):
    """alga_polish_params"""
    _fields_ = [(k, C.c_int32) for k in ("min_cover", "min_percent", "flags")] + [("reserved", C.c_int32 * 5)]


class PolishInfo(_Info):
    """alga_polish_info"""
    _fields_ = [(k, C.c_uint64) for k in ("columns", "voters", "votes", "voted_columns", "changed", "ambiguous", "max_cover")] + \
               [(k, C.c_double) for k in ("ms_sort", "ms_vote", "ms_total")]


class PolishedC(C.Structure):
    """alga_polished"""
    _fields_ = [("n_targets", C.c_int64), ("n_columns", C.c_uint64), ("n_changed", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("d_col_off", "d_words", "d_changed_cols", "d_changed_bases", "d_t_changed", "d_t_ambiguous", "d_counts")]


class Polished(_Result):
    """Result of Engine.polish: zero-copy torch views of the engine's device memory (valid until the next Engine.polish call on that engine;
    clone what has to live longer) -- col_off int32 [n_targets + 1], words int32 [(n_columns + 15) / 16 + 2] (the bits of uint32: column g
    in word g >> 4 at bits 2 * (g & 15)), changed_cols int32 [n_changed] (the bits of uint32, ascending), changed_bases uint8 [n_changed]
    (old | new << 2), t_changed / t_ambiguous int64 [n_targets], counts int32 [n_columns, 4] or None -- and .info (dict of alga_polish_info)."""
    KEYS = (("col_off", "<i4", np.uint32), ("words", "<i4", np.uint32), ("changed_cols", "<i4", np.uint32), ("changed_bases", "|u1", np.uint8),
            ("t_changed", "<i8", np.uint64), ("t_ambiguous", "<i8", np.uint64))
    COUNTS, KEPT = ("n_targets", "n_columns", "n_changed"), "_placements"

    def __init__(self, c, info, device, placements=None):
        super().__init__(c, info, device, placements)
        self.counts = device_view(c.d_counts, (self.n_columns, 4), self._dev, "<i4") if c.d_counts else None

    def _sizes(self):
        return dict(col_off=self.n_targets + 1, words=(self.n_columns + 15) // 16 + 2, changed_cols=self.n_changed, changed_bases=self.n_changed)

    def to_host(self):
        d = super().to_host()
        d["counts"] = None if self.counts is None else self.counts.cpu().numpy().copy().view(np.uint32)
        return d

    def targets(self):
        """(words, begin int64 [T], len int32 [T]): the polished sequences as the ragged target set Engine.place_reads(targets=...) takes
        (the words are the engine's; begin and len are new tensors)"""
        import torch
        off = self.col_off.to(torch.int64) & 0xFFFFFFFF
        return self.words, off[:-1].contiguous(), (off[1:] - off[:-1]).to(torch.int32).contiguous()


SCAFFOLD_BUNDLE_SUPPORTED, SCAFFOLD_BUNDLE_JOIN, SCAFFOLD_BUNDLE_DROPPED_CYCLE = 1, 2, 4     # bits of Scaffolds.b_state
SCAFFOLD_END_HAS_SUPPORTED, SCAFFOLD_END_AMBIGUOUS, SCAFFOLD_END_JOINED = 1, 2, 4         # bits of Scaffolds.end_state


class ScaffoldParams(C.Structure):
    """alga_scaffold_params"""
    _fields_ = [(k, C.c_int32) for k in ("insert", "max_insert", "min_links", "max_second_percent", "min_gap", "flags")] + [("reserved", C.c_int32 * 2)]


class ScaffoldInfo(_Info):
    """alga_scaffold_info"""
    _fields_ = [(k, C.c_uint64) for k in ("pairs_split", "links", "links_too_far", "bundles", "bundles_supported", "ends_ambiguous", "joins", "joins_dropped_cycle",
                                          "scaffolds", "scaffolds_multi", "longest", "n50_targets", "n50_scaffolds")] + \
               [(k, C.c_double) for k in ("ms_links", "ms_chain", "ms_total")]


class ScaffoldsC(C.Structure):
    """alga_scaffolds"""
    _fields_ = [(k, C.c_int64) for k in ("n_targets", "n_bundles", "n_scaffolds", "n_members")] + \
               [(k, C.c_void_p) for k in ("d_b_a", "d_b_b", "d_b_links", "d_b_span", "d_b_gap", "d_b_state", "d_end_state", "d_scaffold", "d_rank", "d_orient", "d_start",
                                          "d_gap_after", "d_join_links", "d_s_off", "d_s_members", "d_s_len")]


class Scaffolds(_Result):
    """Result of Engine.scaffold: zero-copy torch views of the engine's device memory (valid until the next Engine.scaffold call on that engine;
    clone what has to live longer) -- per bundle b_a / b_b / b_links int32 (the bits of uint32), b_span int64, b_gap int32, b_state uint8; end_state
    uint8 [2 * n_targets]; per target scaffold / rank int32, orient uint8, start int64, gap_after int32, join_links int32; s_off int32
    [n_scaffolds + 1], s_members int32 [n_members], s_len int64 [n_scaffolds] -- and .info (dict of alga_scaffold_info)."""
    KEYS = (("b_a", "<i4", np.uint32, "b"), ("b_b", "<i4", np.uint32, "b"), ("b_links", "<i4", np.uint32, "b"), ("b_span", "<i8", np.uint64, "b"),
            ("b_gap", "<i4", np.int32, "b"), ("b_state", "|u1", np.uint8, "b"), ("end_state", "|u1", np.uint8, "e"), ("scaffold", "<i4", np.int32, "t"),
            ("rank", "<i4", np.int32, "t"), ("orient", "|u1", np.uint8, "t"), ("start", "<i8", np.uint64, "t"), ("gap_after", "<i4", np.int32, "t"),
            ("join_links", "<i4", np.uint32, "t"), ("s_off", "<i4", np.uint32, "s1"), ("s_members", "<i4", np.int32, "m"), ("s_len", "<i8", np.uint64, "s"))
    COUNTS, KEPT = ("n_targets", "n_bundles", "n_scaffolds", "n_members"), "_placements"

    def _sizes(self):
        return dict(b=self.n_bundles, e=2 * self.n_targets, t=self.n_targets, s1=self.n_scaffolds + 1, m=self.n_members, s=self.n_scaffolds)

    def layout_tsv(self, host=None):
        """one line per member contig in (scaffold, rank) order: scaffold, rank, contig, orient (+/-), start, length, gap_after, links (tabs);
        the text alga_hip --scaffold_layout= writes"""
        return layout_tsv(host if host is not None else self.to_host())


def layout_tsv(h, tlen=None):
    """the layout of a scaffold result read back (Scaffolds.to_host()).  tlen: the targets' lengths; by default they are taken from the
    result itself (a member ends where the next one starts less its gap, the last one at s_len), so the placement need not be at hand"""
    lines = []
    if tlen is None:
        tlen = np.zeros(len(h["rank"]), dtype=np.int64)
        for j in range(len(h["s_len"])):
            mem = [int(c) for c in h["s_members"][int(h["s_off"][j]):int(h["s_off"][j + 1])]]
            ends = [int(h["start"][c]) for c in mem[1:]] + [int(h["s_len"][j])]
            for c, e in zip(mem, ends):
                tlen[c] = e - int(h["start"][c]) - int(h["gap_after"][c])
    for j in range(len(h["s_len"])):
        for c in h["s_members"][int(h["s_off"][j]):int(h["s_off"][j + 1])]:
            c = int(c)
            lines.append("%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (j, int(h["rank"][c]), c, "-" if h["orient"][c] else "+", int(h["start"][c]), int(tlen[c]),
                                                              int(h["gap_after"][c]), int(h["join_links"][c])))
    return "".join(lines)


class BreakParams(C.Structure):
    """alga_break_params"""
    _fields_ = [(k, C.c_int32) for k in ("min_span", "inset", "margin", "flags")] + [("reserved", C.c_int32 * 4)]


class BreakInfo(_Info):
    """alga_break_info"""
    _fields_ = [(k, C.c_uint64) for k in ("pairs_proper", "pairs_spanning", "candidate_columns", "weak_columns", "runs", "runs_open", "cuts", "targets_cut", "pieces",
                                          "max_span", "longest_piece", "n50_targets", "n50_pieces")] + \
               [(k, C.c_double) for k in ("ms_span", "ms_cut", "ms_total")]


class BrokenC(C.Structure):
    """alga_broken"""
    _fields_ = [(k, C.c_int64) for k in ("n_targets", "n_pieces", "n_cuts")] + [("n_columns", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("d_span", "d_cut_cols", "d_cut_first", "d_cut_last", "d_t_cuts", "d_piece_off", "d_begin", "d_len", "d_piece_target",
                                          "d_piece_start", "d_words")]


class Broken(_RaggedResult):
    """Result of Engine.break_contigs: zero-copy torch views of the engine's device memory (valid until the next Engine.break_contigs call on
    that engine; clone what has to live longer) -- span int32 [n_columns] (the bits of uint32), cut_cols / cut_first / cut_last int32 [n_cuts]
    (column space), t_cuts int32 [n_targets], piece_off int32 [n_pieces + 1], begin int64, len int32, piece_target int32, piece_start int32
    [n_pieces], words int32 [(n_columns + 15) / 16 + 2] (the result's own copy of the bases) -- and .info (dict of alga_break_info)."""
    KEYS = (("span", "<i4", np.uint32, "c"), ("cut_cols", "<i4", np.uint32, "k"), ("cut_first", "<i4", np.uint32, "k"), ("cut_last", "<i4", np.uint32, "k"),
            ("t_cuts", "<i4", np.uint32, "t"), ("piece_off", "<i4", np.uint32, "p1"), ("begin", "<i8", np.uint64, "p"), ("len", "<i4", np.int32, "p"),
            ("piece_target", "<i4", np.int32, "p"), ("piece_start", "<i4", np.uint32, "p"), ("words", "<i4", np.uint32, "w"))
    COUNTS, KEPT = ("n_targets", "n_pieces", "n_cuts", "n_columns"), "_placements"

    def _sizes(self):
        return dict(c=self.n_columns, k=self.n_cuts, t=self.n_targets, p1=self.n_pieces + 1, p=self.n_pieces, w=(self.n_columns + 15) // 16 + 2)

    def cuts_tsv(self, host=None):
        """one line per cut: contig, cut, run_first, run_last (tabs) in target-local columns; the text alga_hip --break_cuts= writes"""
        return cuts_tsv(host if host is not None else self.to_host())


def cuts_tsv(h):
    """the cuts of a break result read back (Broken.to_host()): the piece behind cut i is the i-th piece that starts inside its target"""
    lines = []
    behind = np.nonzero(np.asarray(h["piece_start"]) > 0)[0]
    for i, j in enumerate(behind):
        base = int(h["piece_off"][j]) - int(h["piece_start"][j])
        lines.append("%d\t%d\t%d\t%d\n" % (int(h["piece_target"][j]), int(h["cut_cols"][i]) - base, int(h["cut_first"][i]) - base, int(h["cut_last"][i]) - base))
    return "".join(lines)


GROW_OVERHANGS, GROW_VOTES, GROW_MINUS = 1, 2, 4                   # bits of Grown.state


class GrowParams(C.Structure):
    """alga_grow_params"""
    _fields_ = [(k, C.c_int32) for k in ("k", "max_mismatches", "max_occ", "min_anchor", "min_cover", "min_percent", "max_grow", "flags")] + [("reserved", C.c_int32 * 4)]


class GrowInfo(_Info):
    """alga_grow_info"""
    _fields_ = [(k, C.c_uint64) for k in ("candidates", "overhanging", "voting", "multi", "hits_saturated", "seeds", "seeds_over_max_occ", "index_positions",
                                          "ends_with_voters", "ends_grown", "bases_added", "longest_growth", "stops_cover", "stops_percent", "stops_max",
                                          "columns_before", "columns_after", "n50_before", "n50_after")] + \
               [(k, C.c_double) for k in ("ms_index", "ms_place", "ms_build", "ms_total")]


class GrownC(C.Structure):
    """alga_grown"""
    _fields_ = [(k, C.c_int64) for k in ("n_reads", "n_targets", "max_grow")] + [("n_columns", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("d_end", "d_over", "d_mm", "d_hits", "d_state", "d_count", "d_e_stop", "d_e_voters", "d_left", "d_right", "d_len", "d_col_off",
                                          "d_begin", "d_words")]


class Grown(_RaggedResult):
    """Result of Engine.grow_ends: zero-copy torch views of the engine's device memory (valid until the next Engine.grow_ends call on that
    engine; clone what has to live longer) -- per read end / over int32, mm / hits / state uint8; count int32 [2 * n_targets * max_grow * 4] (the
    bits of uint32); e_stop uint8, e_voters int32 [2 * n_targets]; left / right / len int32 [n_targets], col_off int32 [n_targets + 1], begin
    int64 [n_targets], words int32 [(n_columns + 15) / 16 + 2] (the result's own copy of the bases) -- and .info (dict of alga_grow_info)."""
    KEYS = (("end", "<i4", np.int32, "r"), ("over", "<i4", np.int32, "r"), ("mm", "|u1", np.uint8, "r"), ("hits", "|u1", np.uint8, "r"), ("state", "|u1", np.uint8, "r"),
            ("count", "<i4", np.uint32, "c"), ("e_stop", "|u1", np.uint8, "e"), ("e_voters", "<i4", np.uint32, "e"), ("left", "<i4", np.uint32, "t"),
            ("right", "<i4", np.uint32, "t"), ("len", "<i4", np.int32, "t"), ("col_off", "<i4", np.uint32, "t1"), ("begin", "<i8", np.uint64, "t"),
            ("words", "<i4", np.uint32, "w"))
    COUNTS, KEPT = ("n_reads", "n_targets", "max_grow", "n_columns"), "_placements"

    def _sizes(self):
        return dict(r=self.n_reads, c=8 * self.n_targets * self.max_grow, e=2 * self.n_targets, t=self.n_targets, t1=self.n_targets + 1,
                    w=(self.n_columns + 15) // 16 + 2)

    def grow_tsv(self, host=None):
        """one line per target: contig, left, right, voters_left, voters_right, stop_left, stop_right (tabs); the text alga_hip --grow_layout= writes"""
        return grow_tsv(host if host is not None else self.to_host())


def grow_tsv(h):
    """the growth of a grow result read back (Grown.to_host())"""
    return "".join("%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (t, int(h["left"][t]), int(h["right"][t]), int(h["e_voters"][2 * t]), int(h["e_voters"][2 * t + 1]),
                                                       int(h["e_stop"][2 * t]), int(h["e_stop"][2 * t + 1])) for t in range(len(h["len"])))


MERGE_END_HAS_OVERLAP, MERGE_END_AMBIGUOUS, MERGE_END_JOINED, MERGE_END_DROPPED_CYCLE = 1, 2, 4, 8   # bits of Merged.end_state


class MergeParams(C.Structure):
    """alga_merge_params"""
    _fields_ = [(k, C.c_int32) for k in ("k", "max_mismatches", "max_occ", "min_overlap", "max_overlap", "flags")] + [("reserved", C.c_int32 * 2)]


class MergeInfo(_Info):
    """alga_merge_info"""
    _fields_ = [(k, C.c_uint64) for k in ("ends", "index_positions", "seeds", "seeds_over_max_occ", "ends_with_overlap", "ends_ambiguous", "hits_saturated", "joins",
                                          "joins_dropped_cycle", "join_mismatches", "bases_removed", "longest_overlap", "merged", "merged_multi", "longest",
                                          "columns_before", "columns_after", "n50_before", "n50_after")] + \
               [(k, C.c_double) for k in ("ms_index", "ms_overlap", "ms_build", "ms_total")]


class MergedC(C.Structure):
    """alga_merged"""
    _fields_ = [(k, C.c_int64) for k in ("n_targets", "n_merged", "n_members")] + [("n_columns", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("d_partner", "d_olen", "d_mm", "d_hits", "d_end_state", "d_merged", "d_rank", "d_orient", "d_start", "d_overlap_after", "d_m_off",
                                          "d_m_members", "d_len", "d_col_off", "d_begin", "d_words")]


class Merged(_RaggedResult):
    """Result of Engine.merge_ends: zero-copy torch views of the engine's device memory (valid until the next Engine.merge_ends call on that
    engine; clone what has to live longer) -- per end partner / olen int32, mm / hits / end_state uint8 [2 * n_targets]; per target merged /
    rank int32, orient uint8, start int32 (the bits of uint32), overlap_after int32; m_off int32 [n_merged + 1], m_members int32 [n_members];
    len int32 [n_merged], col_off int32 [n_merged + 1], begin int64 [n_merged], words int32 [(n_columns + 15) / 16 + 2] (the result's own copy
    of the bases) -- and .info (dict of alga_merge_info)."""
    KEYS = (("partner", "<i4", np.int32, "e"), ("olen", "<i4", np.int32, "e"), ("mm", "|u1", np.uint8, "e"), ("hits", "|u1", np.uint8, "e"),
            ("end_state", "|u1", np.uint8, "e"), ("merged", "<i4", np.int32, "t"), ("rank", "<i4", np.int32, "t"), ("orient", "|u1", np.uint8, "t"),
            ("start", "<i4", np.uint32, "t"), ("overlap_after", "<i4", np.int32, "t"), ("m_off", "<i4", np.uint32, "m1"), ("m_members", "<i4", np.int32, "mm"),
            ("len", "<i4", np.int32, "m"), ("col_off", "<i4", np.uint32, "m1"), ("begin", "<i8", np.uint64, "m"), ("words", "<i4", np.uint32, "w"))
    COUNTS = ("n_targets", "n_merged", "n_members", "n_columns")

    def _sizes(self):
        return dict(e=2 * self.n_targets, t=self.n_targets, m=self.n_merged, m1=self.n_merged + 1, mm=self.n_members, w=(self.n_columns + 15) // 16 + 2)

    def merge_tsv(self, tlen=None, host=None):
        """one line per member in (merged, rank) order: merged, rank, contig, orient, start, length, overlap_after, mm (tabs); tlen: the lengths
        of the targets that were merged (by default read back from the targets of the call); the text alga_hip --merge_layout= writes"""
        if tlen is None:
            tlen = self._source[2].cpu().numpy()
        return merge_tsv(host if host is not None else self.to_host(), tlen)


def merge_tsv(h, tlen):
    """the layout of a merge result read back (Merged.to_host())"""
    lines = []
    for j in range(len(h["len"])):
        for c in h["m_members"][int(h["m_off"][j]):int(h["m_off"][j + 1])]:
            c = int(c)
            out = 2 * c + (int(h["orient"][c]) ^ 1)
            lines.append("%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (j, int(h["rank"][c]), c, "-" if h["orient"][c] else "+", int(h["start"][c]), int(tlen[c]),
                                                             int(h["overlap_after"][c]), int(h["mm"][out]) if h["overlap_after"][c] else 0))
    return "".join(lines)


CONTAIN_CONTAINED, CONTAIN_MINUS, CONTAIN_AMBIGUOUS, CONTAIN_DUPLICATE, CONTAIN_KEPT = 1, 2, 4, 8, 16   # bits of Kept.state


class ContainParams(C.Structure):
    """alga_contain_params"""
    _fields_ = [(k, C.c_int32) for k in ("k", "max_permille", "max_occ", "flags")] + [("reserved", C.c_int32 * 2)]


class ContainInfo(_Info):
    """alga_contain_info"""
    _fields_ = [(k, C.c_uint64) for k in ("queries", "index_positions", "seeds", "seeds_over_max_occ", "candidates", "contained", "contained_minus", "duplicates",
                                          "ambiguous", "hits_saturated", "kept", "bases_removed", "longest_contained", "columns_before", "columns_after",
                                          "n50_before", "n50_after")] + \
               [(k, C.c_double) for k in ("ms_index", "ms_contain", "ms_build", "ms_total")]


class KeptC(C.Structure):
    """alga_kept"""
    _fields_ = [(k, C.c_int64) for k in ("n_targets", "n_kept")] + [("n_columns", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("d_host", "d_host_pos", "d_host_orient", "d_mm", "d_hits", "d_state", "d_root", "d_root_pos", "d_root_orient", "d_absorbed", "d_new",
                                          "d_old", "d_len", "d_col_off", "d_begin", "d_words")]


class Kept(_RaggedResult):
    """Result of Engine.drop_contained: zero-copy torch views of the engine's device memory (valid until the next Engine.drop_contained call on
    that engine; clone what has to live longer) -- per input target host / host_pos int32, host_orient uint8, mm int32 (the bits of uint32),
    hits / state uint8, root / root_pos int32, root_orient uint8, absorbed int32 (the bits of uint32), new int32 [n_targets]; old int32
    [n_kept]; len int32 [n_kept], col_off int32 [n_kept + 1], begin int64 [n_kept], words int32 [(n_columns + 15) / 16 + 2] (the result's own
    copy of the bases) -- and .info (dict of alga_contain_info)."""
    KEYS = (("host", "<i4", np.int32, "t"), ("host_pos", "<i4", np.int32, "t"), ("host_orient", "|u1", np.uint8, "t"), ("mm", "<i4", np.uint32, "t"),
            ("hits", "|u1", np.uint8, "t"), ("state", "|u1", np.uint8, "t"), ("root", "<i4", np.int32, "t"), ("root_pos", "<i4", np.int32, "t"),
            ("root_orient", "|u1", np.uint8, "t"), ("absorbed", "<i4", np.uint32, "t"), ("new", "<i4", np.int32, "t"), ("old", "<i4", np.int32, "m"),
            ("len", "<i4", np.int32, "m"), ("col_off", "<i4", np.uint32, "m1"), ("begin", "<i8", np.uint64, "m"), ("words", "<i4", np.uint32, "w"))
    COUNTS = ("n_targets", "n_kept", "n_columns")

    def _sizes(self):
        return dict(t=self.n_targets, m=self.n_kept, m1=self.n_kept + 1, w=(self.n_columns + 15) // 16 + 2)

    def contain_tsv(self, tlen=None, host=None):
        """one line per input target: contig, length, state, new, host, host_pos, host_orient, mm, hits, root, root_pos, root_orient (tabs); tlen:
        the lengths of the targets of the call (by default read back from them); the text alga_hip --contain_layout= writes"""
        if tlen is None:
            tlen = self._source[2].cpu().numpy()
        return contain_tsv(host if host is not None else self.to_host(), tlen)


def contain_tsv(h, tlen):
    """the layout of a containment result read back (Kept.to_host())"""
    return "".join("%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%s\n" % (
        c, int(tlen[c]), int(h["state"][c]), int(h["new"][c]), int(h["host"][c]), int(h["host_pos"][c]), "-" if h["host_orient"][c] else "+", int(h["mm"][c]),
        int(h["hits"][c]), int(h["root"][c]), int(h["root_pos"][c]), "-" if h["root_orient"][c] else "+") for c in range(len(h["state"])))


STITCH_SELECTED, STITCH_HAS_OVERLAP, STITCH_AMBIGUOUS, STITCH_STITCHED, STITCH_DROPPED_CYCLE = 1, 2, 4, 8, 16   # bits of Stitched.j_state


class StitchParams(C.Structure):
    """alga_stitch_params"""
    _fields_ = [(k, C.c_int32) for k in ("max_mismatches", "min_overlap", "max_overlap", "slack", "flags")] + [("reserved", C.c_int32 * 3)]


class StitchInfo(_Info):
    """alga_stitch_info"""
    _fields_ = [(k, C.c_uint64) for k in ("entries", "selected", "with_overlap", "ambiguous", "hits_saturated", "candidates_outside_slack", "stitched", "dropped_cycle",
                                          "join_mismatches", "bases_removed", "longest_overlap", "contigs", "contigs_multi", "longest", "columns_before",
                                          "columns_after", "n50_before", "n50_after")] + \
               [(k, C.c_double) for k in ("ms_overlap", "ms_build", "ms_total")]


class StitchedC(C.Structure):
    """alga_stitched"""
    _fields_ = [(k, C.c_int64) for k in ("n_targets", "n_entries", "n_stitched", "n_members")] + [("n_columns", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("d_j_olen", "d_j_mm", "d_j_hits", "d_j_state", "d_end_entry", "d_stitched", "d_rank", "d_orient", "d_start", "d_overlap_after",
                                          "d_s_off", "d_s_members", "d_len", "d_col_off", "d_begin", "d_words")]


class Stitched(_RaggedResult):
    """Result of Engine.stitch / Engine.stitch_targets: zero-copy torch views of the engine's device memory (valid until the next stitch call on
    that engine; clone what has to live longer) -- per entry j_olen int32, j_mm / j_hits / j_state uint8 [n_entries]; end_entry int32
    [2 * n_targets]; per target stitched / rank int32, orient uint8, start int32 (the bits of uint32), overlap_after int32; s_off int32
    [n_stitched + 1], s_members int32 [n_members]; len int32 [n_stitched], col_off int32 [n_stitched + 1], begin int64 [n_stitched], words int32
    [(n_columns + 15) / 16 + 2] (the result's own copy of the bases) -- and .info (dict of alga_stitch_info)."""
    KEYS = (("j_olen", "<i4", np.int32, "j"), ("j_mm", "|u1", np.uint8, "j"), ("j_hits", "|u1", np.uint8, "j"), ("j_state", "|u1", np.uint8, "j"),
            ("end_entry", "<i4", np.int32, "e"), ("stitched", "<i4", np.int32, "t"), ("rank", "<i4", np.int32, "t"), ("orient", "|u1", np.uint8, "t"),
            ("start", "<i4", np.uint32, "t"), ("overlap_after", "<i4", np.int32, "t"), ("s_off", "<i4", np.uint32, "s1"), ("s_members", "<i4", np.int32, "sm"),
            ("len", "<i4", np.int32, "s"), ("col_off", "<i4", np.uint32, "s1"), ("begin", "<i8", np.uint64, "s"), ("words", "<i4", np.uint32, "w"))
    COUNTS = ("n_targets", "n_entries", "n_stitched", "n_members", "n_columns")

    def _sizes(self):
        return dict(j=self.n_entries, e=2 * self.n_targets, t=self.n_targets, s=self.n_stitched, s1=self.n_stitched + 1, sm=self.n_members,
                    w=(self.n_columns + 15) // 16 + 2)

    def stitch_tsv(self, tlen=None, host=None):
        """one line per member in (stitched, rank) order: stitched, rank, contig, orient, start, length, overlap_after, mm (tabs); tlen: the
        lengths of the targets that were stitched (by default read back from the targets of the call); the text alga_hip --stitch_layout= writes"""
        if tlen is None:
            tlen = self._source[2].cpu().numpy()
        return stitch_tsv(host if host is not None else self.to_host(), tlen)


def stitch_tsv(h, tlen):
    """the layout of a stitch result read back (Stitched.to_host())"""
    lines = []
    for j in range(len(h["len"])):
        for c in h["s_members"][int(h["s_off"][j]):int(h["s_off"][j + 1])]:
            c = int(c)
            out = 2 * c + (int(h["orient"][c]) ^ 1)
            lines.append("%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (j, int(h["rank"][c]), c, "-" if h["orient"][c] else "+", int(h["start"][c]), int(tlen[c]),
                                                             int(h["overlap_after"][c]), int(h["j_mm"][int(h["end_entry"][out])]) if h["overlap_after"][c] else 0))
    return "".join(lines)


GAPPED_MAX_READ = 1024                                           # ALGA_GAPPED_MAX_READ
GAPPED_PLACED, GAPPED_UNIQUE, GAPPED_MINUS, GAPPED_INDEL = 1, 2, 4, 8   # bits of Gapped.state
CIGAR_M, CIGAR_I, CIGAR_D = 0, 1, 2                              # the low two bits of a Gapped.cigar entry


class GappedParams(C.Structure):
    """alga_gapped_params"""
    _fields_ = [(k, C.c_int32) for k in ("k", "max_edits", "max_occ", "flags")] + [("reserved", C.c_int32 * 4)]


class GappedInfo(_Info):
    """alga_gapped_info"""
    _fields_ = [(k, C.c_uint64) for k in ("tried", "skipped_long", "placed", "unique", "with_indel", "edits", "insertions", "deletions", "candidates", "seeds",
                                          "seeds_over_max_occ")] + \
               [(k, C.c_double) for k in ("ms_index", "ms_place", "ms_trace", "ms_depth", "ms_total")]


class GappedC(C.Structure):
    """alga_gapped"""
    _fields_ = [("n_reads", C.c_int64), ("n_targets", C.c_int64), ("n_columns", C.c_uint64), ("n_cigar", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("d_target", "d_pos", "d_end", "d_edits", "d_state", "d_cigar_off", "d_cigar", "d_cover", "d_t_reads", "d_t_bases", "d_t_edits")]


class Gapped(_Result):
    """Result of Engine.place_gapped: zero-copy torch views of the engine's device memory (valid until the next Engine.place_gapped call on that
    engine; clone what has to live longer) -- target / pos / end int32 [n_reads], edits / state uint8 [n_reads], cigar_off int32 [n_reads + 1]
    and cigar int32 [n_cigar] (the bits of uint32: len << 2 | op), cover int32 [n_columns] (the bits of uint32), t_reads / t_bases / t_edits
    int64 [n_targets] -- and .info (dict of alga_gapped_info)."""
    KEYS = (("target", "<i4", np.int32, "r"), ("pos", "<i4", np.int32, "r"), ("end", "<i4", np.int32, "r"), ("edits", "|u1", np.uint8, "r"), ("state", "|u1", np.uint8, "r"),
            ("cigar_off", "<i4", np.uint32, "r1"), ("cigar", "<i4", np.uint32, "c"), ("cover", "<i4", np.uint32, "g"), ("t_reads", "<i8", np.uint64, "t"),
            ("t_bases", "<i8", np.uint64, "t"), ("t_edits", "<i8", np.uint64, "t"))
    COUNTS, KEPT = ("n_reads", "n_targets", "n_columns", "n_cigar"), "_placements"

    def _sizes(self):
        return dict(r=self.n_reads, r1=self.n_reads + 1, c=self.n_cigar, g=self.n_columns, t=self.n_targets)

    def cigar_strings(self, host=None):
        """the CIGAR of every read as text ('' where it is not placed), for example 57M1D93M"""
        return cigar_strings(host if host is not None else self.to_host())


def cigar_strings(h):
    """the scripts of a gapped result read back (Gapped.to_host())"""
    off = h["cigar_off"]
    return ["".join("%d%s" % (int(x) >> 2, "MID"[int(x) & 3]) for x in h["cigar"][int(off[r]):int(off[r + 1])]) for r in range(len(off) - 1)]


SAM_NAMES_DEPTH, SAM_SKIP_UNPLACED = 1, 2                         # alga_sam_params.flags


class PairParams(C.Structure):
    """alga_pair_params"""
    _fields_ = [("max_insert", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 6)]


class PairInfo(_Info):
    """alga_pair_info"""
    _fields_ = [(k, C.c_uint64) for k in ("reads", "live", "placed_h", "placed_g", "unplaced", "pairs", "pairs_proper", "pairs_improper", "pairs_split", "pairs_not_unique",
                                          "pairs_with_gapped", "proper_with_gapped")] + \
               [(k, C.c_int64) for k in ("insert_median", "insert_mean_x100")] + [(k, C.c_double) for k in ("ms_judge", "ms_total")]


class PairCallsC(C.Structure):
    """alga_pair_calls"""
    _fields_ = [("n_reads", C.c_int64), ("n_hist", C.c_int64), ("d_flag", C.c_void_p), ("d_tlen", C.c_void_p), ("d_insert_hist", C.c_void_p)]


class SamParams(C.Structure):
    """alga_sam_params"""
    _fields_ = [("flags", C.c_int32), ("reserved", C.c_int32 * 7)]


class PairCalls(_Result):
    """Result of Engine.judge_pairs: zero-copy torch views of the engine's device memory (valid until the next Engine.judge_pairs call on that
    engine; clone what has to live longer) -- flag int16 [n_reads] (the bits of uint16: the SAM FLAG), tlen int32 [n_reads], insert_hist int64
    [max_insert + 1] -- and .info (dict of alga_pair_info)."""
    KEYS = (("flag", "<i2", np.uint16, "r"), ("tlen", "<i4", np.int32, "r"), ("insert_hist", "<i8", np.uint64, "h"))
    COUNTS = ("n_reads", "n_hist")

    def _sizes(self):
        return dict(r=self.n_reads, h=self.n_hist)


IPOLISH_COUNTS = 1                                               # alga_ipolish_params.flags
IPOLISH_MAX_INS = 13                                            # ALGA_IPOLISH_MAX_INS
EVENT_S, EVENT_I, EVENT_D = 0, 1, 2                              # IndelPolished.ev_kind


class IpolishParams(C.Structure):
    """alga_ipolish_params"""
    _fields_ = [(k, C.c_int32) for k in ("min_cover", "min_percent", "max_ins", "flags")] + [("reserved", C.c_int32 * 4)]


class IpolishInfo(_Info):
    """alga_ipolish_info"""
    _fields_ = [(k, C.c_uint64) for k in ("columns", "voters_hamming", "voters_gapped", "votes", "del_votes", "ins_votes", "ins_too_long", "ins_edge", "shifted_runs",
                                          "shifted_bases", "voted_columns", "substituted", "deleted", "inserted_slots", "inserted_bases", "ambiguous_columns",
                                          "ambiguous_slots", "columns_after", "max_cover")] + \
               [(k, C.c_double) for k in ("ms_votes", "ms_inserts", "ms_build", "ms_total")]


class IpolishedC(C.Structure):
    """alga_ipolished"""
    _fields_ = [("n_targets", C.c_int64), ("n_columns_before", C.c_uint64), ("n_columns", C.c_uint64), ("n_events", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("d_len", "d_col_off", "d_begin", "d_words", "d_new_col", "d_ev_col", "d_ev_kind", "d_ev_len", "d_ev_bases", "d_ev_votes",
                                          "d_ev_cover", "d_t_subs", "d_t_dels", "d_t_ins_bases", "d_t_ambiguous", "d_counts", "d_span")]


class IndelPolished(_Result):
    """Result of Engine.polish_indels: zero-copy torch views of the engine's device memory (valid until the next Engine.polish_indels call but
    one on that engine -- the result is double-buffered; clone what has to live longer) -- len int32 [n_targets], col_off int32 [n_targets + 1]
    (the bits of uint32), begin int64 [n_targets], words int32 [(n_columns + 15) / 16 + 2], new_col int32 [n_columns_before + 1]; the events
    ev_col / ev_bases / ev_votes / ev_cover int32 and ev_kind / ev_len uint8 [n_events]; t_subs / t_dels / t_ins_bases / t_ambiguous int64
    [n_targets]; counts int32 [n_columns_before, 5] and span int32 [n_columns_before] or None -- and .info (dict of alga_ipolish_info)."""
    KEYS = (("len", "<i4", np.int32, "t"), ("col_off", "<i4", np.uint32, "t1"), ("begin", "<i8", np.uint64, "t"), ("words", "<i4", np.uint32, "w"),
            ("new_col", "<i4", np.uint32, "g1"), ("ev_col", "<i4", np.uint32, "e"), ("ev_kind", "|u1", np.uint8, "e"), ("ev_len", "|u1", np.uint8, "e"),
            ("ev_bases", "<i4", np.uint32, "e"), ("ev_votes", "<i4", np.uint32, "e"), ("ev_cover", "<i4", np.uint32, "e"), ("t_subs", "<i8", np.uint64, "t"),
            ("t_dels", "<i8", np.uint64, "t"), ("t_ins_bases", "<i8", np.uint64, "t"), ("t_ambiguous", "<i8", np.uint64, "t"))
    COUNTS = ("n_targets", "n_columns_before", "n_columns", "n_events")

    def __init__(self, c, info, device, source=None):
        super().__init__(c, info, device, source)
        self.counts = device_view(c.d_counts, (self.n_columns_before, 5), self._dev, "<i4") if c.d_counts else None
        self.span = device_view(c.d_span, (self.n_columns_before,), self._dev, "<i4") if c.d_span else None

    def _sizes(self):
        return dict(t=self.n_targets, t1=self.n_targets + 1, w=(self.n_columns + 15) // 16 + 2, g1=self.n_columns_before + 1, e=self.n_events)

    def to_host(self):
        d = super().to_host()
        if self.counts is not None:
            d["counts"] = self.counts.cpu().numpy().copy().view(np.uint32)
            d["span"] = self.span.cpu().numpy().copy().view(np.uint32)
        return d

    @property
    def targets(self):
        """(words, begin int64 [n_targets], len int32 [n_targets]): the new targets as the ragged target set Engine.place_reads(targets=...)
        takes (the tensors are the engine's)"""
        return self.words, self.begin, self.len


def library_path():
    return os.path.join(_HERE, "lib", "libalga_amd.so")


def source_fingerprint():
    """sha256 (first 16 hex digits) over the kernel / engine sources the library is built from (alga_amd/csrc/*, include/alga_amd.h):
    what profiles/ records next to a counter measurement, so that a number is only ever quoted for the code it was measured on.
    (The hash of the binary itself changes with the build directory.)"""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".hpp", ".cpp")) or f == "Makefile")
    files.append(os.path.join(os.path.dirname(_HERE), "include", "alga_amd.h"))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def load_library():
    """Load libalga_amd.so; raises AlgaError (never falls back to anything else) if it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 / libhsa-runtime64.  If the
    # system copy under /opt/rocm is initialised first, torch's copy later finds "No HIP GPUs".  Importing
    # torch first makes the loader resolve this library's NEEDED libamdhip64.so.7 to the copy already mapped.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise AlgaError(-2, "HIP extension %s is not built (run `python -c 'import __graft_entry__ as g; g.build()'`)" % path)
    lib = C.CDLL(path)
    lib.alga_abi_version.restype = C.c_int
    lib.alga_engine_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.alga_engine_destroy.argtypes = [C.c_void_p]
    lib.alga_engine_destroy.restype = None
    lib.alga_last_error.argtypes = [C.c_void_p]
    lib.alga_last_error.restype = C.c_char_p
    lib.alga_engine_device_name.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    lib.alga_engine_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    lib.alga_engine_reserve.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint64]
    lib.alga_prefsuf_default_params.argtypes = [C.POINTER(PrefSufParams)]
    lib.alga_prefsuf_default_params.restype = None
    lib.alga_prefsuf_build_host.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PrefSufParams),
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_free_edges.argtypes = [C.c_void_p, C.c_void_p]
    lib.alga_free_edges.restype = None
    lib.alga_prefsuf_build_host_compact.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PrefSufParams), C.POINTER(CompactEdges)]
    lib.alga_free_compact_edges.argtypes = [C.c_void_p, C.POINTER(CompactEdges)]
    lib.alga_free_compact_edges.restype = None
    lib.alga_host_alloc.argtypes = [C.c_void_p, C.c_size_t]
    lib.alga_host_alloc.restype = C.c_void_p
    lib.alga_host_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.alga_host_free.restype = None
    lib.alga_prefsuf_build_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PrefSufParams), C.c_void_p,
                                              C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_prefsuf_last_stats.argtypes = [C.c_void_p, C.POINTER(PrefSufStats)]
    lib.alga_prefsuf_discover_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PrefSufParams), C.c_int32,
                                                 C.c_int32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                 C.POINTER(C.c_uint64)]
    lib.alga_prefsuf_reduce_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PrefSufParams), C.c_void_p,
                                               C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p,
                                               C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_prefsuf_build_range_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PrefSufParams), C.c_int32, C.c_int32,
                                                    C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_shard_index_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PrefSufParams), C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.alga_shard_join_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_shard_small_keys_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_shard_resolve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.alga_shard_place_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_write_graph.argtypes = [C.c_char_p, C.c_int32, C.c_void_p, C.c_uint64]
    lib.alga_write_gfa_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.c_void_p, C.c_uint64, C.c_char_p, C.c_int32, C.POINTER(GfaInfo)]
    lib.alga_sort_records_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p,
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_sort_edges_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.alga_sort_u64_pairs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                               C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_double)]
    lib.alga_sort_u32_pairs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                               C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_double)]
    lib.alga_sort_desc_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_double)]
    lib.alga_pkb_shard_begin.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PkbParams), C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p]
    lib.alga_pkb_shard_round.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_pkb_shard_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.alga_pkb_shard_end.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_pkb_derive_params.argtypes = [C.c_double, C.c_float, C.c_double, C.c_int32, C.POINTER(PkbParams)]
    lib.alga_pkb_derive_params.restype = None
    lib.alga_can_align_batch_host.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PkbParams), C.c_void_p, C.c_uint64, C.c_void_p]
    lib.alga_li_kmers_host.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PkbParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.alga_pkb_supplement_host.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PkbParams), C.c_void_p, C.c_uint64,
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_pkb_supplement_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PkbParams), C.c_void_p, C.c_uint64, C.c_void_p,
                                               C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_pkb_last_stats.argtypes = [C.c_void_p, C.POINTER(PkbStats)]
    lib.alga_ingest_default_params.argtypes = [C.POINTER(IngestParams)]
    lib.alga_ingest_default_params.restype = None
    lib.alga_ingest_files.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(IngestParams), C.POINTER(NodeSet), C.c_char_p, C.c_size_t]
    lib.alga_free_node_set.argtypes = [C.POINTER(NodeSet)]
    lib.alga_free_node_set.restype = None
    lib.alga_parse_files.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(IngestParams), C.POINTER(ParsedReads), C.c_char_p, C.c_size_t]
    lib.alga_free_parsed_reads.argtypes = [C.POINTER(ParsedReads)]
    lib.alga_free_parsed_reads.restype = None
    lib.alga_preprocess_nodes.argtypes = [C.c_void_p, C.POINTER(PreprocessInput), C.POINTER(DeviceNodeSet)]
    lib.alga_copy_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.alga_contig_trim_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.alga_ingest_device.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(IngestParams), C.POINTER(DeviceNodeSet), C.POINTER(IngestInfo)]
    lib.alga_cut_triangles_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.alga_cut_triangles_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.alga_remove_dangling_branches_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p),
                                                         C.POINTER(C.c_uint64), C.POINTER(TipsInfo)]
    lib.alga_remove_short_parallel_paths_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p),
                                                            C.POINTER(C.c_uint64), C.POINTER(MstInfo)]
    lib.alga_unitigs_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.POINTER(UnitigsC),
                                        C.POINTER(UnitigInfo)]
    lib.alga_contigs_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(UnitigsC),
                                        C.POINTER(ContigInfo)]
    lib.alga_write_unitig_gfa_device.argtypes = [C.c_void_p, C.POINTER(UnitigsC), C.c_char_p, C.c_int32, C.POINTER(GfaInfo)]
    lib.alga_unitig_consensus_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(UnitigsC), C.c_int32, C.c_int32, C.c_void_p,
                                                 C.POINTER(ConsensusC), C.POINTER(ConsensusInfo)]
    lib.alga_write_consensus_fasta_device.argtypes = [C.c_void_p, C.POINTER(UnitigsC), C.POINTER(ConsensusC), C.c_char_p, C.c_int32, C.POINTER(GfaInfo)]
    lib.alga_contig_trim_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.alga_final_contigs_device.argtypes = [C.c_void_p, C.POINTER(UnitigsC), C.POINTER(ConsensusC), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                              C.POINTER(FinalContigsC), C.POINTER(FinalInfo)]
    lib.alga_extend_contigs_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.c_void_p, C.POINTER(UnitigsC), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_void_p, C.POINTER(UnitigsC), C.POINTER(ExtendInfo)]
    lib.alga_extend_seams_get.argtypes = [C.c_void_p, C.POINTER(UnitigsC), C.POINTER(ExtendSeamsC)]
    lib.alga_write_final_fasta_device.argtypes = [C.c_void_p, C.POINTER(UnitigsC), C.POINTER(ConsensusC), C.POINTER(FinalContigsC), C.c_char_p, C.POINTER(GfaInfo)]
    lib.alga_correct_default_params.argtypes = [C.POINTER(CorrectParams)]
    lib.alga_correct_default_params.restype = None
    lib.alga_correct_reads_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(CorrectParams), C.c_void_p, C.POINTER(CorrectInfo)]
    lib.alga_correct_parsed_reads.argtypes = [C.c_void_p, C.POINTER(ParsedReads), C.POINTER(CorrectParams), C.POINTER(CorrectInfo)]
    lib.alga_ingest_corrected_device.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(IngestParams), C.POINTER(CorrectParams), C.POINTER(DeviceNodeSet),
                                                 C.POINTER(IngestInfo), C.POINTER(CorrectInfo)]
    lib.alga_polish_default_params.argtypes = [C.POINTER(PolishParams)]
    lib.alga_polish_default_params.restype = None
    lib.alga_polish_placed_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PlacementsC), C.POINTER(PolishParams), C.c_void_p, C.POINTER(PolishedC),
                                              C.POINTER(PolishInfo)]
    lib.alga_write_polished_fasta_device.argtypes = [C.c_void_p, C.POINTER(UnitigsC), C.POINTER(ConsensusC), C.POINTER(FinalContigsC), C.POINTER(PlacementsC),
                                                     C.POINTER(PolishedC), C.c_int32, C.c_char_p, C.POINTER(GfaInfo)]
    lib.alga_scaffold_default_params.argtypes = [C.POINTER(ScaffoldParams)]
    lib.alga_scaffold_default_params.restype = None
    lib.alga_scaffold_placed_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.c_void_p, C.POINTER(PlacementsC), C.POINTER(ScaffoldParams), C.c_void_p,
                                                C.POINTER(ScaffoldsC), C.POINTER(ScaffoldInfo)]
    lib.alga_write_scaffold_fasta_device.argtypes = [C.c_void_p, C.POINTER(PlacementsC), C.POINTER(ScaffoldsC), C.POINTER(PolishedC), C.c_char_p, C.POINTER(GfaInfo)]
    lib.alga_break_default_params.argtypes = [C.POINTER(BreakParams)]
    lib.alga_break_default_params.restype = None
    lib.alga_break_placed_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.c_void_p, C.POINTER(PlacementsC), C.POINTER(PolishedC), C.POINTER(BreakParams), C.c_void_p,
                                             C.POINTER(BrokenC), C.POINTER(BreakInfo)]
    lib.alga_write_broken_fasta_device.argtypes = [C.c_void_p, C.POINTER(BrokenC), C.c_char_p, C.POINTER(GfaInfo)]
    lib.alga_grow_default_params.argtypes = [C.POINTER(GrowParams)]
    lib.alga_grow_default_params.restype = None
    lib.alga_grow_placed_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PlacementsC), C.POINTER(PolishedC), C.POINTER(GrowParams), C.c_void_p,
                                            C.POINTER(GrownC), C.POINTER(GrowInfo)]
    lib.alga_write_grown_fasta_device.argtypes = [C.c_void_p, C.POINTER(GrownC), C.c_char_p, C.POINTER(GfaInfo)]
    lib.alga_merge_default_params.argtypes = [C.POINTER(MergeParams)]
    lib.alga_merge_default_params.restype = None
    lib.alga_merge_targets_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MergeParams), C.c_void_p, C.POINTER(MergedC),
                                              C.POINTER(MergeInfo)]
    lib.alga_write_merged_fasta_device.argtypes = [C.c_void_p, C.POINTER(MergedC), C.c_char_p, C.POINTER(GfaInfo)]
    lib.alga_contain_default_params.argtypes = [C.POINTER(ContainParams)]
    lib.alga_contain_default_params.restype = None
    lib.alga_drop_contained_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(ContainParams), C.c_void_p, C.POINTER(KeptC),
                                               C.POINTER(ContainInfo)]
    lib.alga_write_kept_fasta_device.argtypes = [C.c_void_p, C.POINTER(KeptC), C.c_char_p, C.POINTER(GfaInfo)]
    lib.alga_stitch_default_params.argtypes = [C.POINTER(StitchParams)]
    lib.alga_stitch_default_params.restype = None
    lib.alga_stitch_targets_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                               C.POINTER(StitchParams), C.c_void_p, C.POINTER(StitchedC), C.POINTER(StitchInfo)]
    lib.alga_stitch_scaffolds_device.argtypes = [C.c_void_p, C.POINTER(PlacementsC), C.POINTER(ScaffoldsC), C.POINTER(PolishedC), C.POINTER(StitchParams), C.c_void_p,
                                                 C.POINTER(StitchedC), C.POINTER(StitchInfo)]
    lib.alga_write_stitched_fasta_device.argtypes = [C.c_void_p, C.POINTER(StitchedC), C.c_char_p, C.POINTER(GfaInfo)]
    lib.alga_gapped_default_params.argtypes = [C.POINTER(GappedParams)]
    lib.alga_gapped_default_params.restype = None
    lib.alga_place_gapped_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(PlacementsC), C.POINTER(GappedParams),
                                             C.c_void_p, C.POINTER(GappedC), C.POINTER(GappedInfo)]
    lib.alga_write_gapped_tsv_device.argtypes = [C.c_void_p, C.POINTER(GappedC), C.c_char_p, C.POINTER(GfaInfo)]
    lib.alga_ipolish_default_params.argtypes = [C.POINTER(IpolishParams)]
    lib.alga_ipolish_default_params.restype = None
    lib.alga_polish_indels_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PlacementsC), C.POINTER(GappedC), C.POINTER(IpolishParams), C.c_void_p,
                                              C.POINTER(IpolishedC), C.POINTER(IpolishInfo)]
    lib.alga_write_ipolished_fasta_device.argtypes = [C.c_void_p, C.POINTER(IpolishedC), C.c_char_p, C.POINTER(GfaInfo)]
    lib.alga_write_ipolish_events_tsv_device.argtypes = [C.c_void_p, C.POINTER(IpolishedC), C.c_char_p, C.POINTER(GfaInfo)]
    lib.alga_pair_default_params.argtypes = [C.POINTER(PairParams)]
    lib.alga_pair_default_params.restype = None
    lib.alga_judge_pairs_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.c_void_p, C.POINTER(PlacementsC), C.POINTER(GappedC), C.POINTER(PairParams), C.c_void_p,
                                            C.POINTER(PairCallsC), C.POINTER(PairInfo)]
    lib.alga_write_sam_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PlacementsC), C.POINTER(GappedC), C.POINTER(PairCallsC), C.POINTER(SamParams), C.c_char_p,
                                          C.POINTER(GfaInfo)]
    _LIB = lib
    return lib


def ingest_files(file1, file2=None, threads=1, **kw):
    """Host input stages (C++, alga_amd/host/ingest.cpp) through the C ABI -> dict with numpy copies."""
    lib = load_library()
    p = IngestParams()
    lib.alga_ingest_default_params(C.byref(p))
    p.threads = int(threads)
    for k, v in kw.items():
        setattr(p, k, v)
    ns = NodeSet()
    err = C.create_string_buffer(512)
    rc = lib.alga_ingest_files(file1.encode(), (file2 or "").encode() or None, C.byref(p), C.byref(ns), err, 512)
    if rc:
        raise AlgaError(rc, err.value.decode())
    n, st = ns.n, ns.stride_words
    out = dict(n=n, stride=st,
               words=np.ctypeslib.as_array(ns.words, shape=(max(n, 1) * st,))[: n * st].reshape(n, st).copy(),
               len=np.ctypeslib.as_array(ns.len, shape=(max(n, 1),))[:n].copy(),
               pair_off=np.ctypeslib.as_array(ns.pair_off, shape=(max(n, 1),))[:n].copy(),
               LEN=ns.LEN, min_overlap=ns.min_overlap, rsoemo=ns.rsoemo, li_kmer_length=ns.li_kmer_length, records=ns.records,
               removed_n=ns.removed_n, removed_str=ns.removed_str, removed_prefix=ns.removed_prefix, removed_short=ns.removed_short)
    lib.alga_free_node_set(C.byref(ns))
    return out


def parse_files(file1, file2=None, threads=1, **kw):
    """Stage 1 of the input (C++ host): every record's two nodes in node order, before duplicate / prefix removal.
    -> dict(rows[2R, stride] u32, len[2R] i32 (-1 removed), params); numpy copies."""
    lib = load_library()
    p = IngestParams()
    lib.alga_ingest_default_params(C.byref(p))
    p.threads = int(threads)
    for k, v in kw.items():
        setattr(p, k, v)
    pr = ParsedReads()
    err = C.create_string_buffer(512)
    rc = lib.alga_parse_files(file1.encode(), (file2 or "").encode() or None, C.byref(p), C.byref(pr), err, 512)
    if rc:
        raise AlgaError(rc, err.value.decode())
    n, st = int(pr.n_nodes), int(pr.stride_words)
    out = dict(n_nodes=n, stride=st, rows=np.ctypeslib.as_array(pr.rows, shape=(max(n, 1) * st,))[: n * st].reshape(n, st).copy(),
               len=np.ctypeslib.as_array(pr.len, shape=(max(n, 1),))[:n].copy(), paired=bool(pr.paired), records=pr.records,
               removed_n=pr.removed_n, removed_str=pr.removed_str, LEN=pr.LEN, min_overlap=pr.min_overlap, rsoemo=pr.rsoemo,
               li_kmer_length=pr.li_kmer_length, avg_len=pr.avg_len, remove_pref_reads=int(p.remove_pref_reads))
    lib.alga_free_parsed_reads(C.byref(pr))
    return out


def pack_reads(codes, lens=None, stride_words=None):
    """codes[n, maxlen] uint8 in {0,1,2,3} (A C G T) -> words[n, stride] uint32 in the reference's layout
    (nucleotide i in bits 2i,2i+1 of a little-endian bit string; src/DataStructures/Read.cpp:40-68)."""
    codes = np.asarray(codes, dtype=np.uint8)
    n, m = codes.shape
    W = (2 * m + 31) // 32
    if stride_words is None:
        stride_words = W
    out = np.zeros((n, stride_words), dtype=np.uint32)
    shifts = (2 * np.arange(16, dtype=np.uint32))[None, None, :]
    lens = None if lens is None else np.asarray(lens)
    CH = 1 << 18                                                   # bounded temporaries (64 B of uint32 per nucleotide row chunk)
    for s0 in range(0, n, CH):
        c = codes[s0:s0 + CH]
        if lens is not None:
            c = np.where(np.arange(m)[None, :] < lens[s0:s0 + CH, None], c, 0).astype(np.uint8)
        pad = W * 16 - m
        if pad:
            c = np.concatenate([c, np.zeros((c.shape[0], pad), np.uint8)], axis=1)
        c = c.reshape(c.shape[0], W, 16).astype(np.uint32)
        out[s0:s0 + CH, :W] = np.bitwise_or.reduce(c << shifts, axis=2)
    return out


def derive_params(avg_len, trim_left=3, trim_right=3, scale=0.55):
    """(min_overlap, rsoe_min_overlap) as src/main.cpp:93-108 of the reference derives them
    (mixed float/int arithmetic with truncation, reproduced literally in float32)."""
    LEN = int(avg_len + trim_left + trim_right)
    sc = np.float32(scale)
    L = int(np.float32(LEN) * sc)
    rsoemo = int(np.float32(LEN) * (sc + np.float32(1)) / np.float32(2))
    return L, rsoemo


REDUCTION = {"auto": 0, "per_target": 1, "source_side": 2}     # alga_reduction
ERR_UNSUPPORTED = -7


class Engine:
    """One engine handle == one HIP device.  Mirrors the reference's GraphCreator life cycle:
    construct -> (setAlignFrom/To masks) -> build -> read the graph."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.alga_engine_create(int(device), C.byref(h))
        if rc:
            raise AlgaError(rc, "alga_engine_create(device=%d) failed -- no usable HIP device" % device)
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.alga_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise AlgaError(rc, (self._lib.alga_last_error(self._h) or b"").decode())

    def set_option(self, name, value):
        """alga_engine_set_option: "probe" ("auto" | "table" | "cluster"), "cluster_bucket_bias", "cluster_pairs", "cluster_order",
        "local_big_max", "auto_reduction_per_target", "mst_mid_nodes", ... (the list is in include/alga_amd.h)."""
        if name == "probe" and isinstance(value, str):
            value = PROBE[value]
        self._check(self._lib.alga_engine_set_option(self._h, name.encode(), int(value)))

    def reserve(self, n_nodes, max_len, min_overlap, n_edges_hint=0):
        """alga_engine_reserve: every device buffer of a build for this shape, ahead of the build."""
        self._check(self._lib.alga_engine_reserve(self._h, int(n_nodes), int(max_len), int(min_overlap), int(n_edges_hint)))

    def device_name(self):
        buf = C.create_string_buffer(256)
        self._lib.alga_engine_device_name(self._h, buf, 256)
        return buf.value.decode()

    @staticmethod
    def params(min_overlap, rsoe_min_overlap, collect_stats=False, reduction="auto"):
        p = PrefSufParams()
        load_library().alga_prefsuf_default_params(C.byref(p))
        p.min_overlap, p.rsoe_min_overlap, p.collect_stats = int(min_overlap), int(rsoe_min_overlap), int(bool(collect_stats))
        p.reduction = REDUCTION[reduction] if isinstance(reduction, str) else int(reduction)
        return p

    def last_stats(self):
        st = PrefSufStats()
        self._check(self._lib.alga_prefsuf_last_stats(self._h, C.byref(st)))
        return st.as_dict()

    # ---- duplicate / prefix-read removal + id compaction on the GPU ---------------------------
    def preprocess_nodes(self, rows, lens, remove_pref_reads=2, min_keep_len=0):
        """rows[2R, stride] u32 / lens[2R] i32 (-1 = removed) on the host -> DeviceNodeSet (device pointers, engine-owned)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = int(lens.shape[0])
        inp = PreprocessInput(rows.ctypes.data, int(rows.shape[1]) if rows.ndim == 2 else 1, lens.ctypes.data, n, int(remove_pref_reads), int(min_keep_len))
        out = DeviceNodeSet()
        self._check(self._lib.alga_preprocess_nodes(self._h, C.byref(inp), C.byref(out)))
        return out

    def ingest_device(self, file1, file2=None, correct=None, **kw):
        """The whole input stage on the GPU (alga_ingest_device): files -> (DeviceNodeSet, info dict); raises AlgaError -7 for the
        inputs that stage does not take (file types other than .fasta / .fastq / .fq, remove_reads_with_n = 0).
        correct: a dict of k / solid_min / min_run (any subset; {} = the defaults) -- the reads are corrected between the parse kernels and
        the removals (alga_ingest_corrected_device), and the info dict gets the correction's counters under "correct"."""
        p = IngestParams()
        self._lib.alga_ingest_default_params(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        ds, info = DeviceNodeSet(), IngestInfo()
        f1, f2 = file1.encode(), (file2 or "").encode() or None
        if correct is None:
            self._check(self._lib.alga_ingest_device(self._h, f1, f2, C.byref(p), C.byref(ds), C.byref(info)))
            return ds, {k: getattr(info, k) for k, _ in IngestInfo._fields_}
        cp, ci = self.correct_params(**correct), CorrectInfo()
        self._check(self._lib.alga_ingest_corrected_device(self._h, f1, f2, C.byref(p), C.byref(cp), C.byref(ds), C.byref(info), C.byref(ci)))
        d = {k: getattr(info, k) for k, _ in IngestInfo._fields_}
        d["correct"] = ci.as_dict()
        return ds, d

    # ---- read error correction by the k-mer spectrum (the definition: include/alga_amd.h) -----
    @staticmethod
    def correct_params(k=21, solid_min=3, min_run=1):
        return CorrectParams(int(k), int(solid_min), int(min_run), 0)

    def correct_reads(self, rows, lens, k=21, solid_min=3, min_run=1):
        """rows[2R, stride] u32 / lens[2R] i32 in the parser's layout on the host (alga_correct_parsed_reads) -> (new rows, info dict);
        the arguments are not modified."""
        rows = np.array(rows, dtype=np.uint32, order="C", copy=True)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = int(lens.shape[0])
        rows = rows.reshape(n, -1) if n else rows.reshape(0, rows.shape[1] if rows.ndim == 2 else 1)
        pr = ParsedReads()
        pr.n_nodes, pr.stride_words = n, int(rows.shape[1])
        pr.rows = rows.ctypes.data_as(C.POINTER(C.c_uint32))
        pr.len = lens.ctypes.data_as(C.POINTER(C.c_int32))
        cp, ci = self.correct_params(k, solid_min, min_run), CorrectInfo()
        self._check(self._lib.alga_correct_parsed_reads(self._h, C.byref(pr), C.byref(cp), C.byref(ci)))
        return rows, ci.as_dict()

    def correct_reads_device(self, rows_t, lens_t, k=21, solid_min=3, min_run=1, stream=None):
        """rows_t int32 [2R, stride] / lens_t int32 [2R]: contiguous torch device tensors in the parser's layout, corrected in place
        (alga_correct_reads_device) -> info dict"""
        import torch
        assert rows_t.dtype == torch.int32 and lens_t.dtype == torch.int32 and rows_t.is_contiguous() and lens_t.is_contiguous()
        n = int(lens_t.shape[0])
        assert rows_t.dim() == 2 and int(rows_t.shape[0]) == n
        torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()
        cp, ci = self.correct_params(k, solid_min, min_run), CorrectInfo()
        self._check(self._lib.alga_correct_reads_device(self._h, _ptr(rows_t), int(rows_t.shape[1]), _ptr(lens_t), n, C.byref(cp),
                                                        C.c_void_p(stream) if stream else None, C.byref(ci)))
        return ci.as_dict()

    # ---- host buffers in, edges out (the drop-in call) --------------------------------------
    def prefsuf_host(self, words, lens, min_overlap, rsoe_min_overlap, align_from=None, align_to=None, collect_stats=False,
                     reduction="auto", twin_rows=False):
        """twin_rows: `words` holds the rows of the ODD nodes alone (n / 2 rows; alga_prefsuf_params.twin_rows)."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = int(lens.shape[0])
        stride = int(words.shape[1]) if words.ndim == 2 else (words.size // max(n // 2 if twin_rows else n, 1))
        keep = [words, lens]
        nd = _Nodes(words.ctypes.data, stride, lens.ctypes.data, n, None, None)
        if align_from is not None:
            af = np.ascontiguousarray(align_from, dtype=np.uint8); keep.append(af); nd.align_from = af.ctypes.data
        if align_to is not None:
            at = np.ascontiguousarray(align_to, dtype=np.uint8); keep.append(at); nd.align_to = at.ctypes.data
        p = self.params(min_overlap, rsoe_min_overlap, collect_stats, reduction)
        p.twin_rows = 1 if twin_rows else 0
        out = C.c_void_p()
        m = C.c_uint64()
        self._check(self._lib.alga_prefsuf_build_host(self._h, C.byref(nd), C.byref(p), C.byref(out), C.byref(m)))
        try:
            e = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int32)), shape=(max(m.value, 1) * 3,))[: m.value * 3]
            return e.reshape(-1, 3).copy()
        finally:
            self._lib.alga_free_edges(self._h, out)

    def host_array(self, shape, dtype):
        """numpy array over pinned host memory (alga_host_alloc); released when the array's base object goes (alga_host_free)"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self._lib.alga_host_alloc(self._h, n)
        if not p:
            raise AlgaError(-1, (self._lib.alga_last_error(self._h) or b"").decode())
        lib, h = self._lib, self._h

        class _Owner:
            def __del__(self_inner):
                lib.alga_host_free(h, p)
        buf = (C.c_char * n).from_address(p)
        buf._owner = _Owner()
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def prefsuf_host_compact(self, words, lens, min_overlap, rsoe_min_overlap, twin_rows=False, repeat=1, as_triples=True):
        """alga_prefsuf_build_host_compact -> (edges int32[m, 3] rebuilt from the compact form (or None), best seconds of the C call alone)"""
        import time
        words = np.ascontiguousarray(words, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = int(lens.shape[0])
        nd = _Nodes(words.ctypes.data, int(words.shape[1]), lens.ctypes.data, n, None, None)
        p = self.params(min_overlap, rsoe_min_overlap)
        p.twin_rows = 1 if twin_rows else 0
        best, edges = None, None
        for it in range(repeat):
            out = CompactEdges()
            t = time.perf_counter()
            self._check(self._lib.alga_prefsuf_build_host_compact(self._h, C.byref(nd), C.byref(p), C.byref(out)))
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
            if it == repeat - 1 and as_triples:
                m = int(out.n_edges)
                deg = np.ctypeslib.as_array(C.cast(out.degree, C.POINTER(C.c_uint8)), shape=(n,)) if n else np.zeros(0, np.uint8)
                edges = np.empty((m, 3), dtype=np.int32)
                if m:
                    edges[:, 0] = np.repeat(np.arange(n, dtype=np.int32), deg)
                    edges[:, 1] = np.ctypeslib.as_array(C.cast(out.dst, C.POINTER(C.c_uint32)), shape=(m,)).view(np.int32)
                    edges[:, 2] = np.ctypeslib.as_array(C.cast(out.offset, C.POINTER(C.c_uint8)), shape=(m,))
            self._lib.alga_free_compact_edges(self._h, C.byref(out))
        return edges, best

    def prefsuf_host_timed(self, words, lens, min_overlap, rsoe_min_overlap, repeat=3, twin_rows=False, digest=False):
        """Wall time of the C call alone (alga_prefsuf_build_host + alga_free_edges; no Python-side copy of the result):
        -> (best seconds, n_edges, digest).  twin_rows: `words` holds the rows of the odd nodes alone (alga_prefsuf_params.twin_rows).
        digest: [count, position-weighted checksum] of the last repeat's host list (host_edges_digest; outside the timing), else None."""
        import time
        words = np.ascontiguousarray(words, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = int(lens.shape[0])
        nd = _Nodes(words.ctypes.data, int(words.shape[1]), lens.ctypes.data, n, None, None)
        p = self.params(min_overlap, rsoe_min_overlap)
        p.twin_rows = 1 if twin_rows else 0
        best, m_out, dg = None, 0, None
        for it in range(repeat):
            out, m = C.c_void_p(), C.c_uint64()
            t = time.perf_counter()
            self._check(self._lib.alga_prefsuf_build_host(self._h, C.byref(nd), C.byref(p), C.byref(out), C.byref(m)))
            dt = time.perf_counter() - t
            if digest and it == repeat - 1:
                dg = host_edges_digest(np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int32)), shape=(int(m.value), 3))) if m.value else [0, 0]
            self._lib.alga_free_edges(self._h, out)
            best = dt if best is None else min(best, dt)
            m_out = int(m.value)
        return best, m_out, dg

    # ---- device-resident node set (torch tensors on this engine's device) --------------------
    @staticmethod
    def _nodes_from_torch(words, lens, align_from=None, align_to=None):
        assert words.is_cuda and lens.is_cuda and words.is_contiguous() and lens.is_contiguous()
        n = int(lens.shape[0])
        stride = int(words.shape[1])
        nd = _Nodes(words.data_ptr(), stride, lens.data_ptr(), n, None, None)
        if align_from is not None:
            nd.align_from = align_from.data_ptr()
        if align_to is not None:
            nd.align_to = align_to.data_ptr()
        return nd

    def prefsuf_device(self, words, lens, min_overlap, rsoe_min_overlap, align_from=None, align_to=None, stream=None,
                       collect_stats=False, reduction="auto"):
        """words: int32/uint32-viewed torch tensor [n, stride] on the device, lens: int32 [n].
        Returns (device pointer of alga_edge[n_edges], n_edges); the memory belongs to the engine."""
        nd = self._nodes_from_torch(words, lens, align_from, align_to)
        p = self.params(min_overlap, rsoe_min_overlap, collect_stats, reduction)
        out = C.c_void_p()
        m = C.c_uint64()
        self._check(self._lib.alga_prefsuf_build_device(self._h, C.byref(nd), C.byref(p), C.c_void_p(stream or 0),
                                                        C.byref(out), C.byref(m)))
        return out.value, int(m.value)

    def keys_device(self, words, lens, min_overlap, rsoe_min_overlap, node_begin, node_end, align_from=None, align_to=None, stream=None, want_meta_flag=False):
        """Minimizer keys + runs of the nodes [node_begin, node_end) -> (d_keys ptr, d_meta ptr) over all n nodes (this range
        filled; the caller all-gathers the rest in place), or None when the clustered probe does not take the input."""
        nd = self._nodes_from_torch(words, lens, align_from, align_to)
        p = self.params(min_overlap, rsoe_min_overlap, False)
        out = NodeKeys()
        self._check(self._lib.alga_prefsuf_keys_device(self._h, C.byref(nd), C.byref(p), int(node_begin), int(node_end), C.c_void_p(stream or 0),
                                                       C.byref(out)))
        if not out.eligible:
            return None
        if want_meta_flag:
            return out.d_keys, out.d_meta, bool(out.meta_needed)
        return out.d_keys, out.d_meta

    def build_range_device(self, words, lens, min_overlap, rsoe_min_overlap, src_begin, src_end, align_from=None, align_to=None,
                           stream=None, collect_stats=False, keys_shared=False):
        """Final edges of the sources [src_begin, src_end) by the source-side reduction -> (ptr, n_edges), or None when
        that form is not exact for the input (ALGA_ERR_UNSUPPORTED): the caller then takes discover/exchange/reduce.
        keys_shared: 1/True = keys_device + the all-gather of its arrays came first; 2 = reuse the entry array of the previous build
        of the same node set (include/alga_amd.h)."""
        nd = self._nodes_from_torch(words, lens, align_from, align_to)
        p = self.params(min_overlap, rsoe_min_overlap, collect_stats)
        p.keys_shared = int(keys_shared)
        out = C.c_void_p()
        m = C.c_uint64()
        rc = self._lib.alga_prefsuf_build_range_device(self._h, C.byref(nd), C.byref(p), int(src_begin), int(src_end),
                                                       C.c_void_p(stream or 0), C.byref(out), C.byref(m))
        if rc == ERR_UNSUPPORTED:
            return None
        self._check(rc)
        return out.value, int(m.value)

    # ---- the bucket-sharded N-GPU form, phase by phase (include/alga_amd.h: alga_shard_*); None = ALGA_ERR_UNSUPPORTED ----
    def shard_index_device(self, words, lens, min_overlap, rsoe_min_overlap, rank, n_ranks, align_from=None, align_to=None, stream=None):
        """-> (d_desc ptr [3 x u32 per descriptor], counts[n_ranks], offsets[n_ranks]) after keys_device + the key all-gather."""
        nd = self._nodes_from_torch(words, lens, align_from, align_to)
        p = self.params(min_overlap, rsoe_min_overlap, False)
        out = C.c_void_p()
        cnt, off = (C.c_uint64 * n_ranks)(), (C.c_uint64 * n_ranks)()
        rc = self._lib.alga_shard_index_device(self._h, C.byref(nd), C.byref(p), int(rank), int(n_ranks), C.c_void_p(stream or 0), C.byref(out), cnt, off)
        if rc == ERR_UNSUPPORTED:
            return None
        self._check(rc)
        return out.value, [int(x) for x in cnt], [int(x) for x in off]

    def shard_join_device(self, words, lens, desc_in, n_desc, align_from=None, align_to=None, stream=None):
        """desc_in: device tensor / pointer of n_desc received descriptors -> (d_pending_src ptr [u32], n_pending) or None."""
        nd = self._nodes_from_torch(words, lens, align_from, align_to)
        out, m = C.c_void_p(), C.c_uint64()
        rc = self._lib.alga_shard_join_device(self._h, C.byref(nd), C.c_void_p(_ptr(desc_in)), C.c_uint64(int(n_desc)), C.c_void_p(stream or 0), C.byref(out), C.byref(m))
        if rc == ERR_UNSUPPORTED:
            return None
        self._check(rc)
        return out.value, int(m.value)

    def shard_small_keys_device(self, pending_all, n_all, stream=None):
        out, m = C.c_void_p(), C.c_uint64()
        self._check(self._lib.alga_shard_small_keys_device(self._h, C.c_void_p(_ptr(pending_all)), C.c_uint64(int(n_all)), C.c_void_p(stream or 0), C.byref(out), C.byref(m)))
        return out.value, int(m.value)

    def shard_resolve_device(self, small_all, n_small_all, n_ranks, stream=None):
        """-> (d_edges ptr, counts[n_ranks], offsets[n_ranks]): final edges grouped by the rank that owns the source id"""
        out = C.c_void_p()
        cnt, off = (C.c_uint64 * n_ranks)(), (C.c_uint64 * n_ranks)()
        self._check(self._lib.alga_shard_resolve_device(self._h, C.c_void_p(_ptr(small_all)), C.c_uint64(int(n_small_all)), C.c_void_p(stream or 0), C.byref(out), cnt, off))
        return out.value, [int(x) for x in cnt], [int(x) for x in off]

    def shard_place_device(self, edges_in, n_in, src_begin, src_end, stream=None):
        out, m = C.c_void_p(), C.c_uint64()
        self._check(self._lib.alga_shard_place_device(self._h, C.c_void_p(_ptr(edges_in)), C.c_uint64(int(n_in)), int(src_begin), int(src_end), C.c_void_p(stream or 0),
                                                      C.byref(out), C.byref(m)))
        return out.value, int(m.value)

    def shard_stats(self):
        st = ShardStats()
        self._lib.alga_shard_last_stats.argtypes = [C.c_void_p, C.POINTER(ShardStats)]
        self._lib.alga_shard_last_stats(self._h, C.byref(st))
        return st.as_dict()

    def discover_device(self, words, lens, min_overlap, rsoe_min_overlap, src_begin, src_end, align_from=None,
                        align_to=None, stream=None, collect_stats=False):
        """-> (d_dst ptr [u32], d_val ptr [u64], n_record_slots); slots with dst == 0xFFFFFFFF are padding."""
        nd = self._nodes_from_torch(words, lens, align_from, align_to)
        p = self.params(min_overlap, rsoe_min_overlap, collect_stats)
        d, v = C.c_void_p(), C.c_void_p()
        m = C.c_uint64()
        self._check(self._lib.alga_prefsuf_discover_device(self._h, C.byref(nd), C.byref(p), int(src_begin), int(src_end),
                                                           C.c_void_p(stream or 0), C.byref(d), C.byref(v), C.byref(m)))
        return d.value, v.value, int(m.value)

    def reduce_device(self, words, lens, min_overlap, rsoe_min_overlap, rec_dst, rec_val, n_records, dst_begin,
                      dst_end, align_from=None, align_to=None, stream=None, collect_stats=False):
        """rec_dst (int32) / rec_val (int64): device pointers (ints) or torch tensors."""
        nd = self._nodes_from_torch(words, lens, align_from, align_to)
        p = self.params(min_overlap, rsoe_min_overlap, collect_stats)

        def ptr(x):
            return C.c_void_p(x if isinstance(x, int) else x.data_ptr())
        out = C.c_void_p()
        m = C.c_uint64()
        self._check(self._lib.alga_prefsuf_reduce_device(self._h, C.byref(nd), C.byref(p), ptr(rec_dst), ptr(rec_val),
                                                         int(n_records), int(dst_begin), int(dst_end),
                                                         C.c_void_p(stream or 0), C.byref(out), C.byref(m)))
        return out.value, int(m.value)

    def sort_records_device(self, rec_dst, rec_val, n_records, n_nodes, stream=None):
        """-> (d_dst_sorted ptr, d_val_sorted ptr, n_valid): records ordered by target id, padding dropped."""
        def ptr(x):
            return C.c_void_p(x if isinstance(x, int) else x.data_ptr())
        d, v = C.c_void_p(), C.c_void_p()
        m = C.c_uint64()
        self._check(self._lib.alga_sort_records_device(self._h, ptr(rec_dst), ptr(rec_val), int(n_records), int(n_nodes),
                                                       C.c_void_p(stream or 0), C.byref(d), C.byref(v), C.byref(m)))
        return d.value, v.value, int(m.value)

    def sort_u32_pairs_device(self, keys, vals, begin_bit=0, own=True, repeat=1, stream=None):
        """alga_sort_u32_pairs_device: (key, value) int32 / uint32 tensors on this device, stable on the key bits [begin_bit, 32) ->
        (keys ptr, vals ptr, best ms).  own: the engine's radix sort (radix_sort.hip), else rocPRIM's.  vals None (own only): the values are
        0, 1, 2, ..."""
        n = int(keys.shape[0])
        ko, vo, ms = C.c_void_p(), C.c_void_p(), C.c_double()
        self._check(self._lib.alga_sort_u32_pairs_device(self._h, keys.data_ptr() if n else None, vals.data_ptr() if n and vals is not None else None, n, int(begin_bit), int(bool(own)),
                                                         int(repeat), C.c_void_p(stream or 0), C.byref(ko), C.byref(vo), C.byref(ms)))
        return ko.value, vo.value, ms.value

    def sort_u64_pairs_device(self, keys, vals, bits, own=True, repeat=1, stream=None):
        """alga_sort_u64_pairs_device: (key, value) int64 tensors on this device, stable on the key bits [0, bits) -> (keys ptr, vals ptr, best ms)"""
        n = int(keys.shape[0])
        ko, vo, ms = C.c_void_p(), C.c_void_p(), C.c_double()
        self._check(self._lib.alga_sort_u64_pairs_device(self._h, keys.data_ptr() if n else None, vals.data_ptr() if n else None, n, int(bits), int(bool(own)),
                                                         int(repeat), C.c_void_p(stream or 0), C.byref(ko), C.byref(vo), C.byref(ms)))
        return ko.value, vo.value, ms.value

    def sort_desc_device(self, keys, vals, begin_bit, end_bit, own=True, repeat=1, stream=None):
        """alga_sort_desc_device: int32 / uint32 keys and int64 values on this device, stable on the key bits [begin_bit, end_bit) (a window that is
        not one: [0, 32)) -> (keys ptr, vals ptr, best ms)"""
        n = int(keys.shape[0])
        ko, vo, ms = C.c_void_p(), C.c_void_p(), C.c_double()
        self._check(self._lib.alga_sort_desc_device(self._h, keys.data_ptr() if n else None, vals.data_ptr() if n else None, n, int(begin_bit), int(end_bit),
                                                    int(bool(own)), int(repeat), C.c_void_p(stream or 0), C.byref(ko), C.byref(vo), C.byref(ms)))
        return ko.value, vo.value, ms.value

    def sort_edges_device(self, edges, n_edges, n_nodes, stream=None):
        """edges: device pointer or int32 tensor [n_edges, 3] -> device pointer of the list ordered by (src, dst)."""
        p = C.c_void_p(edges if isinstance(edges, int) else edges.data_ptr())
        out = C.c_void_p()
        self._check(self._lib.alga_sort_edges_device(self._h, p, int(n_edges), int(n_nodes), C.c_void_p(stream or 0), C.byref(out)))
        return out.value

    # ---- approximate supplement ---------------------------------------------------------------
    @staticmethod
    def pkb_params(avg_len, error_rate, kmer_length_bucket, scale=0.55):
        p = PkbParams()
        load_library().alga_pkb_derive_params(float(avg_len), float(scale), float(error_rate), int(kmer_length_bucket), C.byref(p))
        return p

    @staticmethod
    def _host_nodes(words, lens):
        words = np.ascontiguousarray(words, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = int(lens.shape[0])
        stride = int(words.shape[1]) if words.ndim == 2 else (words.size // max(n, 1))
        return _Nodes(words.ctypes.data, stride, lens.ctypes.data, n, None, None), (words, lens)

    def can_align_batch(self, words, lens, triples, p):
        nd, keep = self._host_nodes(words, lens)
        t = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
        out = np.zeros(len(t), dtype=np.uint8)
        self._check(self._lib.alga_can_align_batch_host(self._h, C.byref(nd), C.byref(p), t.ctypes.data, len(t), out.ctypes.data))
        return out

    def li_kmers(self, words, lens, p, prio):
        nd, keep = self._host_nodes(words, lens)
        n, I = nd.n, p.li_intervals
        h = np.zeros((n, I), dtype=np.uint64)
        ind = np.zeros((n, I), dtype=np.int32)
        cnt = np.zeros(n, dtype=np.int32)
        pr = np.ascontiguousarray(prio, dtype=np.int32)
        self._check(self._lib.alga_li_kmers_host(self._h, C.byref(nd), C.byref(p), pr.ctypes.data, h.ctypes.data, ind.ctypes.data, cnt.ctypes.data))
        return h, ind, cnt

    def pkb_supplement_host(self, words, lens, edges_in, p):
        nd, keep = self._host_nodes(words, lens)
        e = np.ascontiguousarray(edges_in, dtype=np.int32).reshape(-1, 3)
        out = C.c_void_p()
        m = C.c_uint64()
        self._check(self._lib.alga_pkb_supplement_host(self._h, C.byref(nd), C.byref(p), e.ctypes.data, len(e), C.byref(out), C.byref(m)))
        try:
            r = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int32)), shape=(max(m.value, 1) * 3,))[: m.value * 3]
            return r.reshape(-1, 3).copy()
        finally:
            self._lib.alga_free_edges(self._h, out)

    def pkb_supplement_device(self, words, lens, d_edges, n_edges, p, stream=None):
        """node set (torch device tensors) and edge list (device pointer, sorted by (src, dst)) in HBM -> (ptr, n_edges) engine-owned"""
        nd = self._nodes_from_torch(words, lens, None, None)
        out = C.c_void_p()
        m = C.c_uint64()
        self._check(self._lib.alga_pkb_supplement_device(self._h, C.byref(nd), C.byref(p), C.c_void_p(d_edges), C.c_uint64(int(n_edges)),
                                                         C.c_void_p(stream or 0), C.byref(out), C.byref(m)))
        return out.value, int(m.value)

    # ---- the supplement on N ranks: begin -> { round -> [all-gather of the additions] -> merge } x rounds -> end (include/alga_amd.h) ----
    def pkb_shard_begin(self, words, lens, d_edges, n_edges, p, rank, n_ranks, stream=None):
        nd = self._nodes_from_torch(words, lens)
        self._check(self._lib.alga_pkb_shard_begin(self._h, C.byref(nd), C.byref(p), C.c_void_p(d_edges), int(n_edges), int(rank), int(n_ranks), C.c_void_p(stream or 0)))

    def pkb_shard_round(self, stream=None):
        """-> (device pointer of this rank's additions (uint64 keys), how many)"""
        out, m = C.c_void_p(), C.c_uint64()
        self._check(self._lib.alga_pkb_shard_round(self._h, C.c_void_p(stream or 0), C.byref(out), C.byref(m)))
        return out.value, int(m.value)

    def pkb_shard_merge(self, d_all, n_all, stream=None):
        self._check(self._lib.alga_pkb_shard_merge(self._h, C.c_void_p(d_all), int(n_all), C.c_void_p(stream or 0)))

    def pkb_shard_end(self, stream=None):
        out, m = C.c_void_p(), C.c_uint64()
        self._check(self._lib.alga_pkb_shard_end(self._h, C.c_void_p(stream or 0), C.byref(out), C.byref(m)))
        return out.value, int(m.value)

    def pkb_last_stats(self):
        st = PkbStats()
        self._check(self._lib.alga_pkb_last_stats(self._h, C.byref(st)))
        return dict(kmers=list(st.kmers), groups=list(st.groups), can_align_calls=list(st.can_align_calls),
                    edges_after=list(st.edges_after), max_group=st.max_group, ms_total=st.ms_total,
                    group_hist=[list(r) for r in st.group_hist])

    # ---- first simplifier step ----------------------------------------------------------------
    def cut_triangles_host(self, n_nodes, edges, max_offset_parallel_paths):
        """edges [m, 3] sorted by (src, dst) -> the graph after sortEdgesByIncreasingOffset + cutNonAndWeaklyMetricTriangles,
        lists in the reference's order."""
        e = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 3)
        out, m = C.c_void_p(), C.c_uint64()
        self._check(self._lib.alga_cut_triangles_host(self._h, int(n_nodes), e.ctypes.data, len(e), int(max_offset_parallel_paths), C.byref(out), C.byref(m)))
        try:
            r = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int32)), shape=(max(m.value, 1) * 3,))[: m.value * 3]
            return r.reshape(-1, 3).copy()
        finally:
            self._lib.alga_free_edges(self._h, out)

    def cut_triangles_device(self, n_nodes, d_edges_ptr, n_edges, max_offset_parallel_paths, stream=None):
        """device edge list (pointer) -> (device pointer, n_edges_out, n_removed); engine-owned."""
        out, m, rem = C.c_void_p(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.alga_cut_triangles_device(self._h, int(n_nodes), C.c_void_p(d_edges_ptr), int(n_edges), int(max_offset_parallel_paths),
                                                        C.c_void_p(stream or 0), C.byref(out), C.byref(m), C.byref(rem)))
        return out.value, int(m.value), int(rem.value)

    def remove_short_parallel_paths(self, n_nodes, edges, max_offset, n_edges=None, stream=None):
        """Remove the short parallel paths (alga_remove_short_parallel_paths_device: the definition is in include/alga_amd.h) -> (edges, info).
        edges in: a device pointer (with n_edges), an int32 device tensor [m, 3] or a numpy array [m, 3] (uploaded), grouped by src in ascending
        order, every list in the order the triangle cut leaves it in.
        edges out: a zero-copy int32 device tensor [m', 3], grouped by src, the lists in the reference's order, engine-owned, valid until the next
        call of this method (clone what has to live longer); it goes straight into remove_dangling_branches and unitigs.  info: dict of
        alga_mst_info, "winners" = the begs run per round.
        stream: the stream that produced the input, synchronised first (the call runs on the engine's own stream)."""
        import torch
        dev = torch.device("cuda", self.device)
        keep = None
        if isinstance(edges, np.ndarray):
            e = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 3)
            keep = torch.from_numpy(e).to(dev)
            ptr, m = _ptr(keep), len(e)
        elif isinstance(edges, int):
            ptr, m = edges, int(n_edges or 0)
        else:
            keep = edges
            ptr, m = _ptr(edges), int(edges.shape[0]) if n_edges is None else int(n_edges)
        if stream is not None:
            torch.cuda.ExternalStream(stream).synchronize() if isinstance(stream, int) else stream.synchronize()
        else:
            torch.cuda.current_stream(dev).synchronize()
        out, mo, info = C.c_void_p(), C.c_uint64(), MstInfo()
        self._check(self._lib.alga_remove_short_parallel_paths_device(self._h, int(n_nodes), C.c_void_p((ptr or None) if m else None), C.c_uint64(m), int(max_offset),
                                                                      None, C.byref(out), C.byref(mo), C.byref(info)))
        del keep
        return device_view(out.value, (int(mo.value), 3), "cuda:%d" % self.device), info.as_dict()

    def remove_dangling_branches(self, n_nodes, edges, max_offset, n_edges=None, stream=None):
        """Clip the tips (alga_remove_dangling_branches_device: the definition is in include/alga_amd.h) -> (edges, info).
        edges in: a device pointer (with n_edges), an int32 device tensor [m, 3] or a numpy array [m, 3] (uploaded), in any order.
        edges out: a zero-copy int32 device tensor [m', 3] sorted by (src, dst, offset), engine-owned, valid until the next call of this method
        (clone what has to live longer); info: dict of alga_tips_info, "removed" = the counts per pass (down, up, down, up, ...).
        stream: the stream that produced the input, synchronised first (the call runs on the engine's own stream)."""
        import torch
        dev = torch.device("cuda", self.device)
        keep = None
        if isinstance(edges, np.ndarray):
            e = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 3)
            keep = torch.from_numpy(e).to(dev)
            ptr, m = _ptr(keep), len(e)
        elif isinstance(edges, int):
            ptr, m = edges, int(n_edges or 0)
        else:
            keep = edges
            ptr, m = _ptr(edges), int(edges.shape[0]) if n_edges is None else int(n_edges)
        if stream is not None:
            torch.cuda.ExternalStream(stream).synchronize() if isinstance(stream, int) else stream.synchronize()
        else:
            torch.cuda.current_stream(dev).synchronize()
        out, mo, info = C.c_void_p(), C.c_uint64(), TipsInfo()
        self._check(self._lib.alga_remove_dangling_branches_device(self._h, int(n_nodes), C.c_void_p((ptr or None) if m else None), C.c_uint64(m), int(max_offset), None,
                                                                   C.byref(out), C.byref(mo), C.byref(info)))
        del keep
        return device_view(out.value, (int(mo.value), 3), "cuda:%d" % self.device), info.as_dict()

    def contig_trim(self, words, lens, threshold=25):
        """src/main.cpp:636-697 on the GPU: packed contigs -> trim_left[n_contigs] (int32)."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        out = np.zeros(len(lens), dtype=np.int32)
        self._check(self._lib.alga_contig_trim_host(self._h, words.ctypes.data, int(words.shape[1]) if words.ndim == 2 else 1, lens.ctypes.data, len(lens),
                                                    int(threshold), out.ctypes.data))
        return out

    def write_gfa(self, path, words, lens, edges, n_edges=None, twins=True, sequences=True, stream=None):
        """The graph as GFA 1.0, formatted on the device (alga_write_gfa_device) -> dict of alga_gfa_info.
        words [n, stride] / lens [n]: the node set as torch device tensors (numpy arrays are uploaded first); edges: a device pointer
        (with n_edges), an int32 device tensor [m, 3] or a numpy array [m, 3] (uploaded), sorted by (src, dst, offset).
        twins: ALGA's layout (node 2k+1 = read k, 2k its reverse complement; one segment per pair); sequences: the ACGT field (else `*`).
        stream: the stream that produced the inputs, synchronised first (the call runs on the engine's own stream)."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(words, np.ndarray):
            words = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev)
        if isinstance(lens, np.ndarray):
            lens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
        keep = None
        if isinstance(edges, np.ndarray):
            e = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 3)
            keep = torch.from_numpy(e).to(dev)
            ptr, m = _ptr(keep), len(e)
        elif isinstance(edges, int):
            ptr, m = edges, int(n_edges or 0)
        else:
            keep = edges
            ptr, m = _ptr(edges), int(edges.shape[0]) if n_edges is None else int(n_edges)
        if stream is not None:
            torch.cuda.ExternalStream(stream).synchronize() if isinstance(stream, int) else stream.synchronize()
        else:
            torch.cuda.current_stream(dev).synchronize()
        nd = self._nodes_from_torch(words, lens)
        info = GfaInfo()
        flags = (GFA_TWINS if twins else 0) | (GFA_SEQUENCES if sequences else 0)
        self._check(self._lib.alga_write_gfa_device(self._h, C.byref(nd), C.c_void_p(ptr or None), C.c_uint64(m), os.fsencode(path), flags,
                                                    C.byref(info)))
        del keep
        return info.as_dict()

    def unitigs(self, words, lens, edges, n_edges=None, skip_isolated=False, stream=None):
        """The unitig graph (alga_unitigs_device: the definition is in include/alga_amd.h) -> Unitigs.
        words [n, stride] / lens [n]: the node set in the twin layout as torch device tensors (numpy arrays are uploaded first); edges: a
        device pointer (with n_edges), an int32 device tensor [m, 3] or a numpy array [m, 3] (uploaded), in any order.
        stream: the stream that produced the inputs, synchronised first (the call runs on the engine's own stream)."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(words, np.ndarray):
            words = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev)
        if isinstance(lens, np.ndarray):
            lens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
        keep = None
        if isinstance(edges, np.ndarray):
            e = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 3)
            keep = torch.from_numpy(e).to(dev)
            ptr, m = _ptr(keep), len(e)
        elif isinstance(edges, int):
            ptr, m = edges, int(n_edges or 0)
        else:
            keep = edges
            ptr, m = _ptr(edges), int(edges.shape[0]) if n_edges is None else int(n_edges)
        if stream is not None:
            torch.cuda.ExternalStream(stream).synchronize() if isinstance(stream, int) else stream.synchronize()
        else:
            torch.cuda.current_stream(dev).synchronize()
        n = int(lens.shape[0])
        nd = _Nodes(_ptr(words), int(words.shape[1]) if words.dim() == 2 else 1, _ptr(lens), n, None, None)
        out, info = UnitigsC(), UnitigInfo()
        self._check(self._lib.alga_unitigs_device(self._h, C.byref(nd), C.c_void_p(ptr or None), C.c_uint64(m), UNITIG_SKIP_ISOLATED if skip_isolated else 0,
                                                  None, C.byref(out), C.byref(info)))
        del keep
        return Unitigs(out, info.as_dict(), self.device)

    def contigs(self, words, lens, edges, max_offset, n_edges=None, stream=None):
        """The contigs (alga_contigs_device: contract, cut the contracted graph at max_offset, contract again; the definition is in
        include/alga_amd.h) -> Unitigs, with .info a dict of alga_contig_info.  The result becomes the engine's current unitig result:
        unitig_consensus, write_unitig_gfa and write_consensus_fasta take it (the FASTA then names its records contig_id=<j>).
        words [n, stride] / lens [n]: the node set in the twin layout as torch device tensors (numpy arrays are uploaded first); edges: a
        device pointer (with n_edges), an int32 device tensor [m, 3] or a numpy array [m, 3] (uploaded), in any order.
        stream: the stream that produced the inputs, synchronised first (the call runs on the engine's own stream)."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(words, np.ndarray):
            words = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev)
        if isinstance(lens, np.ndarray):
            lens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
        keep = None
        if isinstance(edges, np.ndarray):
            e = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 3)
            keep = torch.from_numpy(e).to(dev)
            ptr, m = _ptr(keep), len(e)
        elif isinstance(edges, int):
            ptr, m = edges, int(n_edges or 0)
        else:
            keep = edges
            ptr, m = _ptr(edges), int(edges.shape[0]) if n_edges is None else int(n_edges)
        if stream is not None:
            torch.cuda.ExternalStream(stream).synchronize() if isinstance(stream, int) else stream.synchronize()
        else:
            torch.cuda.current_stream(dev).synchronize()
        n = int(lens.shape[0])
        nd = _Nodes(_ptr(words), int(words.shape[1]) if words.dim() == 2 else 1, _ptr(lens), n, None, None)
        out, info = UnitigsC(), ContigInfo()
        self._check(self._lib.alga_contigs_device(self._h, C.byref(nd), C.c_void_p(ptr or None), C.c_uint64(m), int(max_offset), 0,
                                                  None, C.byref(out), C.byref(info)))
        del keep
        return Unitigs(out, info.as_dict(), self.device)

    def extend_contigs(self, words, lens, pair_off, contigs, min_chain_weight, min_connections=5, max_insert=1000, stream=None):
        """Contigs extended through junctions that paired reads support (alga_extend_contigs_device; the definition is in include/alga_amd.h)
        -> Unitigs, with .info a dict of alga_extend_info and .seams = (seam_off int64 [n_pairs + 1], seam_entry int32), zero-copy views.
        words / lens: the node set the LAST Engine.contigs call was made from, contigs: that call's result (no longer valid afterwards);
        pair_off uint8 [n]: Global::pairedReadOffset per node (0 unpaired, 1: the mate is v + 2, 2: v - 2), None: no pairs.  The result becomes
        the engine's current unitig result, as a contig result does.  The reference's min_chain_weight is int(2 * mean live read length)."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(words, np.ndarray):
            words = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev)
        if isinstance(lens, np.ndarray):
            lens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
        if isinstance(pair_off, np.ndarray):
            pair_off = torch.from_numpy(np.ascontiguousarray(pair_off, dtype=np.uint8)).to(dev)
        if pair_off is not None:
            assert pair_off.dtype == torch.uint8 and pair_off.is_contiguous() and int(pair_off.shape[0]) == int(lens.shape[0])
        if stream is not None:
            torch.cuda.ExternalStream(stream).synchronize() if isinstance(stream, int) else stream.synchronize()
        else:
            torch.cuda.current_stream(dev).synchronize()
        nd = _Nodes(_ptr(words), int(words.shape[1]) if words.dim() == 2 else 1, _ptr(lens), int(lens.shape[0]), None, None)
        out, info, seams = UnitigsC(), ExtendInfo(), ExtendSeamsC()
        self._check(self._lib.alga_extend_contigs_device(self._h, C.byref(nd), C.c_void_p(_ptr(pair_off) or None),
                                                         C.byref(contigs._c), int(min_chain_weight), int(min_connections), int(max_insert), 0, None,
                                                         C.byref(out), C.byref(info)))
        self._check(self._lib.alga_extend_seams_get(self._h, C.byref(out), C.byref(seams)))
        res = Unitigs(out, info.as_dict(), self.device)
        d = "cuda:%d" % self.device
        res.seams = (device_view(seams.d_seam_off, (res.n_pairs + 1,), d, "<i8"), device_view(seams.d_seam_entry, (int(seams.n_seams),), d))
        return res

    def write_unitig_gfa(self, path, unitigs, sequences=True, consensus=None):
        """The result of the LAST Engine.unitigs call as GFA 1.0 (alga_write_unitig_gfa_device) -> dict of alga_gfa_info: pair k is segment k,
        a unitig edge and its twin are one link.  consensus: the result of the LAST Engine.unitig_consensus call -- the segments then carry
        the untrimmed consensus instead of the spelled sequence (the link overlaps hold for it as they are)."""
        info = GfaInfo()
        flags = (GFA_SEQUENCES if sequences else 0) | (GFA_CONSENSUS if consensus is not None else 0)
        self._check(self._lib.alga_write_unitig_gfa_device(self._h, C.byref(unitigs._c), os.fsencode(path), flags, C.byref(info)))
        return info.as_dict()

    def unitig_consensus(self, words, lens, unitigs, min_votes=3, votes=False, stream=None):
        """Consensus sequences of the unitigs (alga_unitig_consensus_device: the definition is in include/alga_amd.h) -> Consensus.
        words / lens: the node set the LAST Engine.unitigs call was made from (torch device tensors; numpy arrays are uploaded first);
        unitigs: that call's result.  min_votes: the window ends at the first / last column whose winning base has more votes than this
        (the reference: 3; 0: no trimming).  votes: also return the winning count of every column (one byte, saturated at 255)."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(words, np.ndarray):
            words = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev)
        if isinstance(lens, np.ndarray):
            lens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
        if stream is not None:
            torch.cuda.ExternalStream(stream).synchronize() if isinstance(stream, int) else stream.synchronize()
        else:
            torch.cuda.current_stream(dev).synchronize()
        nd = _Nodes(_ptr(words), int(words.shape[1]) if words.dim() == 2 else 1, _ptr(lens), int(lens.shape[0]), None, None)
        out, info = ConsensusC(), ConsensusInfo()
        self._check(self._lib.alga_unitig_consensus_device(self._h, C.byref(nd), C.byref(unitigs._c), int(min_votes), CONSENSUS_VOTES if votes else 0,
                                                           None, C.byref(out), C.byref(info)))
        return Consensus(out, info.as_dict(), unitigs, self.device)

    def write_consensus_fasta(self, path, unitigs, consensus, min_length=200):
        """The windows of the LAST Engine.unitig_consensus call as FASTA (alga_write_consensus_fasta_device) -> dict of alga_gfa_info
        (segments = records): `>unitig_<k>_length=<len>` and the sequence on one line, for every pair with len >= min_length."""
        info = GfaInfo()
        self._check(self._lib.alga_write_consensus_fasta_device(self._h, C.byref(unitigs._c), C.byref(consensus._c), os.fsencode(path), int(min_length),
                                                                C.byref(info)))
        return info.as_dict()

    def contig_trim_device(self, words, begin, lens, threshold=25, stream=None):
        """The trim of contig ends against each other (src/main.cpp:636-697) on ragged sequences in device memory (alga_contig_trim_device)
        -> trim_left int32 [n], a torch device tensor.  words: the 2-bit packed array (int32 / uint32, any shape), begin int64 [n]: the base
        index of each sequence's first base in it (any index), lens int32 [n]; torch device tensors (numpy arrays are uploaded first).
        Sequences longer than 1002 nt enter the build as their first and last 501 nt: there is no length limit.  The call runs a build on
        the engine (its last build result is gone); the current unitig, consensus and final results stay."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(words, np.ndarray):
            words = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev)
        if isinstance(begin, np.ndarray):
            begin = torch.from_numpy(np.ascontiguousarray(begin).astype(np.int64)).to(dev)
        if isinstance(lens, np.ndarray):
            lens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
        assert begin.dtype == torch.int64 and lens.dtype == torch.int32 and begin.shape == lens.shape
        if stream is not None:
            torch.cuda.ExternalStream(stream).synchronize() if isinstance(stream, int) else stream.synchronize()
        else:
            torch.cuda.current_stream(dev).synchronize()
        n = int(lens.shape[0])
        out = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        m = C.c_uint64()
        self._check(self._lib.alga_contig_trim_device(self._h, _ptr(words), _ptr(begin), _ptr(lens), n, int(threshold), None, _ptr(out), C.byref(m)))
        self.last_trim_edges = int(m.value)
        return out

    def final_contigs(self, unitigs, consensus, min_length=200, new_reads_percent=95, trim_threshold=25):
        """The final contig set (alga_final_contigs_device: OutputWriterNew::filterContigs' length and new-read filter in longest-first order,
        the numbering, the trim of the ends against each other; the definition is in include/alga_amd.h) -> FinalContigs.
        unitigs / consensus: the results of the LAST Engine.contigs (or unitigs) and unitig_consensus calls.  trim_threshold 0: no trim."""
        out, info = FinalContigsC(), FinalInfo()
        self._check(self._lib.alga_final_contigs_device(self._h, C.byref(unitigs._c), C.byref(consensus._c), int(min_length), int(new_reads_percent),
                                                        int(trim_threshold), 0, None, C.byref(out), C.byref(info)))
        return FinalContigs(out, info.as_dict(), unitigs, consensus, self.device)

    def write_final_fasta(self, path, final, placements=None, polished=None, depth=True):
        """The accepted contigs of the LAST Engine.final_contigs call as FASTA (alga_write_final_fasta_device) -> dict of alga_gfa_info
        (segments = records): `>contig_id=<id>_length=<len>` and the window on one line, in id order.  placements: the result of the LAST
        Engine.place_reads(final=final) call -- the headers then end in `_reads=<n>_depth=<q>.<dd>` (alga_write_final_fasta_depth_device).
        polished: the result of the LAST Engine.polish of those placements -- the sequences are then the polished ones
        (alga_write_polished_fasta_device), the headers with the depth iff `depth`."""
        info = GfaInfo()
        if polished is not None:
            assert placements is not None, "polished needs the placements it was made from"
            self._check(self._lib.alga_write_polished_fasta_device(self._h, C.byref(final._unitigs._c), C.byref(final._consensus._c), C.byref(final._c),
                                                                   C.byref(placements._c), C.byref(polished._c), 1 if depth else 0, os.fsencode(path), C.byref(info)))
            return info.as_dict()
        if placements is not None:
            return self._write(self._lib.alga_write_final_fasta_depth_device, path, final._unitigs, final._consensus, final, placements)
        return self._write(self._lib.alga_write_final_fasta_device, path, final._unitigs, final._consensus, final)

    # ---- reads placed on sequences: depth, pairs, inserts (the definition: include/alga_amd.h) -----
    @staticmethod
    def place_params(k=21, max_mismatches=4, max_occ=256, max_insert=1000, depth_multi=False, flags=None):
        p = PlaceParams()
        p.k, p.max_mismatches, p.max_occ, p.max_insert = int(k), int(max_mismatches), int(max_occ), int(max_insert)
        p.flags = int(flags) if flags is not None else (PLACE_DEPTH_MULTI if depth_multi else 0)
        return p

    def _dev(self):
        import torch
        return torch.device("cuda", self.device)

    def _write(self, fn, path, *handles):
        """a text writer of the C ABI over result handles (None where one is optional) -> dict of alga_gfa_info"""
        info = GfaInfo()
        self._check(fn(self._h, *[C.byref(h._c) if h is not None else None for h in handles], os.fsencode(path), C.byref(info)))
        return info.as_dict()

    def place_reads(self, words, lens, targets=None, final=None, pair_off=None, stream=None, **params):
        """Every read of a node set in twin layout placed on target sequences (alga_place_reads_device) -> Placements.  words [n, stride] /
        lens [n]: node 2r + 1 is read r, node 2r its reverse complement; pair_off uint8 [n] or None.  targets = (packed words, begin int64 [T],
        len int32 [T]): ragged sequences, sequence t from base index begin[t] on; or final = the result of the LAST Engine.final_contigs
        call: target id == contig id (alga_place_reads_on_final_device).  Host arrays are uploaded first; tensors are used where they are and
        left untouched.  params: k, max_mismatches, max_occ, max_insert, depth_multi."""
        assert (targets is None) != (final is None), "give targets or final"
        dev = self._dev()
        nd, (words, lens, pair_off) = _twin_nodes(words, lens, dev, pair_off)
        pp, out, info = self.place_params(**params), PlacementsC(), PlaceInfo()
        if final is not None:
            self._check(self._lib.alga_place_reads_on_final_device(self._h, C.byref(nd), C.c_void_p(_ptr(pair_off) or None), C.byref(final._unitigs._c),
                                                                   C.byref(final._consensus._c), C.byref(final._c), C.byref(pp), _stream_arg(stream, dev),
                                                                   C.byref(out), C.byref(info)))
        else:
            twords, tbegin, tlen = _ragged_targets(targets, dev)
            self._check(self._lib.alga_place_reads_device(self._h, C.byref(nd), C.c_void_p(_ptr(pair_off) or None), C.c_void_p(_ptr(twords) or None),
                                                          C.c_void_p(_ptr(tbegin) or None), C.c_void_p(_ptr(tlen) or None), int(tlen.shape[0]), C.byref(pp),
                                                          _stream_arg(stream, dev), C.byref(out), C.byref(info)))
        return Placements(out, info.as_dict(), self.device, final)

    def polish(self, words, lens, placements, min_cover=3, min_percent=60, multi=False, counts=False, stream=None):
        """The placed targets voted again by every placed read (alga_polish_placed_device) -> Polished.  words / lens: the node set that was
        placed; placements: the result of the LAST Engine.place_reads call.  A column changes to the base with the most votes iff its cover is
        at least min_cover and that base has at least min_percent of it; multi: MULTI reads vote too; counts: keep the four counts per column."""
        dev = self._dev()
        nd, keep = _twin_nodes(words, lens, dev)
        pp, out, info = PolishParams(), PolishedC(), PolishInfo()
        pp.min_cover, pp.min_percent, pp.flags = int(min_cover), int(min_percent), (POLISH_MULTI if multi else 0) | (POLISH_COUNTS if counts else 0)
        self._check(self._lib.alga_polish_placed_device(self._h, C.byref(nd), C.byref(placements._c), C.byref(pp), _stream_arg(stream, dev), C.byref(out),
                                                        C.byref(info)))
        return Polished(out, info.as_dict(), self.device, placements)

    def scaffold(self, words, lens, pair_off, placements, insert=None, max_insert=1000, min_links=5, max_second_percent=50, min_gap=10, stream=None):
        """Scaffolds from the pairs the placement split over two targets (alga_scaffold_placed_device) -> Scaffolds.  words / lens / pair_off:
        the node set that was placed and its pairing (None: no pairs); placements: the result of the LAST Engine.place_reads call.  insert: the
        library's insert size, by default the placement's insert_median (refused where that is -1: no proper pair was seen).  Two ends are joined
        iff each is the other's only choice: at least min_links links within max_insert, and no second bundle with max_second_percent of them."""
        dev = self._dev()
        if insert is None:
            insert = int(placements.info["insert_median"])
            if insert < 0:
                raise AlgaError(-1, "Engine.scaffold: the placement saw no proper pair (insert_median -1): give insert")
        nd, (words, lens, pair_off) = _twin_nodes(words, lens, dev, pair_off)
        pp, out, info = ScaffoldParams(), ScaffoldsC(), ScaffoldInfo()
        pp.insert, pp.max_insert, pp.min_links, pp.max_second_percent, pp.min_gap = int(insert), int(max_insert), int(min_links), int(max_second_percent), int(min_gap)
        self._check(self._lib.alga_scaffold_placed_device(self._h, C.byref(nd), C.c_void_p(_ptr(pair_off) or None), C.byref(placements._c), C.byref(pp),
                                                          _stream_arg(stream, dev), C.byref(out), C.byref(info)))
        return Scaffolds(out, info.as_dict(), self.device, placements)

    def write_scaffold_fasta(self, path, placements, scaffolds, polished=None):
        """The scaffolds of the LAST Engine.scaffold call as FASTA (alga_write_scaffold_fasta_device) -> dict of alga_gfa_info (segments =
        records): `>scaffold_id=<j>_length=<len>_contigs=<m>` and the contigs with their gaps as runs of N on one line, in id order.  polished:
        the result of the LAST Engine.polish of those placements -- the bases are then the polished ones."""
        return self._write(self._lib.alga_write_scaffold_fasta_device, path, placements, scaffolds, polished)

    def break_contigs(self, words, lens, pair_off, placements, polished=None, margin=None, min_span=1, inset=21, stream=None):
        """The placed targets cut where no proper pair spans them (alga_break_placed_device) -> Broken.  words / lens / pair_off: the node set
        that was placed and its pairing (None: no pairs, nothing is cut); placements: the result of the LAST Engine.place_reads call; polished:
        the result of the LAST Engine.polish of those placements -- the pieces then carry the polished bases.  A pair spans the columns from
        inset behind its first to inset before its last; a stretch of columns spanned by fewer than min_span pairs, at least margin columns
        from both ends of its target and with spanned columns on both sides, is cut in its middle.  margin: by default the placement's
        insert_median (refused where that is -1: no proper pair was seen)."""
        dev = self._dev()
        if margin is None:
            margin = int(placements.info["insert_median"])
            if margin < 0:
                raise AlgaError(-1, "Engine.break_contigs: the placement saw no proper pair (insert_median -1): give margin")
        nd, (words, lens, pair_off) = _twin_nodes(words, lens, dev, pair_off)
        pp, out, info = BreakParams(), BrokenC(), BreakInfo()
        pp.min_span, pp.inset, pp.margin = int(min_span), int(inset), int(margin)
        self._check(self._lib.alga_break_placed_device(self._h, C.byref(nd), C.c_void_p(_ptr(pair_off) or None), C.byref(placements._c),
                                                       C.byref(polished._c) if polished is not None else None, C.byref(pp), _stream_arg(stream, dev),
                                                       C.byref(out), C.byref(info)))
        return Broken(out, info.as_dict(), self.device, placements)

    def write_broken_fasta(self, path, broken):
        """The pieces of the LAST Engine.break_contigs call as FASTA (alga_write_broken_fasta_device) -> dict of alga_gfa_info (segments =
        records): `>contig_id=<j>_length=<len>_from=<t>_start=<s>` per piece with a length, j the piece id."""
        return self._write(self._lib.alga_write_broken_fasta_device, path, broken)

    def grow_ends(self, words, lens, placements, polished=None, stream=None, **params):
        """The ends of the placed targets grown with the unplaced reads that hang over them (alga_grow_placed_device) -> Grown.  words / lens:
        the node set that was placed; placements: the result of the LAST Engine.place_reads call; polished: the result of the LAST
        Engine.polish of those placements -- the grown targets then carry the polished bases.  params: k, max_mismatches, max_occ, min_anchor,
        min_cover, min_percent, max_grow (the fields of alga_grow_params; the library's defaults where not given).  A further round is a
        placement on Grown.targets() and a further call."""
        dev = self._dev()
        nd, keep = _twin_nodes(words, lens, dev)
        pp, out, info = GrowParams(), GrownC(), GrowInfo()
        self._lib.alga_grow_default_params(C.byref(pp))
        _set_params(pp, params, ("k", "max_mismatches", "max_occ", "min_anchor", "min_cover", "min_percent", "max_grow", "flags"), "Engine.grow_ends")
        self._check(self._lib.alga_grow_placed_device(self._h, C.byref(nd), C.byref(placements._c), C.byref(polished._c) if polished is not None else None,
                                                      C.byref(pp), _stream_arg(stream, dev), C.byref(out), C.byref(info)))
        return Grown(out, info.as_dict(), self.device, placements)

    def write_grown_fasta(self, path, grown):
        """The grown targets of the LAST Engine.grow_ends call as FASTA (alga_write_grown_fasta_device) -> dict of alga_gfa_info (segments =
        records): `>contig_id=<t>_length=<len>_left=<xl>_right=<xr>` per target with a length."""
        return self._write(self._lib.alga_write_grown_fasta_device, path, grown)

    def merge_ends(self, targets, stream=None, **params):
        """Contigs whose ends overlap merged into one sequence (alga_merge_targets_device) -> Merged.  targets = (packed words, begin int64 [T],
        len int32 [T]): ragged sequences as Engine.place_reads takes them, for instance Grown.targets() or the Merged.targets() of the call
        before.  Host arrays are uploaded first; tensors are used where they are and left untouched.  params: k, max_mismatches, max_occ,
        min_overlap, max_overlap (the fields of alga_merge_params; the library's defaults where not given)."""
        dev = self._dev()
        twords, tbegin, tlen = _ragged_targets(targets, dev)
        assert twords.is_contiguous()
        pp, out, info = MergeParams(), MergedC(), MergeInfo()
        self._lib.alga_merge_default_params(C.byref(pp))
        _set_params(pp, params, ("k", "max_mismatches", "max_occ", "min_overlap", "max_overlap", "flags"), "Engine.merge_ends")
        self._check(self._lib.alga_merge_targets_device(self._h, C.c_void_p(_ptr(twords) or None), C.c_void_p(_ptr(tbegin) or None), C.c_void_p(_ptr(tlen) or None),
                                                        int(tlen.shape[0]), C.byref(pp), _stream_arg(stream, dev), C.byref(out), C.byref(info)))
        return Merged(out, info.as_dict(), self.device, (twords, tbegin, tlen))     # the tensors the targets came from stay alive with the result

    def write_merged_fasta(self, path, merged):
        """The merged contigs of the LAST Engine.merge_ends call as FASTA (alga_write_merged_fasta_device) -> dict of alga_gfa_info (segments =
        records): `>contig_id=<j>_length=<len>_contigs=<m>` per merged contig."""
        return self._write(self._lib.alga_write_merged_fasta_device, path, merged)

    def drop_contained(self, targets, stream=None, **params):
        """Contigs contained in another contig dropped (alga_drop_contained_device) -> Kept.  targets = (packed words, begin int64 [T], len int32
        [T]): ragged sequences as Engine.place_reads takes them, for instance Merged.targets() or the Kept.targets() of the call before.  Host
        arrays are uploaded first; tensors are used where they are and left untouched.  params: k, max_permille, max_occ (the fields of
        alga_contain_params; the library's defaults where not given)."""
        dev = self._dev()
        twords, tbegin, tlen = _ragged_targets(targets, dev)
        assert twords.is_contiguous()
        pp, out, info = ContainParams(), KeptC(), ContainInfo()
        self._lib.alga_contain_default_params(C.byref(pp))
        _set_params(pp, params, ("k", "max_permille", "max_occ", "flags", "reserved"), "Engine.drop_contained")
        self._check(self._lib.alga_drop_contained_device(self._h, C.c_void_p(_ptr(twords) or None), C.c_void_p(_ptr(tbegin) or None), C.c_void_p(_ptr(tlen) or None),
                                                         int(tlen.shape[0]), C.byref(pp), _stream_arg(stream, dev), C.byref(out), C.byref(info)))
        return Kept(out, info.as_dict(), self.device, (twords, tbegin, tlen))       # the tensors the targets came from stay alive with the result

    def write_kept_fasta(self, path, kept):
        """The kept contigs of the LAST Engine.drop_contained call as FASTA (alga_write_kept_fasta_device) -> dict of alga_gfa_info (segments =
        records): `>contig_id=<j>_length=<len>_absorbed=<m>` per kept contig."""
        return self._write(self._lib.alga_write_kept_fasta_device, path, kept)

    _STITCH_PARAMS = ("max_mismatches", "min_overlap", "max_overlap", "slack", "flags")

    def stitch(self, placements, scaffolds, polished=None, stream=None, **params):
        """The joins of the scaffolds whose two contig ends overlap stitched into one sequence (alga_stitch_scaffolds_device) -> Stitched.
        placements: the result of the LAST Engine.place_reads call; scaffolds: the result of the LAST Engine.scaffold call on it (its bundles
        are the entries); polished: the result of the LAST Engine.polish of those placements -- the stitched contigs then carry the polished
        bases.  params: max_mismatches, min_overlap, max_overlap, slack (the fields of alga_stitch_params; the library's defaults where not
        given).  A further round is a placement on Stitched.targets(), a scaffold call and a further call."""
        import torch
        dev = self._dev()
        pp, out, info = StitchParams(), StitchedC(), StitchInfo()
        self._lib.alga_stitch_default_params(C.byref(pp))
        _set_params(pp, params, self._STITCH_PARAMS, "Engine.stitch")
        self._check(self._lib.alga_stitch_scaffolds_device(self._h, C.byref(placements._c), C.byref(scaffolds._c), C.byref(polished._c) if polished is not None else None,
                                                           C.byref(pp), _stream_arg(stream, dev), C.byref(out), C.byref(info)))
        off = placements.col_off.to(torch.int64) & 0xFFFFFFFF                    # (the bits of uint32)
        return Stitched(out, info.as_dict(), self.device, (placements, scaffolds, (off[1:] - off[:-1]).to(torch.int32)))

    def stitch_targets(self, targets, entries, stream=None, **params):
        """The entries whose two contig ends overlap stitched into one sequence (alga_stitch_targets_device) -> Stitched.  targets = (packed
        words, begin int64 [T], len int32 [T]): ragged sequences as Engine.place_reads takes them, for instance Merged.targets() or the
        Stitched.targets() of the call before.  entries = (a, b, gap[, state]): ends a / b (uint32 as host arrays, int32 with the same bits as
        tensors; x = 2t left, 2t + 1 right), gap int32, state uint8 as Scaffolds.b_state (None or left out: every entry is selected).  Host
        arrays are uploaded first; tensors are used where they are and left untouched.  params: as Engine.stitch."""
        import torch
        dev = self._dev()
        twords, tbegin, tlen = _ragged_targets(targets, dev)
        assert twords.is_contiguous()
        ja, jb, jgap = _upload(entries[0], np.uint32, dev, np.int32), _upload(entries[1], np.uint32, dev, np.int32), _upload(entries[2], np.int32, dev)
        jstate = _upload(entries[3], np.uint8, dev) if len(entries) > 3 else None
        J = int(ja.shape[0])
        for x in (ja, jb, jgap):
            assert x.dtype == torch.int32 and x.shape == (J,) and x.is_contiguous()
        assert jstate is None or (jstate.dtype == torch.uint8 and jstate.shape == (J,) and jstate.is_contiguous())
        pp, out, info = StitchParams(), StitchedC(), StitchInfo()
        self._lib.alga_stitch_default_params(C.byref(pp))
        _set_params(pp, params, self._STITCH_PARAMS, "Engine.stitch_targets")
        self._check(self._lib.alga_stitch_targets_device(self._h, C.c_void_p(_ptr(twords) or None), C.c_void_p(_ptr(tbegin) or None), C.c_void_p(_ptr(tlen) or None),
                                                         int(tlen.shape[0]), C.c_void_p(_ptr(ja) or None), C.c_void_p(_ptr(jb) or None), C.c_void_p(_ptr(jgap) or None),
                                                         C.c_void_p(_ptr(jstate) or None) if jstate is not None else None, J, C.byref(pp), _stream_arg(stream, dev),
                                                         C.byref(out), C.byref(info)))
        return Stitched(out, info.as_dict(), self.device, (twords, tbegin, tlen, ja, jb, jgap, jstate))   # what the call read stays alive with the result

    def write_stitched_fasta(self, path, stitched):
        """The stitched contigs of the LAST stitch call as FASTA (alga_write_stitched_fasta_device) -> dict of alga_gfa_info (segments =
        records): `>contig_id=<j>_length=<len>_contigs=<m>` per stitched contig."""
        return self._write(self._lib.alga_write_stitched_fasta_device, path, stitched)

    def place_gapped(self, words, lens, placements, targets=None, final=None, stream=None, **params):
        """The reads the Hamming placement left unplaced laid onto the same targets by edit distance (alga_place_gapped_device) -> Gapped.
        words / lens: the node set that was placed; placements: the result of the LAST Engine.place_reads call; targets = the (packed words,
        begin int64 [T], len int32 [T]) that call was given, or final = the Engine.final_contigs result it was given.  Host arrays are
        uploaded first; tensors are used where they are and left untouched.  params: k, max_edits, max_occ (the fields of alga_gapped_params;
        the library's defaults where not given)."""
        import torch
        assert (targets is None) != (final is None), "give targets or final"
        dev = self._dev()
        nd, keep = _twin_nodes(words, lens, dev)
        if final is not None:
            # the targets of alga_place_reads_on_final_device: target j = the window of the pair order[j] in the consensus words
            u, fin = final._unitigs, final
            order = fin.order.to(torch.int64)
            live = fin.verdict.to(torch.int64)[order] == 2
            zero = torch.zeros_like(order)
            tbegin = (16 * u.word_off.to(torch.int64)[order] + torch.where(live, fin.begin.to(torch.int64)[order], zero)).contiguous()
            tlen = torch.where(live, fin.len.to(torch.int64)[order], zero).to(torch.int32).contiguous()
            targets = (final._consensus.words, tbegin, tlen)
        twords, tbegin, tlen = _ragged_targets(targets, dev)
        pp, out, info = GappedParams(), GappedC(), GappedInfo()
        self._lib.alga_gapped_default_params(C.byref(pp))
        _set_params(pp, params, ("k", "max_edits", "max_occ", "flags"), "Engine.place_gapped")
        self._check(self._lib.alga_place_gapped_device(self._h, C.byref(nd), C.c_void_p(_ptr(twords) or None), C.c_void_p(_ptr(tbegin) or None),
                                                       C.c_void_p(_ptr(tlen) or None), int(tlen.shape[0]), C.byref(placements._c), C.byref(pp),
                                                       _stream_arg(stream, dev), C.byref(out), C.byref(info)))
        return Gapped(out, info.as_dict(), self.device, (placements, twords, tbegin, tlen))

    def write_gapped_tsv(self, path, gapped):
        """The gapped placements of the LAST Engine.place_gapped call as text (alga_write_gapped_tsv_device) -> dict of alga_gfa_info (segments =
        lines): `read target pos end strand edits unique cigar` (tabs) per gapped-placed read, in read order."""
        return self._write(self._lib.alga_write_gapped_tsv_device, path, gapped)

    def polish_indels(self, words, lens, placements, gapped, min_cover=3, min_percent=60, max_ins=6, counts=False, stream=None):
        """The placed targets voted by the Hamming-placed and the gapped reads together (alga_polish_indels_device) -> IndelPolished: columns
        substituted or deleted, strings of at most max_ins bases inserted between two columns, the new targets.  words / lens: the node set
        that was placed; placements: the result of the LAST Engine.place_reads call; gapped: the result of the LAST Engine.place_gapped call,
        made from those placements.  counts: keep the five counts per column and the span per slot.  A further round is a placement on
        IndelPolished.targets."""
        dev = self._dev()
        nd, keep = _twin_nodes(words, lens, dev)
        pp, out, info = IpolishParams(), IpolishedC(), IpolishInfo()
        pp.min_cover, pp.min_percent, pp.max_ins, pp.flags = int(min_cover), int(min_percent), int(max_ins), IPOLISH_COUNTS if counts else 0
        self._check(self._lib.alga_polish_indels_device(self._h, C.byref(nd), C.byref(placements._c), C.byref(gapped._c), C.byref(pp), _stream_arg(stream, dev),
                                                        C.byref(out), C.byref(info)))
        return IndelPolished(out, info.as_dict(), self.device, (placements, gapped))

    def write_ipolished_fasta(self, path, ipolished):
        """The new targets of the LAST Engine.polish_indels call as FASTA (alga_write_ipolished_fasta_device) -> dict of alga_gfa_info (segments =
        records): `>contig_id=<t>_length=<len>_subs=<s>_ins=<i>_dels=<d>` per target with a length."""
        return self._write(self._lib.alga_write_ipolished_fasta_device, path, ipolished)

    def write_ipolish_events_tsv(self, path, ipolished):
        """The events of the LAST Engine.polish_indels call as text (alga_write_ipolish_events_tsv_device) -> dict of alga_gfa_info (segments =
        lines): `contig pos kind len old new votes cover` (tabs) per event, pos the old position inside the contig."""
        return self._write(self._lib.alga_write_ipolish_events_tsv_device, path, ipolished)

    def judge_pairs(self, words, lens, placements, gapped=None, pair_off=None, max_insert=None, stream=None, **params):
        """Every pair judged over the Hamming and the gapped placement together, the SAM FLAG and TLEN of every read
        (alga_judge_pairs_device) -> PairCalls.  words / lens / pair_off: the node set that was placed and its pairing (None: no pairs);
        placements: the result of the LAST Engine.place_reads call; gapped: the result of the LAST Engine.place_gapped call made from it, or
        None: the Hamming pass alone.  max_insert: the library's default (1000) where not given.  params: flags, reserved (tests)."""
        dev = self._dev()
        nd, (words, lens, pair_off) = _twin_nodes(words, lens, dev, pair_off)
        pp, out, info = PairParams(), PairCallsC(), PairInfo()
        self._lib.alga_pair_default_params(C.byref(pp))
        if max_insert is not None:
            pp.max_insert = int(max_insert)
        _set_params(pp, params, ("flags", "reserved"), "Engine.judge_pairs")
        self._check(self._lib.alga_judge_pairs_device(self._h, C.byref(nd), C.c_void_p(_ptr(pair_off) or None), C.byref(placements._c),
                                                      C.byref(gapped._c) if gapped is not None else None, C.byref(pp), _stream_arg(stream, dev), C.byref(out),
                                                      C.byref(info)))
        return PairCalls(out, info.as_dict(), self.device, (placements, gapped))

    def write_sam(self, path, words, lens, placements, calls, gapped=None, names_depth=False, skip_unplaced=False, **params):
        """Every live read as a SAM record, formatted on the device (alga_write_sam_device) -> dict of alga_gfa_info (segments = records).
        words / lens: the node set that was placed; placements / gapped: as Engine.judge_pairs was given them; calls: the result of the LAST
        Engine.judge_pairs call.  names_depth: the @SQ names as the depth FASTA's header token (contig_id=.._length=.._reads=.._depth=..),
        else as the plain final FASTA's; skip_unplaced: no records for unplaced reads.  QNAME is r<index>: the engine keeps no read names."""
        dev = self._dev()
        nd, keep = _twin_nodes(words, lens, dev)
        pp, info = SamParams(), GfaInfo()
        pp.flags = (SAM_NAMES_DEPTH if names_depth else 0) | (SAM_SKIP_UNPLACED if skip_unplaced else 0)
        _set_params(pp, params, ("flags", "reserved"), "Engine.write_sam")
        _stream_arg(None, dev)
        self._check(self._lib.alga_write_sam_device(self._h, C.byref(nd), C.byref(placements._c), C.byref(gapped._c) if gapped is not None else None,
                                                    C.byref(calls._c), C.byref(pp), os.fsencode(path), C.byref(info)))
        return info.as_dict()

    def write_graph(self, path, n_nodes, edges):
        edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 3)
        rc = self._lib.alga_write_graph(path.encode(), int(n_nodes), edges.ctypes.data, len(edges))
        if rc:
            raise AlgaError(rc, "alga_write_graph(%s) failed" % path)


class MultiEngine:
    """alga_multi_*: the N GPUs of one node behind one handle -- one process, one host thread and one engine per rank
    (alga_amd/csrc/engine_multi.hip).  devices may name the same GPU several times with transport="copy" (how a one-GPU box tests it)."""

    def __init__(self, devices, transport="auto"):
        self._lib = load_library()
        self._lib.alga_multi_create.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        self._lib.alga_multi_destroy.argtypes = [C.c_void_p]
        self._lib.alga_multi_destroy.restype = None
        self._lib.alga_multi_last_error.argtypes = [C.c_void_p]
        self._lib.alga_multi_last_error.restype = C.c_char_p
        self._lib.alga_multi_prefsuf_build_host.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PrefSufParams), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        self._lib.alga_multi_prefsuf_build_device.argtypes = [C.c_void_p, C.POINTER(_Nodes), C.POINTER(PrefSufParams), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        self._lib.alga_multi_free_edges.argtypes = [C.c_void_p, C.c_void_p]
        self._lib.alga_multi_free_edges.restype = None
        self._lib.alga_multi_last_stats.argtypes = [C.c_void_p, C.POINTER(MultiStats), C.c_void_p]
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self._lib.alga_multi_create(devs, len(devices), TRANSPORT[transport] if isinstance(transport, str) else int(transport), C.byref(h))
        if rc:
            raise AlgaError(rc, "alga_multi_create(devices=%s, transport=%s) failed" % (list(devices), transport))
        self._h, self.n = h, len(devices)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.alga_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise AlgaError(rc, (self._lib.alga_multi_last_error(self._h) or b"").decode())

    def set_option(self, name, value):
        """alga_multi_set_option: "form" ("auto" | "replicated" | "bucket_sharded")."""
        if name == "form" and isinstance(value, str):
            value = MULTI_FORM[value]
        self._lib.alga_multi_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        self._check(self._lib.alga_multi_set_option(self._h, name.encode(), int(value)))

    def rank_shard_stats(self, rank):
        """alga_shard_last_stats of one rank's engine (the bucket-sharded form's counters and device times)."""
        self._lib.alga_multi_engine.argtypes = [C.c_void_p, C.c_int32]
        self._lib.alga_multi_engine.restype = C.c_void_p
        self._lib.alga_shard_last_stats.argtypes = [C.c_void_p, C.POINTER(ShardStats)]
        st = ShardStats()
        self._lib.alga_shard_last_stats(C.c_void_p(self._lib.alga_multi_engine(self._h, int(rank))), C.byref(st))
        return st.as_dict()

    def set_rank_option(self, rank, name, value):
        """alga_engine_set_option on ONE rank's engine (alga_multi_engine): tests make a single rank decline this way."""
        self._lib.alga_multi_engine.argtypes = [C.c_void_p, C.c_int32]
        self._lib.alga_multi_engine.restype = C.c_void_p
        self._lib.alga_engine_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        eh = self._lib.alga_multi_engine(self._h, int(rank))
        if not eh:
            raise AlgaError(-1, "no such rank")
        rc = self._lib.alga_engine_set_option(C.c_void_p(eh), name.encode(), int(value))
        if rc:
            raise AlgaError(rc, "alga_engine_set_option(%s) on rank %d" % (name, rank))

    def prefsuf_host(self, words, lens, min_overlap, rsoe_min_overlap, align_from=None, align_to=None, collect_stats=False, reduction="auto", twin_rows=False):
        """twin_rows: `words` holds the rows of the odd nodes alone (alga_prefsuf_params.twin_rows)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = int(lens.shape[0])
        stride = int(words.shape[1]) if words.ndim == 2 else (words.size // max(n // 2 if twin_rows else n, 1))
        keep = [words, lens]
        nd = _Nodes(words.ctypes.data, stride, lens.ctypes.data, n, None, None)
        if align_from is not None:
            af = np.ascontiguousarray(align_from, dtype=np.uint8); keep.append(af); nd.align_from = af.ctypes.data
        if align_to is not None:
            at = np.ascontiguousarray(align_to, dtype=np.uint8); keep.append(at); nd.align_to = at.ctypes.data
        p = Engine.params(min_overlap, rsoe_min_overlap, collect_stats, reduction)
        p.twin_rows = 1 if twin_rows else 0
        out, m = C.c_void_p(), C.c_uint64()
        self._check(self._lib.alga_multi_prefsuf_build_host(self._h, C.byref(nd), C.byref(p), C.byref(out), C.byref(m)))
        try:
            e = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int32)), shape=(max(m.value, 1) * 3,))[: m.value * 3]
            return e.reshape(-1, 3).copy()
        finally:
            self._lib.alga_multi_free_edges(self._h, out)

    def prefsuf_device(self, per_rank, min_overlap, rsoe_min_overlap):
        """per_rank: [(words, lens)] torch tensors on each rank's device (the same node set) -> (device pointer on rank 0's GPU, n_edges)."""
        arr = (_Nodes * self.n)(*[Engine._nodes_from_torch(w, l) for w, l in per_rank])
        p = Engine.params(min_overlap, rsoe_min_overlap)
        out, m = C.c_void_p(), C.c_uint64()
        self._check(self._lib.alga_multi_prefsuf_build_device(self._h, arr, C.byref(p), C.byref(out), C.byref(m)))
        return out.value, int(m.value)

    def pkb_supplement_device(self, per_rank, d_edges_rank0, n_edges, p):
        """alga_multi_pkb_supplement_device: the approximate supplement on the handle's ranks; the exact graph on rank 0's GPU (what prefsuf_device
        returned) -> (device pointer on rank 0's GPU, n_edges)."""
        self._lib.alga_multi_pkb_supplement_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PkbParams), C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        arr = (_Nodes * self.n)(*[Engine._nodes_from_torch(w, l) for w, l in per_rank])
        out, m = C.c_void_p(), C.c_uint64()
        self._check(self._lib.alga_multi_pkb_supplement_device(self._h, arr, C.byref(p), C.c_void_p(d_edges_rank0), int(n_edges), C.byref(out), C.byref(m)))
        return out.value, int(m.value)

    def last_stats(self):
        st = MultiStats()
        per = (PrefSufStats * self.n)()
        self._check(self._lib.alga_multi_last_stats(self._h, C.byref(st), C.cast(per, C.c_void_p)))
        d = {k: getattr(st, k) for k, _ in st._fields_}
        d["ranks"] = [x.as_dict() for x in per]
        return d


def _upload(x, dt, dev, view=None):
    """a host array as a tensor on `dev` (converted to dt, its bits seen as `view` where given); None and tensors are passed through"""
    if x is None or not isinstance(x, np.ndarray):
        return x
    import torch
    a = np.ascontiguousarray(x, dtype=dt)
    return torch.from_numpy(a.view(view) if view is not None else a).to(dev)


def _twin_nodes(words, lens, dev, pair_off=None):
    """a node set in twin layout as the C ABI takes it: host arrays uploaded, tensors used where they are -> (_Nodes, (words, lens, pair_off): the
    tensors behind its pointers, for the caller to keep alive)"""
    import torch
    words, lens, pair_off = _upload(words, np.uint32, dev, np.int32), _upload(lens, np.int32, dev), _upload(pair_off, np.uint8, dev)
    n = int(lens.shape[0])
    assert lens.dtype == torch.int32 and lens.is_contiguous() and words.is_contiguous()
    if pair_off is not None:
        assert pair_off.dtype == torch.uint8 and pair_off.is_contiguous() and int(pair_off.shape[0]) == n
    return _Nodes(_ptr(words), int(words.shape[1]) if words.dim() == 2 and n else 1, _ptr(lens), n, None, None), (words, lens, pair_off)


def _ragged_targets(targets, dev):
    """(packed words, begin int64 [T], len int32 [T]) as tensors on `dev`: host arrays uploaded, tensors used where they are"""
    import torch
    twords, tbegin, tlen = targets
    twords, tlen = _upload(twords, np.uint32, dev, np.int32), _upload(tlen, np.int32, dev)
    if isinstance(tbegin, np.ndarray):
        tbegin = torch.from_numpy(np.ascontiguousarray(tbegin).astype(np.int64)).to(dev)
    assert tbegin.dtype == torch.int64 and tlen.dtype == torch.int32 and tbegin.shape == tlen.shape and tbegin.is_contiguous() and tlen.is_contiguous()
    return twords, tbegin, tlen


def _stream_arg(stream, dev):
    """what a stage call needs of the streams: the caller's stream (a torch stream or a raw handle) and torch's current one have finished what
    they were given (the uploads among it) -> the raw handle as the C ABI takes it (None: the engine's own stream)"""
    import torch
    if stream is not None:
        torch.cuda.ExternalStream(stream).synchronize() if isinstance(stream, int) else stream.synchronize()
    torch.cuda.current_stream(dev).synchronize()
    return C.c_void_p(stream) if isinstance(stream, int) and stream else None


def _set_params(pp, params, names, who):
    """the fields `names` of a params struct from **params (`reserved`: its first entry); another name is a TypeError"""
    for k, v in params.items():
        if k not in names:
            raise TypeError("%s: unknown parameter %r" % (who, k))
        if k == "reserved":
            pp.reserved[0] = int(v)
        else:
            setattr(pp, k, int(v))
    return pp


def _ptr(x):
    """device pointer of a torch tensor (or an int that already is one; None / empty -> 0)"""
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    return x.data_ptr() if x.numel() else 0


class _DevArray:
    """Zero-copy view of engine-owned device memory for torch (via __cuda_array_interface__)."""

    def __init__(self, ptr, shape, typestr="<i4"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def device_view(ptr, shape, device=None, typestr="<i4"):
    """torch tensor (int32, int64 with typestr "<i8", uint8 with "|u1") aliasing `ptr` (no copy).  Valid until the engine reuses
    the buffer."""
    import torch
    if int(np.prod(shape)) == 0:
        return torch.empty(tuple(shape), dtype={"<i4": torch.int32, "<i8": torch.int64, "|u1": torch.uint8, "<i2": torch.int16}[typestr], device=device or "cuda")
    return torch.as_tensor(_DevArray(ptr, shape, typestr), device=device or "cuda")


def host_edges_digest(e):
    """alga_amd.multigpu.edges_digest for a HOST edge list (numpy int32 [m, 3]): the same wrap-around int64 arithmetic -> [count, checksum]"""
    k = int(e.shape[0])
    acc = np.uint64(0)
    with np.errstate(over="ignore"):
        for s0 in range(0, k, 1 << 24):
            c = e[s0:s0 + (1 << 24)].astype(np.int64)
            w = np.arange(s0 + 1, s0 + c.shape[0] + 1, dtype=np.int64) | 1
            v = ((c[:, 0] * 1000003 + c[:, 1]) * 10007 + c[:, 2]) * w
            acc = acc + v.view(np.uint64).sum(dtype=np.uint64)
    return [k, int(np.array([acc], dtype=np.uint64).view(np.int64)[0])]


def device_edges_to_numpy(ptr, n_edges):
    """Copy an engine-owned device edge list to host (torch is only the memcpy)."""
    if n_edges == 0:
        return np.zeros((0, 3), np.int32)
    return device_view(ptr, (n_edges, 3)).cpu().numpy().copy()
