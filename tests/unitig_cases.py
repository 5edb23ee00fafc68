"""Hand-written unitig cases with their answers written out (tests/test_unitig_cpu.py checks the Python definition against them,
tests/test_gpu_unitig.py the device), and the loaders of the reference's graph dumps under tests/golden.

Every case: reads as strings (read k = node 2k+1, its reverse complement = node 2k), edges in any order, and the expected
path_node / path_pos / path_off / len / unitig edges, with and without ALGA_UNITIG_SKIP_ISOLATED where that differs."""
import gzip
import json
import os

import numpy as np

import alga_amd
import oracle_lib as O

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def nodes_of(reads):
    """reads (strings) -> (words, lens) of the twin layout"""
    L = max(len(r) for r in reads)
    codes = np.zeros((2 * len(reads), L), dtype=np.uint8)
    lens = np.zeros(2 * len(reads), dtype=np.int32)
    for k, r in enumerate(reads):
        c = np.array([_CODE[x] for x in r], dtype=np.uint8)
        codes[2 * k + 1, : len(c)] = c
        codes[2 * k, : len(c)] = 3 - c[::-1]
        lens[2 * k] = lens[2 * k + 1] = len(c)
    return alga_amd.pack_reads(codes, lens), lens


def _rc(s):
    return "".join("ACGT"[3 - _CODE[x]] for x in reversed(s))


A8, C8, G8 = "AAAAAAAA", "CCCCCCCC", "GGGGGGGG"
R = ["ACGTTGCA", "GTTGCAAG", "TGCAAGGC", "CAAGGCTA"]          # windows of one genome, two bases apart

# name -> dict(reads, edges, then per skip_isolated in (False, True) the expected arrays; "same": both flags give the same)
CASES = {
    # 1 -> 3 -> 5 given without its twin edges: E* adds 4 -> 2 -> 0; the path whose head is 1 (< 4) is `+`
    "chain_twins_missing": dict(
        reads=R[:3], edges=[(1, 3, 2), (3, 5, 2)],
        want=dict(path_node=[1, 3, 5], path_pos=[0, 2, 4], path_off=[0, 3], len=[12], edges=[], seq=["ACGTTGCAAGGC"]),
        info=dict(edges_sym=4, twins_added=2, compactable=4, cycles_cut=0, longest_nodes=3, longest_bases=12)),
    # A forks into B and C, both join in D: nothing is compactable; a unitig of one node has its even node as `+`
    "fork_and_join": dict(
        reads=R[:4], edges=[(1, 3, 2), (1, 5, 3), (3, 7, 3), (5, 7, 2), (2, 0, 2), (4, 0, 3), (6, 2, 3), (6, 4, 2)],
        want=dict(path_node=[0, 2, 4, 6], path_pos=[0, 0, 0, 0], path_off=[0, 1, 2, 3, 4], len=[8, 8, 8, 8],
                  edges=[(0, 2, 2), (0, 4, 3), (2, 6, 3), (3, 1, 2), (4, 6, 2), (5, 1, 3), (7, 3, 3), (7, 5, 2)],
                  seq=[_rc(R[0]), _rc(R[1]), _rc(R[2]), _rc(R[3])]),
        info=dict(edges_sym=8, twins_added=0, compactable=0, cycles_cut=0, longest_nodes=1)),
    "self_loop": dict(
        reads=[A8], edges=[(1, 1, 3)],
        want=dict(path_node=[0], path_pos=[0], path_off=[0, 1], len=[8], edges=[(0, 0, 3), (1, 1, 3)], seq=["TTTTTTTT"]),
        info=dict(edges_sym=2, twins_added=1, compactable=0)),
    # u -> u^1 is its own twin
    "self_twin_edge": dict(
        reads=[A8], edges=[(1, 0, 2)],
        want=dict(path_node=[0], path_pos=[0], path_off=[0, 1], len=[8], edges=[(0, 1, 2)], seq=["TTTTTTTT"]),
        info=dict(edges_sym=1, twins_added=0, compactable=0)),
    # ring 1 -> 3 -> 5 -> 1 and its twin ring 4 -> 2 -> 0 -> 4: m = 0 lies in the twin ring, its in-edge 2 -> 0 and the twin of that, 1 -> 3, are cut:
    # 0 -> 4 -> 2 (head 0, `+`) and 3 -> 5 -> 1
    "ring_and_twin_ring": dict(
        reads=[A8, C8, G8], edges=[(1, 3, 2), (3, 5, 2), (5, 1, 2)],
        want=dict(path_node=[0, 4, 2], path_pos=[0, 2, 4], path_off=[0, 3], len=[12], edges=[(0, 0, 6), (1, 1, 6)], seq=["TTCCGGGGGGGG"]),
        info=dict(edges_sym=6, twins_added=3, compactable=4, cycles_cut=1, longest_nodes=3)),
    # 1 -> 3 -> 2 -> 0 -> 1 is its own twin: 3 -> 2 and 0 -> 1 are edges u -> u^1, never compactable; [1, 3] and its twin [2, 0] remain
    "ring_own_twin": dict(
        reads=[A8, C8], edges=[(1, 3, 2), (3, 2, 2), (2, 0, 2), (0, 1, 2)],
        want=dict(path_node=[1, 3], path_pos=[0, 2], path_off=[0, 2], len=[10], edges=[(0, 1, 4), (1, 0, 4)], seq=["AACCCCCCCC"]),
        info=dict(edges_sym=4, twins_added=0, compactable=2, cycles_cut=0)),
    "parallel_edges_two_offsets": dict(
        reads=[A8, C8], edges=[(1, 3, 4), (1, 3, 2)],
        want=dict(path_node=[1, 3], path_pos=[0, 2], path_off=[0, 2], len=[10], edges=[], seq=["AACCCCCCCC"]),
        info=dict(edges_sym=2, twins_added=1, compactable=2)),
    # offset 0: node 1 contributes no base (the last node at a position spells it)
    "offset0_chain": dict(
        reads=[A8, C8, G8], edges=[(1, 3, 0), (3, 5, 3)],
        want=dict(path_node=[1, 3, 5], path_pos=[0, 0, 3], path_off=[0, 3], len=[11], edges=[], seq=["CCCGGGGGGGG"]),
        info=dict(edges_sym=4, compactable=4)),
    # a -> b -> a with offset 0 both ways: a cycle of two; the twin cycle 2 -> 0 -> 2 holds m = 0: cut 2 -> 0 and 1 -> 3
    "offset0_two_cycle": dict(
        reads=[A8, C8], edges=[(1, 3, 0), (3, 1, 0)],
        want=dict(path_node=[0, 2], path_pos=[0, 0], path_off=[0, 2], len=[8], edges=[(0, 0, 0), (1, 1, 0)], seq=["GGGGGGGG"]),
        info=dict(edges_sym=4, twins_added=2, compactable=2, cycles_cut=1)),
    # read 2 (nodes 4, 5) has no edge at all
    "isolated_nodes": dict(
        reads=[A8, C8, G8], edges=[(1, 3, 2)],
        want=dict(path_node=[1, 3, 4], path_pos=[0, 2, 0], path_off=[0, 2, 3], len=[10, 8], edges=[], seq=["AACCCCCCCC", "CCCCCCCC"]),
        want_skip=dict(path_node=[1, 3], path_pos=[0, 2], path_off=[0, 2], len=[10], edges=[], seq=["AACCCCCCCC"]),
        info=dict(edges_sym=2, twins_added=1, compactable=2), isolated=1),
}

# (reads, lens override or None, edges): each must be refused
REFUSALS = {
    "twin_lengths_differ": ([A8, C8], {0: 7}, [(1, 3, 2)]),
    "id_out_of_range": ([A8, C8], None, [(1, 4, 2)]),
    "negative_id": ([A8, C8], None, [(-1, 3, 2)]),
    "dead_endpoint": ([A8, C8], {2: 0, 3: 0}, [(1, 3, 2)]),
    "negative_offset": ([A8, C8], None, [(1, 3, -1)]),
    "offset_not_below_len": ([A8, C8], None, [(1, 3, 8)]),
    "contained_target": ([A8, "CCCC"], None, [(1, 3, 2)]),          # 2 + 4 < 8: the twin's offset would be negative
}


def refusal_nodes(name):
    reads, override, edges = REFUSALS[name]
    words, lens = nodes_of(reads)
    lens = lens.copy()
    for k, v in (override or {}).items():
        lens[k] = v
    return words, lens, np.array(edges, dtype=np.int32).reshape(-1, 3)


def expected(case, skip_isolated):
    c = CASES[case]
    return c["want_skip"] if skip_isolated and "want_skip" in c else c["want"]


def assert_equals_expected(u, case, skip_isolated):
    c, w = CASES[case], expected(case, skip_isolated)
    assert u["n_pairs"] == len(w["len"])
    assert u["path_node"].tolist() == w["path_node"]
    assert u["path_pos"].tolist() == w["path_pos"]
    assert [int(x) for x in u["path_off"]] == w["path_off"]
    assert u["len"].tolist() == w["len"]
    assert [tuple(x) for x in u["edges"].tolist()] == w["edges"]
    import unitig_checker as U
    assert [U.sequence(u, k) for k in range(u["n_pairs"])] == w["seq"]
    assert [int(x) for x in u["word_off"]] == np.concatenate([[0], np.cumsum((np.array(w["len"], dtype=np.int64) + 15) // 16)]).astype(int).tolist()
    for k, v in c["info"].items():
        assert u["info"][k] == v, k
    assert u["info"]["isolated_skipped"] == (c.get("isolated", 0) if skip_isolated else 0)


# ---- the reference's graph dumps -------------------------------------------------------------------------------------------
GOLDEN_GRAPHS = ["f1_cfg1.graph", "f1_cfg1.aftercut.graph", "f2_err2.graph", "f2_err2.aftercut.graph", "f3_paired.graph", "f4_varlen.graph",
                 "f4_varlen.aftercut.graph", "f5_messy.graph", "f5_messy.aftercut.graph", "f6_l40.graph", "f7_pkb.supplement.graph", "f7_pkb.aftercut.graph"]
ERROR_FREE = ("f1_cfg1", "f3_paired", "f6_l40")
# live nodes, edges of E*, oriented unitigs, nodes of the longest path: the prototype's figures (a cross-check, not the specification)
GOLDEN_TABLE = {"f1_cfg1.graph": (15766, 15838, 80, 3326), "f1_cfg1.aftercut.graph": (15766, 15764, 2, 7883), "f3_paired.graph": (8418, 8436, 24, 4181),
                "f6_l40.graph": (6452, 6450, 2, 3226), "f2_err2.graph": (11994, 3290, 11796, 3), "f2_err2.aftercut.graph": (11994, 2818, 11684, 4),
                "f4_varlen.graph": (6730, 15928, 6446, 3), "f4_varlen.aftercut.graph": (6730, 13960, 6248, 4), "f5_messy.graph": (6904, 17036, 6766, 3),
                "f5_messy.aftercut.graph": (6904, 14548, 6558, 3), "f7_pkb.supplement.graph": (11994, 6468, 11876, 4),
                "f7_pkb.aftercut.graph": (11994, 3932, 11292, 9)}

_cache = {}


def golden(golden_dir, graph):
    """(words, lens, edges) of one dump; node sets are cached per fixture"""
    fixture = graph.split(".")[0]
    if fixture not in _cache:
        if fixture == "f7_pkb":
            _cache[fixture] = O.load_nodes_bin(os.path.join(golden_dir, "f7_pkb.nodes.bin.gz"))
        else:
            fx = O.Fixture(golden_dir, fixture)
            try:
                f1, f2 = fx.inputs()
                lo, rs = fx.explicit_params()
                nd = O.ingest(f1, f2, min_overlap=lo, rsoemo=rs)
            finally:
                fx.cleanup()
            _cache[fixture] = (nd["words"], nd["len"])
    words, lens = _cache[fixture]
    with gzip.open(os.path.join(golden_dir, graph + ".gz"), "rb") as f:
        n, e = O.parse_graph(f.read())
    assert n == len(lens)
    return words, lens, e
