"""Hand-made graphs for the contigs (include/alga_amd.h: alga_contigs_device) with their answers written out: tests/test_contigs_cpu.py holds
the Python definition (tests/contig_checker.py) to them, tests/test_gpu_contigs.py the device.

Node sets are lengths only (read k = node 2k+1, its twin 2k; 100 nt unless a case says otherwise) over pseudo-random rows: every edge is a
dovetail, the rows matter to the spelled sequences alone.  Edges are given in the forward direction; E* adds the twins.  `want`: the layout
arrays and the contig graph; `info`: the counts that must come out (per-round lists in full).

The issue's "bubble tied in weight and key, with v in one chain and v^1 in the other" cannot be built: the twin of the second chain runs through
v too, so v has two successors and is no path node (case tie_through_v_and_its_twin shows what happens instead: all eight edges are contigs
of their own).  Two open chains of one group never tie in (weight, key): an interior node lies in one chain only, and E* holds one edge
per (src, dst)."""
import numpy as np


def nodes_of(n_reads, lens=None):
    L = np.full(2 * n_reads, 100, dtype=np.int32)
    for k, v in (lens or {}).items():
        L[2 * k] = L[2 * k + 1] = v
    stride = (int(L.max()) + 15) // 16
    rows = np.random.RandomState(n_reads * 7919 + int(L.sum())).randint(0, 1 << 32, size=(2 * n_reads, stride), dtype=np.uint64).astype(np.uint32)
    for v in range(2 * n_reads):                                          # bits behind the length are zero, as in every packed row
        used = int(L[v])
        for w in range(stride):
            keep = min(max(used - 16 * w, 0), 16)
            rows[v, w] &= np.uint32((1 << (2 * keep)) - 1)
    return rows, L


CASES = {
    # 1 -> 3 -> 5: one chain, the unitig
    "plain_chain": dict(
        reads=3, max_offset=100, edges=[(1, 3, 10), (3, 5, 10)],
        want=dict(path_node=[1, 3, 5], path_pos=[0, 10, 20], path_off=[0, 3], len=[120], edges=[]),
        info=dict(edges_sym=4, rounds=1, chains=[2], parallel_drops=[0], groups_cut=[0], base_edges_dropped=[0], final_edges=4, path_nodes=2,
                  junction_nodes=4, cycles_cut=0, closed_chains=0, reads_dropped=0, longest_nodes=3, longest_bases=120, total_bases=120)),
    # Z -> A, A -> B, A -> C (a fork; its twin is a join): read A (nodes 0 / 1) is in all three contigs
    "fork_and_join": dict(
        reads=4, max_offset=100, edges=[(7, 1, 10), (1, 3, 10), (1, 5, 20)],
        want=dict(path_node=[0, 6, 1, 3, 1, 5], path_pos=[0, 10, 0, 10, 0, 20], path_off=[0, 2, 4, 6], len=[110, 110, 120],
                  edges=[(0, 3, 10), (0, 5, 10), (2, 1, 10), (4, 1, 20)]),
        info=dict(edges_sym=6, rounds=1, chains=[6], final_edges=6, path_nodes=0, junction_nodes=8, reads_dropped=0)),
    # S -> A, A -> B -> D (20), A -> C -> D (60), D -> T; the bound above 60: the heavy chain goes, round 2 makes one contig
    "bubble_heavy_below_bound": dict(
        reads=6, max_offset=100, edges=[(1, 3, 10), (3, 5, 10), (5, 9, 10), (3, 7, 30), (7, 9, 30), (9, 11, 10)],
        want=dict(path_node=[1, 3, 5, 9, 11], path_pos=[0, 10, 20, 30, 40], path_off=[0, 5], len=[140], edges=[]),
        info=dict(edges_sym=12, rounds=2, chains=[8, 2], parallel_drops=[2, 0], groups_cut=[0, 0], base_edges_dropped=[4, 0], final_edges=8,
                  path_nodes=6, junction_nodes=4, reads_dropped=2, longest_nodes=5)),
    # ... the bound below 60: both chains stay (Graph::contractPath refuses the heavy one)
    "bubble_heavy_above_bound": dict(
        reads=6, max_offset=50, edges=[(1, 3, 10), (3, 5, 10), (5, 9, 10), (3, 7, 30), (7, 9, 30), (9, 11, 10)],
        want=dict(path_node=[1, 3, 3, 5, 9, 3, 7, 9, 9, 11], path_pos=[0, 10, 0, 10, 20, 0, 30, 60, 0, 10], path_off=[0, 2, 5, 8, 10],
                  len=[110, 120, 160, 110],
                  edges=[(1, 3, 10), (1, 5, 10), (2, 0, 20), (3, 7, 20), (4, 0, 60), (5, 7, 60), (6, 2, 10), (6, 4, 10)]),
        info=dict(edges_sym=12, rounds=1, chains=[8], parallel_drops=[0], groups_cut=[0], base_edges_dropped=[0], final_edges=12, path_nodes=4,
                  junction_nodes=8, reads_dropped=0)),
    # A -> C (20) against A -> B -> C (10 + 10): equal weights, the direct edge has no interior and loses
    "direct_edge_loses": dict(
        reads=3, max_offset=100, edges=[(1, 5, 20), (1, 3, 10), (3, 5, 10)],
        want=dict(path_node=[1, 3, 5], path_pos=[0, 10, 20], path_off=[0, 3], len=[120], edges=[]),
        info=dict(edges_sym=6, rounds=2, chains=[4, 2], parallel_drops=[2, 0], groups_cut=[0, 0], base_edges_dropped=[2, 0], final_edges=4, reads_dropped=0)),
    # A -> B -> D and A -> C -> D, both 20: read B (1) < read C (2), the chain through B stays
    "equal_bubble_by_read_index": dict(
        reads=4, max_offset=100, edges=[(1, 5, 10), (5, 7, 10), (1, 3, 10), (3, 7, 10)],
        want=dict(path_node=[1, 3, 7], path_pos=[0, 10, 20], path_off=[0, 3], len=[120], edges=[]),
        info=dict(edges_sym=8, rounds=2, chains=[4, 2], parallel_drops=[2, 0], base_edges_dropped=[4, 0], final_edges=4, reads_dropped=2)),
    # A -> v -> D and A -> v^1 -> D (v = 3): v and v^1 get two successors each, nothing is a path node, every edge is a contig
    "tie_through_v_and_its_twin": dict(
        reads=4, max_offset=100, edges=[(1, 3, 10), (3, 7, 10), (1, 2, 10), (2, 7, 10)],
        want=dict(path_node=[1, 2, 1, 3, 2, 7, 3, 7], path_pos=[0, 10, 0, 10, 0, 10, 0, 10], path_off=[0, 2, 4, 6, 8], len=[110, 110, 110, 110],
                  edges=[(1, 2, 10), (1, 5, 10), (3, 0, 10), (3, 7, 10), (4, 0, 10), (4, 7, 10), (6, 2, 10), (6, 5, 10)]),
        info=dict(edges_sym=8, rounds=1, chains=[8], parallel_drops=[0], groups_cut=[0], final_edges=8, path_nodes=0, junction_nodes=6)),
    # a -> x -> c (10 + 10) against a -> c (20), x a junction (x -> y): the chains are single edges, the cut of H removes a -> c
    "triangle_through_a_junction": dict(
        reads=4, max_offset=100, edges=[(1, 3, 10), (3, 5, 10), (1, 5, 20), (3, 7, 50)],
        want=dict(path_node=[1, 3, 3, 5, 3, 7], path_pos=[0, 10, 0, 10, 0, 50], path_off=[0, 2, 4, 6], len=[110, 110, 150],
                  edges=[(1, 3, 10), (1, 5, 10), (2, 0, 10), (4, 0, 50)]),
        info=dict(edges_sym=8, rounds=2, chains=[8, 6], parallel_drops=[0, 0], groups_cut=[2, 0], base_edges_dropped=[2, 0], final_edges=6, reads_dropped=0)),
    # the same with len[c] = 150 and the bound 60: a -> c weighs 20, its twin 70 > 60 -- the cut removes only a -> c, the twin condition the other
    "triangle_only_the_twin_too_heavy": dict(
        reads=4, lens={2: 150}, max_offset=60, edges=[(1, 3, 10), (3, 5, 10), (1, 5, 20), (3, 7, 50)],
        want=dict(path_node=[1, 3, 3, 5, 3, 7], path_pos=[0, 10, 0, 10, 0, 50], path_off=[0, 2, 4, 6], len=[110, 160, 150],
                  edges=[(1, 3, 10), (1, 5, 10), (2, 0, 60), (4, 0, 50)]),
        info=dict(edges_sym=8, rounds=2, chains=[8, 6], parallel_drops=[0, 0], groups_cut=[1, 0], base_edges_dropped=[2, 0], final_edges=6)),
    # S -> A, A -> B -> D (20) | A -> C -> D (60), D -> T: 40 in all; S -> E -> T weighs 50.  Round 1 removes A-C-D, only then S .. T is one
    # chain and round 2 removes S-E-T, round 3 finds nothing
    "nested_bubbles_three_rounds": dict(
        reads=7, max_offset=100, edges=[(1, 3, 10), (3, 5, 10), (5, 9, 10), (3, 7, 30), (7, 9, 30), (9, 11, 10), (1, 13, 25), (13, 11, 25)],
        want=dict(path_node=[1, 3, 5, 9, 11], path_pos=[0, 10, 20, 30, 40], path_off=[0, 5], len=[140], edges=[]),
        info=dict(edges_sym=16, rounds=3, chains=[10, 4, 2], parallel_drops=[2, 2, 0], groups_cut=[0, 0, 0], base_edges_dropped=[4, 4, 0], final_edges=8,
                  reads_dropped=4, path_nodes=6, junction_nodes=4)),
    # 1 -> 3 -> 5 -> 1 and the twin ring 4 -> 2 -> 0 -> 4: m = 0 lies in the twin ring; 0 and 1 leave P and both rings are closed chains
    "pure_ring": dict(
        reads=3, max_offset=100, edges=[(1, 3, 10), (3, 5, 10), (5, 1, 10)],
        want=dict(path_node=[0, 4, 2, 0], path_pos=[0, 10, 20, 30], path_off=[0, 4], len=[130], edges=[(0, 0, 30), (1, 1, 30)]),
        info=dict(edges_sym=6, rounds=1, chains=[2], final_edges=6, path_nodes=4, junction_nodes=2, cycles_cut=1, closed_chains=2, longest_nodes=4)),
    # T -> R1, R1 -> R2 -> R3 -> R1: R1 is a junction, the ring a closed chain from it
    "ring_with_tail": dict(
        reads=4, max_offset=100, edges=[(1, 3, 10), (3, 5, 10), (5, 7, 10), (7, 3, 10)],
        want=dict(path_node=[1, 3, 2, 6, 4, 2], path_pos=[0, 10, 0, 10, 20, 30], path_off=[0, 2, 6], len=[110, 130],
                  edges=[(1, 2, 10), (2, 2, 30), (3, 0, 30), (3, 3, 30)]),
        info=dict(edges_sym=8, rounds=1, chains=[4], final_edges=8, path_nodes=4, junction_nodes=4, cycles_cut=0, closed_chains=2)),
    # S -> A, A -> T, A -> L -> A: the loop is a closed chain (c = a) and takes no part in the groups
    "loop_back_to_its_junction": dict(
        reads=4, max_offset=100, edges=[(1, 3, 10), (3, 5, 10), (3, 7, 10), (7, 3, 10)],
        want=dict(path_node=[1, 3, 2, 6, 2, 3, 5], path_pos=[0, 10, 0, 10, 20, 0, 10], path_off=[0, 2, 5, 7], len=[110, 120, 110],
                  edges=[(1, 2, 10), (1, 5, 10), (2, 2, 20), (2, 5, 20), (3, 0, 20), (3, 3, 20), (4, 0, 10), (4, 3, 10)]),
        info=dict(edges_sym=8, rounds=1, chains=[6], final_edges=8, path_nodes=2, junction_nodes=6, closed_chains=2)),
    # A -> H -> A^1 (3 -> 5 -> 2): its twin is 3 -> 4 -> 2, also from A: c = a^1, a closed chain; (3, 4) < (3, 5) is `+`
    "hairpin": dict(
        reads=3, max_offset=100, edges=[(3, 5, 10), (5, 2, 10)],
        want=dict(path_node=[3, 4, 2], path_pos=[0, 10, 20], path_off=[0, 3], len=[120], edges=[]),
        info=dict(edges_sym=4, rounds=1, chains=[2], final_edges=4, path_nodes=2, junction_nodes=2, closed_chains=2)),
    # 1 -> 0 is its own twin: one chain, once
    "self_twin_edge": dict(
        reads=1, max_offset=100, edges=[(1, 0, 10)],
        want=dict(path_node=[1, 0], path_pos=[0, 10], path_off=[0, 2], len=[110], edges=[]),
        info=dict(edges_sym=1, rounds=1, chains=[1], final_edges=1, path_nodes=0, junction_nodes=2, closed_chains=1)),
    # read 2 (nodes 4, 5) has no edge: it is in no contig
    "isolated_node": dict(
        reads=3, max_offset=100, edges=[(1, 3, 10)],
        want=dict(path_node=[1, 3], path_pos=[0, 10], path_off=[0, 2], len=[110], edges=[]),
        info=dict(edges_sym=2, rounds=1, chains=[2], final_edges=2, path_nodes=0, junction_nodes=4, reads_dropped=0)),
    "empty_edge_list": dict(
        reads=2, max_offset=100, edges=[],
        want=dict(path_node=[], path_pos=[], path_off=[0], len=[], edges=[]),
        info=dict(edges_sym=0, rounds=1, chains=[0], parallel_drops=[0], groups_cut=[0], base_edges_dropped=[0], final_edges=0, path_nodes=0,
                  junction_nodes=0, closed_chains=0, longest_nodes=0, longest_bases=0, total_bases=0)),
}


def inputs(name):
    c = CASES[name]
    words, lens = nodes_of(c["reads"], c.get("lens"))
    return words, lens, np.array(c["edges"], dtype=np.int32).reshape(-1, 3), c["max_offset"]


def spelled(words, lens, path_node, path_pos, L):
    """The sequence of one contig straight from step 8: base j comes from the LAST entry with pos <= j (codes, uint8)"""
    out = np.zeros(L, dtype=np.uint8)
    for v, p in zip(path_node, path_pos):
        q = np.arange(int(lens[v]))
        out[p: p + int(lens[v])] = (words[v, q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & 3
    return out


def assert_equals_expected(u, name):
    c = CASES[name]
    w = c["want"]
    assert u["n_pairs"] == len(w["len"]), name
    assert u["path_node"].tolist() == w["path_node"], name
    assert u["path_pos"].tolist() == w["path_pos"], name
    assert [int(x) for x in u["path_off"]] == w["path_off"], name
    assert u["len"].tolist() == w["len"], name
    assert [tuple(x) for x in u["edges"].tolist()] == w["edges"], name
    assert [int(x) for x in u["word_off"]] == np.concatenate([[0], np.cumsum((np.array(w["len"], dtype=np.int64) + 15) // 16)]).astype(int).tolist()
    for k, v in c["info"].items():
        assert u["info"][k] == v, (name, k, u["info"][k], v)
    words, lens, _, _ = inputs(name)
    wo = [int(x) for x in u["word_off"]]
    for k, L in enumerate(w["len"]):
        a, b = w["path_off"][k], w["path_off"][k + 1]
        want = spelled(words, lens, w["path_node"][a:b], w["path_pos"][a:b], L)
        row = u["words"][wo[k]: wo[k + 1]]
        q = np.arange(L)
        assert (((row[q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & 3) == want).all(), (name, k)
