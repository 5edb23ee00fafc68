"""Inputs for the graph stages (triangle cut, unitig graph, GFA export) that a linear iid genome never makes: reads of circular
replicons -- after the triangle cut every ring is ONE cycle of compactable edges --, a ring with a repeat (the graph branches), rings
beside a linear chromosome, and dense random graphs full of triangles, parallel edges, self-loops and rows of hundreds of edges.

tests/test_graph_cases_cpu.py pins what the CPU side (oracle build, oracle cut, tests/unitig_checker.py) makes of every set and checks
the Python restatement of the cut below against the oracle; tests/test_gpu_graph_cases.py runs the device on the same inputs.

The read sets are handed to the engine as node sets, without the ingest stage, so the start positions are DISTINCT per replicon: two
equal reads (which the ingest stage would drop) overlap each other with offset 0 both ways, and a graph of thousands of such 2-cycles
hides the ring."""
import collections

import numpy as np

import alga_amd
import oracle_lib as O
import unitig_checker as U

READ_LEN, MIN_OVERLAP, RSOEMO = 100, 55, 77
MOPP = max(250, int(1.75 * READ_LEN))                    # the cap of the triangle cut as src/main.cpp derives it

Reads = collections.namedtuple("Reads", "words lens genomes circular replicon start strand")


def replicon_reads(circular, linear, n, length, seed, copy=None, first=None):
    """Reads of iid genomes: `circular` / `linear` are the replicon lengths (the circular ones come first in the numbering of the
    replicons), `n` the number of reads of every replicon (a list) or of all together (an int: shared out in proportion to the
    lengths).  A read is a window of `length` bases -- round the end of a circular replicon -- at a start no other read of its
    replicon has, on a random strand; the order is shuffled across the replicons.  copy = (from, to, len) writes bases
    [from, from + len) of replicon 0 over [to, to + len) before the reads are taken (a read that lies inside the second copy is left
    out when the same read of the first copy is there: no two reads are equal).  first = r swaps a read of replicon r to index 0
    (pair 0 then lies on that replicon's path or cycle).
    -> Reads: words / lens in the twin layout (node 2k+1 = read k, 2k its reverse complement), the genomes (uint8 codes), and per
    read its replicon, start and strand (1 = reverse complement of the window)."""
    rng = np.random.default_rng(seed)
    sizes = list(circular) + list(linear)
    genomes = [rng.integers(0, 4, size=g, dtype=np.uint8) for g in sizes]
    if copy is not None:
        a, b, c = copy
        genomes[0][b: b + c] = genomes[0][a: a + c].copy()
    if isinstance(n, int):
        n = [n * g // sum(sizes) for g in sizes]
    codes, rep, starts = [], [], []
    for r, (g, k) in enumerate(zip(sizes, n)):
        ring = r < len(circular)
        s = np.sort(rng.choice(g if ring else g - length + 1, size=k, replace=False))
        if copy is not None and r == 0:
            # a window inside the second copy spells what the window at the same place of the first does: one of the two is enough
            a, b, c = copy
            s = s[~((s >= b) & (s + length <= b + c) & np.isin(s - b + a, s))]
        codes.append(genomes[r][(s[:, None] + np.arange(length)[None, :]) % g])
        rep.append(np.full(k, r, dtype=np.int32))
        starts.append(s.astype(np.int64))
    codes, rep, starts = np.concatenate(codes), np.concatenate(rep), np.concatenate(starts)
    strand = (rng.random(len(codes)) < 0.5).astype(np.int8)
    perm = rng.permutation(len(codes))
    if first is not None:
        j = int(np.nonzero(rep[perm] == first)[0][0])
        perm[[0, j]] = perm[[j, 0]]
    codes, rep, starts, strand = codes[perm], rep[perm], starts[perm], strand[perm]
    rc = (3 - codes)[:, ::-1]
    fwd = np.where(strand[:, None] == 1, rc, codes)
    both = np.stack([(3 - fwd)[:, ::-1], fwd], axis=1).reshape(2 * len(codes), length)
    lens = np.full(2 * len(codes), length, dtype=np.int32)
    return Reads(alga_amd.pack_reads(both, lens), lens, genomes, len(circular), rep, starts, strand)


# name -> the arguments of replicon_reads.  `rings_only`: every replicon is a ring without a repeat, so after the cut the graph is one
# cycle per ring and the structural facts of the CPU test hold (pairs == replicons, one self-link of offset G per ring).
SETS = {
    "ring_20k": dict(circular=[20000], linear=[], n=6000, seed=101, rings_only=True),
    "three_rings": dict(circular=[30000, 3000, 1200], linear=[], n=12000, seed=102, rings_only=True),
    # the 40 kb chromosome is linear: its path is ranked while the two rings stand still; a ring read is pair 0 (k_ut_cut with v == 0)
    "rings_and_linear": dict(circular=[30000, 1200], linear=[40000], n=23000, seed=103, first=0, rings_only=False),
    # bases [2000, 2400) once more 15 kb further on: the graph branches at both ends of the repeat.  After the cut: the repeat and the
    # two arcs between its copies, three unitigs that are no cycles, joined by 8 unitig edges
    "ring_with_repeat": dict(circular=[30000], linear=[], n=10000, seed=104, copy=(2000, 17000, 400), rings_only=False),
    # 240 000 nodes >= 2^16: the size from which the ruling set is the default
    "ring_400k": dict(circular=[400000], linear=[], n=120000, seed=105, rings_only=True),
    # a ring of 40 reads whose 80 node ids hold NO sampled id of the ruling set (ut_sampled: one id in 64) beside a ring that holds
    # about a hundred: no ruler ever walks the short ring or its twin, the ruler phase leaves them to the rounds after it.  Which
    # ring holds how many is SAMPLED_IDS below.  The seed has to be one for which the short ring holds none AND closes (40 reads on
    # 300 bases: a gap wider than READ_LEN - MIN_OVERLAP = 45 opens it); the CPU test shows both for 106.
    "short_ring_beside_ring": dict(circular=[20000, 300], linear=[], n=[6000, 40], seed=106, rings_only=True),
}


def ut_sampled(v):
    """k_ut_ruler_flags' choice of the ruling set (unitig_kernels.hip: ut_sampled), in numpy"""
    return ((np.asarray(v, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(26) == 0


def sampled_ids(reads):
    """per replicon: how many of its nodes (both strands) the ruling set samples"""
    ids = np.arange(len(reads.lens))
    hit = ut_sampled(ids)
    return [int(hit[np.repeat(reads.replicon, 2) == r].sum()) for r in range(len(reads.genomes))]


_cache = {}


def reads_of(name):
    if ("reads", name) not in _cache:
        a = dict(SETS[name])
        a.pop("rings_only")
        _cache["reads", name] = replicon_reads(length=READ_LEN, **a)
    return _cache["reads", name]


def oracle_graphs(name):
    """(edges of the oracle's build, sorted by (src, dst, offset); the oracle's triangle cut of them, lists in the reference's order)"""
    if ("graphs", name) not in _cache:
        r = reads_of(name)
        e, _, _ = O.prefsuf(r.words, r.lens, MIN_OVERLAP, RSOEMO)
        _cache["graphs", name] = (e, O.cut_triangles(len(r.lens), e, MOPP))
    return _cache["graphs", name]


def checker(name, after_cut, skip_isolated=False):
    key = ("unitigs", name, after_cut, skip_isolated)
    if key not in _cache:
        r = reads_of(name)
        _cache[key] = U.unitigs(r.words, r.lens, oracle_graphs(name)[1 if after_cut else 0], skip_isolated=skip_isolated)
    return _cache[key]


def figures(name):
    """what PINNED holds for one set, computed afresh on the CPU"""
    out = {}
    for after_cut in (False, True):
        u = checker(name, after_cut)
        i = u["info"]
        out["after_cut" if after_cut else "built"] = dict(edges=len(oracle_graphs(name)[1 if after_cut else 0]), pairs=u["n_pairs"], cycles_cut=i["cycles_cut"],
                                                          longest_nodes=i["longest_nodes"], longest_bases=i["longest_bases"], unitig_edges=len(u["edges"]))
    return out


def read_codes(reads):
    """the reads themselves (the odd nodes) as uint8 codes [n_reads, length]"""
    w = reads.words[1::2]
    c = ((w[:, :, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(len(w), -1)
    return c[:, : int(reads.lens.max())].astype(np.uint8)


def codes_of(u, k):
    """the bases of pair k of a unitig result (checker or device) as uint8 codes"""
    wo = u["word_off"].astype(np.int64)
    w = u["words"][wo[k]: wo[k + 1]]
    q = np.arange(int(u["len"][k]))
    return ((w[q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & 3).astype(np.uint8)


def assert_ring_facts(reads, u):
    """What the unitig graph of reads of rings has to be, whoever computed it (stated from the genomes, without the checker): one
    pair per ring; its two self-links have exactly the ring's length as offset; the first G bases are a rotation of the genome or of its
    reverse complement; the rest repeats the beginning (the last reads run round the cut)."""
    sizes = [len(g) for g in reads.genomes]
    assert u["n_pairs"] == len(sizes) and u["info"]["cycles_cut"] == len(sizes)
    e = u["edges"]
    assert len(e) == 2 * len(sizes)
    assert (e[:, 0] == e[:, 1]).all() and (e[:, 0] == np.arange(2 * len(sizes))).all()
    assert (e[0::2, 2] == e[1::2, 2]).all()
    assert sorted(e[0::2, 2].tolist()) == sorted(sizes)
    assert len(set(sizes)) == len(sizes)
    for k in range(len(sizes)):
        G = int(e[2 * k, 2])
        genome = reads.genomes[sizes.index(G)]
        seq = codes_of(u, k)
        L = len(seq)
        assert G < L < G + READ_LEN
        twice = np.concatenate([genome, genome]).tobytes()
        twice_rc = (3 - np.concatenate([genome, genome]))[::-1].tobytes()
        assert seq[:G].tobytes() in twice or seq[:G].tobytes() in twice_rc
        assert (seq[G:] == seq[: L - G]).all()


def assert_reads_in_unitigs(reads, u):
    """every read of an error-free set is a substring of its unitig at path_pos (vectorised over the nodes, base by base)"""
    pn, pp, po = u["path_node"].astype(np.int64), u["path_pos"].astype(np.int64), u["path_off"].astype(np.int64)
    wo = u["word_off"].astype(np.int64)
    pair_of_entry = np.repeat(np.arange(u["n_pairs"]), np.diff(po))
    lens = reads.lens
    for q in range(int(lens.max())):
        sel = lens[pn] > q
        j = pp[sel] + q
        at = wo[pair_of_entry[sel]] + (j >> 4)
        ucode = (u["words"][at] >> (2 * (j & 15)).astype(np.uint32)) & 3
        ncode = (reads.words[pn[sel], q >> 4] >> np.uint32(2 * (q & 15))) & 3
        assert (ucode == ncode).all(), q


# ---- dense graphs for the triangle cut ------------------------------------------------------------------------------------------
# (n, mean out-degree, largest offset, parallel edges, self-loops, hub rows): neighbours within +-12 ids of the source, so almost every
# edge closes several triangles, and offsets from a handful of values, so that equal path sums are the rule
DENSE = {
    "plain_off6": (1500, 4, 6, False, False, 0),
    "parallel_off9_1hub": (2000, 5, 9, True, False, 1),
    "loops_off12_2hubs": (2500, 4, 12, False, True, 2),
    "parallel_loops_off40_3hubs": (3000, 6, 40, True, True, 3),
}
DENSE_MOPP = (3, 7, 250)


def dense_graph(rng, n, mean_deg, max_off, parallel, loops, hubs):
    """-> edges int32 [m, 3] sorted by (src, dst, offset), no triple twice.  parallel: one edge in five gets a second edge to the same
    neighbour with another offset; loops: one node in ten gets a self-loop (otherwise none); hubs: that many rows get 100 .. 300
    edges to neighbours within +-200 ids (parallel ones among them when `parallel`)."""
    m = n * mean_deg
    src = rng.integers(0, n, size=m)
    d = rng.integers(1, 13, size=m) * rng.choice([-1, 1], size=m)
    e = [np.stack([src, (src + d) % n, rng.integers(1, max_off + 1, size=m)], axis=1)]
    for h in rng.choice(n, size=hubs, replace=False):
        k = int(rng.integers(100, 301))
        d = rng.integers(1, 201, size=k) * rng.choice([-1, 1], size=k)
        e.append(np.stack([np.full(k, h), (h + d) % n, rng.integers(1, max_off + 1, size=k)], axis=1))
    e = np.concatenate(e)
    if loops:
        v = rng.choice(n, size=n // 10, replace=False)
        e = np.concatenate([e, np.stack([v, v, rng.integers(1, max_off + 1, size=len(v))], axis=1)])
    # one (src, dst) once ...
    e = e[np.lexsort((e[:, 2], e[:, 1], e[:, 0]))]
    e = e[np.concatenate([[True], (np.diff(e[:, 0]) != 0) | (np.diff(e[:, 1]) != 0)])]
    if parallel:
        # ... then a second offset for one in five (1 + (o + k) mod max_off with 0 <= k < max_off - 1 is never o)
        twice = e[rng.random(len(e)) < 0.2].copy()
        twice[:, 2] = 1 + (twice[:, 2] + rng.integers(0, max_off - 1, size=len(twice))) % max_off
        e = np.concatenate([e, twice])
        e = e[np.lexsort((e[:, 2], e[:, 1], e[:, 0]))]
    return np.ascontiguousarray(e, dtype=np.int32)


def dense_case(name):
    if ("dense", name) not in _cache:
        n, mean_deg, max_off, parallel, loops, hubs = DENSE[name]
        rng = np.random.default_rng(sorted(DENSE).index(name) + 700)
        e = dense_graph(rng, n, mean_deg, max_off, parallel, loops, hubs)
        # a node set that makes the graph a legal unitig input: every row max_off + 1 random bases long (any offset is a dovetail)
        L = max_off + 1
        lens = np.full(n, L, dtype=np.int32)
        words = alga_amd.pack_reads(rng.integers(0, 4, size=(n, L), dtype=np.uint8), lens)
        _cache["dense", name] = (n, e, words, lens)
    return _cache["dense", name]


def thinned(name):
    """one edge in ten of a dense graph: sparse enough that a few hundred edges are compactable (paths of up to half a dozen nodes, now
    and then a cycle) between the self-loops, u -> u^1 edges and parallel edges -- the dense graphs themselves compact nothing"""
    n, e, words, lens = dense_case(name)
    rng = np.random.default_rng(sorted(DENSE).index(name) + 800)
    return np.ascontiguousarray(e[rng.random(len(e)) < 0.1])


def literal_cut(n, edges, mopp):
    """The first simplifier step written down from the reference's source, container for container:
    Graph::sortEdgesByIncreasingOffset (lists ordered by (offset, neighbour)), the two passes of
    GraphSimplifier::cutNonAndWeaklyMetricTriangles (collect on the unchanged graph, then remove) and Graph::removeDirectedEdge
    (every entry with that neighbour, from the back, swapped with the last and popped).  -> edges [m, 3] grouped by source, in list order"""
    V = [[] for _ in range(n)]
    for a, b, o in np.asarray(edges).tolist():
        V[a].append((b, o))
    for i in range(n):
        V[i].sort(key=lambda p: (p[1], p[0]))
    to_remove = []
    for i in range(n):
        dst = {}
        for a, w1 in V[i]:
            for b, w2 in V[a]:
                dst[b] = min(dst[b], w1 + w2) if b in dst else w1 + w2
        for b, w in V[i]:
            if w > mopp:
                continue
            if b in dst and dst[b] == w:
                to_remove.append((i, b))
    for a, b in to_remove:
        p = len(V[a]) - 1
        for i in range(len(V[a]) - 1, -1, -1):
            if V[a][i][0] == b:
                V[a][i], V[a][p] = V[a][p], V[a][i]
                V[a].pop()
                p -= 1
    out = [(i, b, o) for i in range(n) for b, o in V[i]]
    return np.array(out, dtype=np.int32).reshape(-1, 3)


# ---- what the CPU side makes of every read set: oracle build -> oracle cut -> checker (tests/test_graph_cases_cpu.py recomputes it) ----
def _fig(edges, pairs, cycles_cut, longest_nodes, longest_bases, unitig_edges):
    return dict(edges=edges, pairs=pairs, cycles_cut=cycles_cut, longest_nodes=longest_nodes, longest_bases=longest_bases, unitig_edges=unitig_edges)


# These figures come from the CPU run alone, never from the device.
PINNED = {
    "ring_20k": dict(built=_fig(12013, 14, 0, 5987, 20036, 54), after_cut=_fig(12000, 1, 1, 6000, 20098, 2)),
    "three_rings": dict(built=_fig(24012, 17, 2, 10512, 30041, 62), after_cut=_fig(23998, 3, 3, 10526, 30091, 6)),
    "rings_and_linear": dict(built=_fig(46052, 62, 1, 9675, 30044, 234), after_cut=_fig(45996, 3, 2, 12921, 39994, 4)),
    "ring_with_repeat": dict(built=_fig(19948, 14, 0, 4874, 14790, 50), after_cut=_fig(19938, 3, 0, 4936, 14790, 8)),
    "ring_400k": dict(built=_fig(240409, 446, 0, 11091, 37169, 1710), after_cut=_fig(240000, 1, 1, 120000, 400084, 2)),
    # (this build has no transitive edge: the cut removes nothing, both rings are single cycles from the start)
    "short_ring_beside_ring": dict(built=_fig(12080, 2, 2, 6000, 20096, 4), after_cut=_fig(12080, 2, 2, 6000, 20096, 4)),
}
# per replicon: how many of its node ids the ruling set samples (sampled_ids)
SAMPLED_IDS = {"ring_20k": [188], "three_rings": [330, 38, 8], "rings_and_linear": [306, 7, 407], "ring_with_repeat": [312], "ring_400k": [3750],
               "short_ring_beside_ring": [189, 0]}
