"""Dangling-branch removal on the GPU (alga_remove_dangling_branches_device): the surviving edges and the per-pass counts equal the Python
restatement (tests/tips_checker.py, `keep` empty) on the reference's graphs after the cut and after the restated MST step, on the read
sets and dense graphs of tests/graph_cases.py, on 200 random graphs, on inputs that need many iterations and one that meets the
reference's early stop; refusals; the unitigs of the clipped graph; the command line."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import gfa_writer as G
import graph_cases as GC
import oracle_lib as O
import tips_checker as T
import unitig_cases as K
import unitig_checker as U

pytestmark = pytest.mark.gpu
BOUNDS = (0, 1, 60, 10 ** 6)


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def clip_equals(eng, n, edges, bound, what=""):
    """device == restatement: edge list and per-pass counts; -> (edges as numpy, info)"""
    import torch
    want, counts = T.remove_dangling_branches(n, edges, bound)
    got, info = eng.remove_dangling_branches(n, edges, bound)
    print(what, "bound", bound, "passes", counts, "branching", info["branching_nodes"], "overflow", info["overflow_nodes"])
    assert torch.equal(got.cpu(), torch.from_numpy(want)), what
    assert torch.equal(torch.tensor(info["removed"], dtype=torch.int64), torch.tensor(counts, dtype=torch.int64)), (what, info["removed"], counts)
    assert info["passes"] == len(counts) == 2 * info["iterations"] and info["removed_total"] == sum(counts)
    assert info["edges_in"] == len(edges) and info["edges_out"] == len(want) == info["edges_unique"] - sum(counts)
    return want, info


def golden_bound(golden_dir, name):
    meta = json.load(open(os.path.join(golden_dir, "n5_aftersimplifier.json")))
    return meta[name]["max_offset_dangling_branches"] if name in meta else 377


def after_mst(n, edges, bound):
    g = T.graph_from_edges(n, edges)
    T.remove_short_parallel_paths(g, bound)
    return T.edges_from_graph(g)


@pytest.mark.parametrize("name", ["f2_err2", "f4_varlen", "f7_pkb"])
def test_reference_graphs_after_the_cut_and_after_the_mst_step(eng, golden_dir, name):
    with gzip.open(os.path.join(golden_dir, name + ".aftercut.graph.gz"), "rb") as f:
        n, cut = O.parse_graph(f.read())
    bound = golden_bound(golden_dir, name)
    mst = after_mst(n, cut, bound)
    assert 0 < len(mst) < len(cut)
    removed = 0
    for what, e in (("after the cut", cut), ("after the MST step", mst)):
        for b in (bound,) + BOUNDS:
            _, info = clip_equals(eng, n, e, b, "%s %s" % (name, what))
            removed += info["removed_total"]
        # the order of the input does not matter
        perm = np.random.default_rng(11).permutation(len(e))
        clip_equals(eng, n, np.ascontiguousarray(e[perm]), bound, "%s %s, shuffled" % (name, what))
    assert removed > 0


@pytest.mark.parametrize("name", sorted(GC.SETS))
def test_read_sets(eng, name):
    r = GC.reads_of(name)
    built, cut = GC.oracle_graphs(name)
    bound = int(GC.MOPP * GC.READ_LEN / np.float32(100))
    clip_equals(eng, len(r.lens), cut, bound, name + " after the cut")
    if len(r.lens) <= 50000:
        clip_equals(eng, len(r.lens), built, bound, name + " as built")
        clip_equals(eng, len(r.lens), cut, 10 ** 6, name + " after the cut")


def test_dense_graphs_take_the_overflow_route(eng):
    """parallel edges, self-loops, rows of 100 .. 300 edges: the pre-reduction and the overflow route"""
    overflow = 0
    for name in sorted(GC.DENSE):
        n, e, _, _ = GC.dense_case(name)
        for b in GC.DENSE_MOPP + (0,):
            _, info = clip_equals(eng, n, e, b, name)
            overflow += info["overflow_nodes"]
            assert info["edges_unique"] == len(np.unique(e[:, :2], axis=0))
        for b in (7, 10 ** 6):
            _, info = clip_equals(eng, n, GC.thinned(name), b, name + " thinned")
            overflow += info["overflow_nodes"]
    assert overflow > 0


def random_graph(rng):
    """chains with tips, sparse and dense random graphs; self-loops, parallel edges and zero offsets among them"""
    kind = int(rng.integers(0, 4))
    n = int(rng.integers(2, 2001 if kind != 2 else 120))
    m = int(rng.integers(0, [int(1.3 * n) + 1, 3 * n, n * n // 2 + 1, 2 * n][kind]))
    e = np.stack([rng.integers(0, n, m), rng.integers(0, n, m), rng.integers(0, [1, 4, 30, 200][int(rng.integers(0, 4))], m)], axis=1)
    if kind == 0 and n > 5:
        spine = np.stack([np.arange(n - 1), np.arange(1, n), rng.integers(0, 20, n - 1)], axis=1)
        e = np.concatenate([e, spine[rng.random(n - 1) < 0.9]])
    return n, np.ascontiguousarray(e, dtype=np.int32), int([0, 1, 5, 30, 100, 10 ** 6][int(rng.integers(0, 6))])


def test_200_random_graphs(eng):
    most = 0
    for seed in range(200):
        n, e, bound = random_graph(np.random.default_rng(4000 + seed))
        _, info = clip_equals(eng, n, e, bound, "seed %d" % seed)
        most = max(most, info["iterations"])
    assert most >= 3


def fork_tree(depth, bound):
    """A complete binary tree of out-edges of offset 1 under node 1, whose parent 0 also has an edge of offset bound + 1 (never a tip).  A
    fork of two tips loses one per iteration, and only then is what is left a tip of the fork above: iteration j clips 2^(depth - j) chains
    of j edges, iteration depth + 1 the last chain."""
    e = [(0, 1, 1), (0, 2, bound + 1)]
    level, nxt = [1], 3
    for _ in range(depth):
        new = []
        for v in level:
            e += [(v, nxt, 1), (v, nxt + 1, 1)]
            new += [nxt, nxt + 1]
            nxt += 2
        level = new
    return nxt, np.array(e, dtype=np.int32)


def test_input_that_needs_more_than_three_iterations(eng):
    n, e = fork_tree(5, 100)
    want, info = clip_equals(eng, n, e, 100, "fork tree of depth 5")
    assert info["iterations"] == 7 and info["removed"][::2] == [16, 16, 12, 8, 5, 6, 0] and len(want) == 1


def test_early_stop_of_the_reference(eng):
    """depth 16: iteration i = 15 clips one chain of 16 edges, 0 < 16 <= 30, so the loop stops (src/GraphSimplifiers/GraphSimplifier.cpp:212)
    although the next iteration would have clipped the chain that is left"""
    n, e = fork_tree(16, 100)
    want, info = clip_equals(eng, n, e, 100, "fork tree of depth 16")
    assert info["iterations"] == 16 and info["removed"][30] == 16 and info["removed"][31] == 0
    assert len(want) == 2 + 16                                               # the last chain is still there
    _, again = clip_equals(eng, n, want, 100, "what the early stop left")
    assert again["removed"] == [17, 0, 0, 0] and again["edges_out"] == 1           # the chain of 16 and the edge 0 -> 1 above it


@pytest.mark.parametrize("bad", [(3, 4, -1), (3, 8, 5), (-1, 2, 5), (8, 0, 0)])
def test_refusals_write_nothing(eng, bad):
    import torch
    n, e = 8, np.array([(0, 1, 1), (0, 2, 11), (1, 3, 1), (1, 4, 1), (2, 5, 2), (5, 6, 0), (7, 0, 3)], dtype=np.int32)
    got, _ = eng.remove_dangling_branches(n, e, 10)
    snap = got.clone()
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.remove_dangling_branches(n, np.concatenate([e, np.array([bad], dtype=np.int32)]), 10)
    assert ei.value.code == -1
    assert torch.equal(got, snap)                                            # the previous result is untouched
    assert torch.equal(eng.remove_dangling_branches(n, e, 10)[0], snap)      # and the engine usable
    with pytest.raises(alga_amd.AlgaError):
        eng.remove_dangling_branches(0, e, 10)
    assert eng.remove_dangling_branches(0, np.zeros((0, 3), np.int32), 10)[1]["removed"] == [0, 0]


def _unitig_arrays(u):
    return {k: u[k] for k in ("n_pairs", "words", "word_off", "len", "path_node", "path_pos", "path_off", "edges")}


@pytest.mark.parametrize("ruling", [0, 1])
@pytest.mark.parametrize("name", ["f2_err2", "f4_varlen"])
def test_unitigs_of_the_clipped_graph(eng, golden_dir, name, ruling):
    words, lens, cut = K.golden(golden_dir, name + ".aftercut.graph")
    bound = golden_bound(golden_dir, name)
    want_edges, _ = T.remove_dangling_branches(len(lens), cut, bound)
    clipped, info = eng.remove_dangling_branches(len(lens), cut, bound)
    assert info["removed_total"] > 0
    try:
        eng.set_option("unitig_ruling", ruling)
        for skip in (False, True):
            got = eng.unitigs(words, lens, clipped, skip_isolated=skip).to_host()        # the device list goes straight in
            want = U.unitigs(words, lens, want_edges, skip_isolated=skip)
            assert got["n_pairs"] == want["n_pairs"]
            for k, v in _unitig_arrays(want).items():
                assert np.array_equal(got[k], v), (k, skip)
        if name == "f2_err2":
            before = eng.unitigs(words, lens, cut, skip_isolated=True).info
            after = eng.unitigs(words, lens, clipped, skip_isolated=True)
            unclipped_pairs = U.unitigs(words, lens, cut, skip_isolated=True)["n_pairs"]
            print("f2 unitigs (pairs, longest bases): unclipped", unclipped_pairs, before["longest_bases"], "clipped", after.n_pairs, after.info["longest_bases"])
            assert after.n_pairs <= unclipped_pairs and after.info["longest_bases"] >= before["longest_bases"]
    finally:
        eng.set_option("unitig_ruling", -1)


def test_cli_clips_tips_before_the_unitigs(golden_dir, tmp_path):
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    fx = O.Fixture(golden_dir, "f2_err2")
    try:
        f1, _ = fx.inputs()
        out, plain = str(tmp_path / "clipped.gfa"), str(tmp_path / "plain.gfa")
        for path, extra in ((out, ["--clip_tips=1"]), (plain, [])):
            r = subprocess.run([exe, "--file1=" + f1, "--output=o.fasta", "--unitigs=" + path] + extra, cwd=str(tmp_path), stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            assert ("Tips clipped" in r.stderr) == bool(extra)
    finally:
        fx.cleanup()
    words, lens, cut = K.golden(golden_dir, "f2_err2.aftercut.graph")
    # the bound as the reference derives it: the mean length of the reads the cut graph still has an edge at
    live = np.zeros(len(lens), dtype=bool)
    live[cut[:, 0]] = True; live[cut[:, 1]] = True
    avg = float(lens[live & (lens > 0)].astype(np.float64).mean())
    bound = int(262 * avg / np.float32(100))
    assert bound == golden_bound(golden_dir, "f2_err2")
    clipped, _ = T.remove_dangling_branches(len(lens), cut, bound)

    def gfa(edges):
        want = U.unitigs(words, lens, edges, skip_isolated=True)
        rows = U.padded_rows(want)
        w2 = np.zeros((2 * want["n_pairs"], rows.shape[1]), dtype=np.uint32)
        w2[1::2] = rows
        return G.gfa_bytes(w2, np.repeat(want["len"], 2), want["edges"], twins=True, sequences=True)[0]

    assert open(out, "rb").read() == gfa(clipped)
    assert open(plain, "rb").read() == gfa(cut)                              # without the option: as before
