"""Removal of short parallel paths on the GPU (alga_remove_short_parallel_paths_device): the lists equal the Python restatement of the
reference's sequential step (tests/tips_checker.py: remove_short_parallel_paths), entry for entry, on the reference's graphs after the cut, on
the read sets and dense graphs of tests/graph_cases.py and on 200 random graphs; the rounds equal the schedule stated in tests/mst_schedule.py;
determinism; the chain paths -> clip -> unitigs; refusals; the command line.

The device claims EXACT balls (mst_walk.h: mst_ball computes shortest distances), so `rounds` and `winners` are asserted equal to what
tests/mst_schedule.py computes, not merely bounded by it."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import gfa_writer as G
import graph_cases as GC
import mst_schedule as S
import oracle_lib as O
import tips_checker as T
import unitig_cases as K
import unitig_checker as U

pytestmark = pytest.mark.gpu
BOUNDS = (0, 1, 60, 1000)


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def restated(n, edges, bound):
    g = T.graph_from_edges(n, edges)
    T.remove_short_parallel_paths(g, bound)
    return T.edges_from_graph(g)


def paths_equal(eng, n, edges, bound, what="", schedule=False):
    """device == restatement, list for list; with `schedule` also the rounds -> (edges as numpy, info)"""
    import torch
    want = restated(n, edges, bound)
    got, info = eng.remove_short_parallel_paths(n, edges, bound)
    print(what, "bound", bound, "edges", info["edges_in"], "->", info["edges_out"], "rounds", info["rounds"], "winners", info["winners"][:8], "begs",
          info["begs_run"], "of", info["branching_nodes"], "overflow", info["overflow_begs"], "largest ball", info["ball_max"],
          "ms %.3f + %.3f" % (info["ms_prepare"], info["ms_rounds"]))
    assert torch.equal(got.cpu(), torch.from_numpy(want)), what
    assert info["edges_in"] == len(edges) and info["edges_out"] == len(want)
    assert info["begs_run"] <= info["branching_nodes"] and len(info["winners"]) == min(info["rounds"], alga_amd.engine.MST_MAX_ROUNDS)
    assert info["rounds"] <= info["begs_run"] and (info["rounds"] > 0) == (info["begs_run"] > 0)
    if info["rounds"] <= alga_amd.engine.MST_MAX_ROUNDS:
        assert sum(info["winners"]) == info["begs_run"]
    if schedule:
        h = T.graph_from_edges(n, edges)
        s = S.remove_short_parallel_paths_rounds(h, bound)
        assert (info["rounds"], info["begs_run"], info["branching_nodes"], info["ball_max"]) == (s["rounds"], s["begs_run"], s["branching_nodes"], s["ball_max"]), (what, s)
        assert info["winners"] == s["winners"][: alga_amd.engine.MST_MAX_ROUNDS]
    return want, info


def recorded(golden_dir, name):
    meta = json.load(open(os.path.join(golden_dir, "n5_aftersimplifier.json")))
    return meta.get(name)


def recorded_bound(golden_dir, name):
    c = recorded(golden_dir, name)
    return c["max_offset_parallel_paths_scaled"] if c else {"f7_pkb": 377, "f5_messy": 283}[name]


def after_cut(golden_dir, name):
    with gzip.open(os.path.join(golden_dir, name + ".aftercut.graph.gz"), "rb") as f:
        return O.parse_graph(f.read())


@pytest.mark.parametrize("name", ["f2_err2", "f4_varlen", "f5_messy", "f7_pkb"])
def test_reference_graphs_after_the_cut(eng, golden_dir, name):
    n, cut = after_cut(golden_dir, name)
    bound = recorded_bound(golden_dir, name)
    want, info = paths_equal(eng, n, cut, bound, name, schedule=True)
    assert 0 < len(want) < len(cut) and info["rounds"] > 1
    c = recorded(golden_dir, name)
    if c:
        assert info["edges_out"] == c["edges_after_mst"] == {"f2_err2": 2735, "f4_varlen": 6756}[name]
    for b in BOUNDS:
        paths_equal(eng, n, cut, b, name, schedule=(b == 60))


def test_nothing_branches_in_f1_cfg1(eng, golden_dir):
    import torch
    n, cut = after_cut(golden_dir, "f1_cfg1")
    for b in (recorded_bound(golden_dir, "f1_cfg1"),) + BOUNDS:
        want, info = paths_equal(eng, n, cut, b, "f1_cfg1", schedule=True)
        assert info["rounds"] == 0 and info["branching_nodes"] == 0 and info["winners"] == []
        assert np.array_equal(want, cut) and info["edges_out"] == recorded(golden_dir, "f1_cfg1")["edges_after_mst"] == 15764
    got, _ = eng.remove_short_parallel_paths(n, torch.from_numpy(cut).to("cuda:0"), 235)              # a device tensor goes in as it is
    assert torch.equal(got.cpu(), torch.from_numpy(cut))


@pytest.mark.parametrize("name", sorted(GC.SETS))
def test_read_sets(eng, name):
    r = GC.reads_of(name)
    _, cut = GC.oracle_graphs(name)
    bound = int(GC.MOPP * GC.READ_LEN / np.float32(100))
    paths_equal(eng, len(r.lens), cut, bound, name + " after the cut")
    paths_equal(eng, len(r.lens), cut, 60, name + " after the cut")


def test_dense_graphs_take_the_overflow_route(eng):
    """Parallel edges, self-loops, rows of 100 .. 300 edges: the hubs' state does not fit into LDS.  Bounds 3, 7 and 0 of the offsets 0 .. 40
    these graphs have.  Their third bound in the other graph tests, 250, is left to the thinned graphs here: with it every ball of a dense graph
    is everything the beg reaches, about 1500 nodes, no two pending begs are independent (one winner per round, about 1450 rounds of 2000
    balls each: the worst case that tests/test_mst_schedule_cpu.py pins on a chain), which costs minutes and shows nothing the thinned graphs,
    the chain below and the random graphs at a bound of 10^6 do not.
    Every graph with a hub must take the overflow route at bounds 3 and 7 (a hub's row alone is more than a state in LDS collects); plain_off6
    has no hub and rows of a handful of edges, so whether one of its begs outgrows LDS is a matter of the bound alone: it is counted into the
    sum, not required; at bound 0 a beg collects only its own zero-offset entries."""
    overflow = 0
    for name in sorted(GC.DENSE):
        n, e, _, _ = GC.dense_case(name)
        for b in (3, 7, 0):
            _, info = paths_equal(eng, n, e, b, name)
            overflow += info["overflow_begs"]
            assert info["overflow_begs"] > 0 or b == 0 or GC.DENSE[name][5] == 0, name          # every graph with a hub takes the route
        t = GC.thinned(name)
        for b in (7, 250, 10 ** 6):
            paths_equal(eng, n, t, b, name + " thinned")
    assert overflow > 0


def test_second_overflow_tier(eng, golden_dir):
    """With first-tier states of 8 nodes, whatever LDS (192 nodes, 256 edges) cannot hold cannot be held there either: it reaches the states
    sized for the whole graph."""
    n, cut = after_cut(golden_dir, "f4_varlen")
    dn, de, _, _ = GC.dense_case("parallel_off9_1hub")
    try:
        eng.set_option("mst_mid_nodes", 8)
        _, info = paths_equal(eng, n, cut, 1000, "f4_varlen, second tier")
        assert info["overflow_begs"] > 0
        _, info = paths_equal(eng, dn, de, 7, "parallel_off9_1hub, second tier")
        assert info["overflow_begs"] > 0
    finally:
        eng.set_option("mst_mid_nodes", 4096)


def test_200_random_graphs(eng):
    most, overflow = 0, 0
    for seed in range(200):
        n, e, bound = S.random_graph(np.random.default_rng(4000 + seed), n_max=600)
        _, info = paths_equal(eng, n, e, bound, "seed %d" % seed, schedule=(n <= 150))
        most = max(most, info["rounds"])
        overflow += info["overflow_begs"]
    assert most >= 10 and overflow > 0


def test_ids_ascending_along_a_chain(eng):
    n, e = S.ascending_chain(150)
    _, info = paths_equal(eng, n, e, 10 ** 6, "ascending chain", schedule=True)
    assert info["rounds"] == info["begs_run"] > alga_amd.engine.MST_MAX_ROUNDS                    # one winner per round: the worst case
    _, info = paths_equal(eng, n, e, -1, "negative bound")                                         # nothing is ever expanded
    assert info["rounds"] == 1 and info["edges_out"] == len(e)


def test_two_calls_give_identical_bytes(eng, golden_dir):
    import torch
    n, cut = after_cut(golden_dir, "f4_varlen")
    a, ia = eng.remove_short_parallel_paths(n, cut, 321)
    a = a.clone()
    b, ib = eng.remove_short_parallel_paths(n, cut, 321)
    assert torch.equal(a, b) and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert {k: v for k, v in ia.items() if not k.startswith("ms_")} == {k: v for k, v in ib.items() if not k.startswith("ms_")}


def _unitig_arrays(u):
    return {k: u[k] for k in ("n_pairs", "words", "word_off", "len", "path_node", "path_pos", "path_off", "edges")}


@pytest.mark.parametrize("ruling", [0, 1])
@pytest.mark.parametrize("name", ["f2_err2", "f4_varlen"])
def test_paths_then_clip_then_unitigs(eng, golden_dir, name, ruling):
    import torch
    words, lens, cut = K.golden(golden_dir, name + ".aftercut.graph")
    bound = recorded_bound(golden_dir, name)
    want_edges, _ = T.remove_dangling_branches(len(lens), restated(len(lens), cut, bound), bound)
    mst, info = eng.remove_short_parallel_paths(len(lens), cut, bound)
    assert info["edges_out"] < len(cut)
    clipped, tinfo = eng.remove_dangling_branches(len(lens), mst, bound)                 # the device list goes straight in
    assert torch.equal(clipped.cpu(), torch.from_numpy(want_edges)) and tinfo["removed_total"] > 0
    try:
        eng.set_option("unitig_ruling", ruling)
        for skip in (False, True):
            got = eng.unitigs(words, lens, clipped, skip_isolated=skip).to_host()
            want = U.unitigs(words, lens, want_edges, skip_isolated=skip)
            assert got["n_pairs"] == want["n_pairs"]
            for k, v in _unitig_arrays(want).items():
                assert np.array_equal(got[k], v), (k, skip)
        # the paths' own output goes into the unitigs as well
        got = eng.unitigs(words, lens, eng.remove_short_parallel_paths(len(lens), cut, bound)[0], skip_isolated=True).to_host()
        want = U.unitigs(words, lens, restated(len(lens), cut, bound), skip_isolated=True)
        for k, v in _unitig_arrays(want).items():
            assert np.array_equal(got[k], v), k
    finally:
        eng.set_option("unitig_ruling", -1)


def test_device_chain_gives_the_reference_dump_of_f1_cfg1(eng, golden_dir):
    c = recorded(golden_dir, "f1_cfg1")
    assert c["keep"] == []                                                   # the reference skipped no removal: the comparison below is with all of its simplifier
    n, cut = after_cut(golden_dir, "f1_cfg1")
    mst, _ = eng.remove_short_parallel_paths(n, cut, c["max_offset_parallel_paths_scaled"])
    clipped, tinfo = eng.remove_dangling_branches(n, mst, c["max_offset_dangling_branches"])
    assert tinfo["removed"] == c["pass_counts"]
    with gzip.open(os.path.join(golden_dir, "f1_cfg1.aftersimplifier.graph.gz"), "rb") as f:
        assert O.graph_bytes(n, clipped.cpu().numpy()) == f.read()


@pytest.mark.parametrize("bad", [[(3, 4, -1)], [(3, 8, 5)], [(-1, 2, 5)], [(8, 0, 0)], [(7, 1, 1), (6, 1, 1)]])
def test_refusals_write_nothing(eng, bad):
    import torch
    n, e = 8, np.array([(0, 1, 1), (0, 2, 2), (0, 2, 11), (1, 2, 1), (1, 3, 1), (1, 4, 1), (2, 5, 2), (5, 6, 0)], dtype=np.int32)
    got, info = eng.remove_short_parallel_paths(n, e, 10)
    assert info["edges_out"] < len(e)
    snap = got.clone()
    bad = np.array(bad, dtype=np.int32)
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.remove_short_parallel_paths(n, np.concatenate([e, bad]), 10)
    assert ei.value.code == -1
    assert torch.equal(got, snap)                                                # the previous result is untouched
    assert torch.equal(eng.remove_short_parallel_paths(n, e, 10)[0], snap)       # and the engine usable
    with pytest.raises(alga_amd.AlgaError):
        eng.remove_short_parallel_paths(n, np.ascontiguousarray(e[::-1]), 10)    # not grouped by src
    with pytest.raises(alga_amd.AlgaError):
        eng.remove_short_parallel_paths(0, e, 10)
    out, info = eng.remove_short_parallel_paths(0, np.zeros((0, 3), np.int32), 10)
    assert out.shape == (0, 3) and info["rounds"] == 0 and info["winners"] == [] and info["edges_out"] == 0
    out, info = eng.remove_short_parallel_paths(5, np.zeros((0, 3), np.int32), 10)
    assert out.shape == (0, 3) and info["rounds"] == 0


def test_cli_removes_parallel_paths_before_the_clip(golden_dir, tmp_path):
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    fx = O.Fixture(golden_dir, "f2_err2")
    files = {"both": ["--parallel_paths=1", "--clip_tips=1"], "paths": ["--parallel_paths=1"], "clip": ["--clip_tips=1"], "plain": [], "off": ["--parallel_paths=0"]}
    try:
        f1, _ = fx.inputs()
        for key, extra in files.items():
            r = subprocess.run([exe, "--file1=" + f1, "--output=o.fasta", "--unitigs=" + str(tmp_path / (key + ".gfa"))] + extra, cwd=str(tmp_path),
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            assert ("Short parallel paths removed" in r.stderr) == ("--parallel_paths=1" in extra)
            assert ("Tips clipped" in r.stderr) == ("--clip_tips=1" in extra)
            if key == "both":
                line = [x for x in r.stderr.splitlines() if x.startswith("Short parallel paths removed")][0]
                print(line)
                assert "bound 377 " in line and " 2735 edges out, 18 rounds" in line
    finally:
        fx.cleanup()
    words, lens, cut = K.golden(golden_dir, "f2_err2.aftercut.graph")
    # the bound as the reference derives it: the mean length of the reads the cut graph still has an edge at
    live = np.zeros(len(lens), dtype=bool)
    live[cut[:, 0]] = True; live[cut[:, 1]] = True
    avg = float(lens[live & (lens > 0)].astype(np.float64).mean())
    bound = int(262 * avg / np.float32(100))
    assert bound == recorded_bound(golden_dir, "f2_err2")
    mst = restated(len(lens), cut, bound)
    both, _ = T.remove_dangling_branches(len(lens), mst, bound)
    clipped, _ = T.remove_dangling_branches(len(lens), cut, bound)

    def gfa(edges):
        want = U.unitigs(words, lens, edges, skip_isolated=True)
        rows = U.padded_rows(want)
        w2 = np.zeros((2 * want["n_pairs"], rows.shape[1]), dtype=np.uint32)
        w2[1::2] = rows
        return G.gfa_bytes(w2, np.repeat(want["len"], 2), want["edges"], twins=True, sequences=True)[0], want["n_pairs"]

    read = lambda key: open(str(tmp_path / (key + ".gfa")), "rb").read()
    assert read("both") == gfa(both)[0]
    assert read("paths") == gfa(mst)[0]
    assert read("clip") == gfa(clipped)[0]                                   # without the option: as before
    assert read("plain") == gfa(cut)[0] == read("off")
    pairs = lambda key: sum(1 for x in read(key).split(b"\n") if x.startswith(b"S\t"))
    print("f2_err2 unitig pairs: cut", pairs("plain"), "cut + clip", pairs("clip"), "cut + paths + clip", pairs("both"))
    assert pairs("both") == gfa(both)[1] and pairs("both") <= pairs("clip") <= pairs("plain")
