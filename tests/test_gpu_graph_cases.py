"""The graph stages on the GPU (overlap build, triangle cut, unitig graph, the two GFA writers, the command line) on the inputs of
tests/graph_cases.py: reads of rings, of rings beside a linear chromosome, of a ring with a repeat, and dense random graphs with
parallel edges, self-loops and rows of hundreds of edges.  Every comparison is exact: arrays, counters, list order, file bytes
against the CPU oracle, tests/unitig_checker.py and tests/gfa_writer.py; on top of that, what the genomes alone say about the device's
result (self-link offset == ring length, rotation, every read inside its unitig).  Every unitig test runs in both ranking forms.

Left out: nothing of the issue's list.  The 400 kb ring runs with the other sets and once more three ways (test_ring_400k_three_ways)."""
import math
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import gfa_writer as G
import graph_cases as GC
import oracle_lib as O
import unitig_checker as U
from alga_amd import workload
from test_gpu_unitig import _dev, _unitig_gfa_want, assert_same

pytestmark = pytest.mark.gpu
RING_SETS = sorted(k for k, s in GC.SETS.items() if s["rings_only"])


@pytest.fixture(scope="module", params=["jumping", "ruling_set"])
def eng(request):
    """every unitig test twice, as in tests/test_gpu_unitig.py: plain pointer jumping, and with the ruling set ranked first"""
    e = alga_amd.Engine(0)
    e.ruling = request.param == "ruling_set"
    e.set_option("unitig_ruling", 1 if e.ruling else 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cut_eng():
    """the triangle cut does not rank anything: once"""
    e = alga_amd.Engine(0)
    yield e
    e.close()


def unitigs_equal(eng, w, l, want_of, edges, d_edges=None, shuffle_seed=None):
    """device == checker with and without SKIP_ISOLATED, and for a shuffled edge order; want_of(skip) -> the checker's result.
    -> the device result without the flag (host copies)"""
    first = None
    for skip in (False, True):
        want = want_of(skip)
        u = eng.unitigs(w, l, d_edges[0] if d_edges else edges, n_edges=d_edges[1] if d_edges else None, skip_isolated=skip)
        got = u.to_host()
        assert_same(got, want, "skip=%s" % skip)
        if shuffle_seed is not None and len(edges):
            perm = np.random.default_rng(shuffle_seed).permutation(len(edges))
            assert_same(eng.unitigs(w, l, np.ascontiguousarray(edges[perm]), skip_isolated=skip).to_host(), want, "shuffled, skip=%s" % skip)
        first = first or got
    return first


def build_and_cut(eng, name):
    """build and cut on the device, both equal to the oracle's; -> (reads, w, l, (d, m) of the cut graph, its host copy)"""
    r = GC.reads_of(name)
    built, cut = GC.oracle_graphs(name)
    w, l = _dev(eng, r.words, r.lens)
    d, m = eng.prefsuf_device(w, l, GC.MIN_OVERLAP, GC.RSOEMO)
    e = alga_amd.engine.device_edges_to_numpy(d, m)
    assert e.shape == built.shape and (e == built).all()
    d2, m2, removed = eng.cut_triangles_device(len(r.lens), d, m, GC.MOPP)
    e2 = alga_amd.engine.device_edges_to_numpy(d2, m2)
    assert e2.shape == cut.shape and (e2 == cut).all()                       # list order included
    assert removed == m - m2
    return r, w, l, (d2, m2), e2


@pytest.mark.parametrize("name", sorted(GC.SETS))
def test_read_set(eng, name):
    """build == oracle, cut (host and device form) == oracle with list order, unitigs of the raw and of the cut graph == checker"""
    r = GC.reads_of(name)
    built, cut = GC.oracle_graphs(name)
    n = len(r.lens)
    w, l = _dev(eng, r.words, r.lens)
    host_cut = eng.cut_triangles_host(n, built, GC.MOPP)
    assert host_cut.shape == cut.shape and (host_cut == cut).all()
    d, m = eng.prefsuf_device(w, l, GC.MIN_OVERLAP, GC.RSOEMO)
    e = alga_amd.engine.device_edges_to_numpy(d, m)
    assert e.shape == built.shape and (e == built).all()
    raw = unitigs_equal(eng, w, l, lambda skip: GC.checker(name, False, skip), e, d_edges=(d, m), shuffle_seed=11)
    GC.assert_reads_in_unitigs(r, raw)
    d2, m2, removed = eng.cut_triangles_device(n, d, m, GC.MOPP)
    e2 = alga_amd.engine.device_edges_to_numpy(d2, m2)
    assert e2.shape == cut.shape and (e2 == cut).all()
    assert removed == m - m2 == len(built) - len(cut)
    assert (alga_amd.engine.device_edges_to_numpy(d, m) == built).all()      # the input of the cut is untouched
    got = unitigs_equal(eng, w, l, lambda skip: GC.checker(name, True, skip), e2, d_edges=(d2, m2), shuffle_seed=12)
    print(name, "ruling" if eng.ruling else "jumping", eng.unitigs(w, l, d2, n_edges=m2).info)
    # on the device result itself, without the checker
    GC.assert_reads_in_unitigs(r, got)
    if GC.SETS[name]["rings_only"]:
        GC.assert_ring_facts(r, got)
        skipped = eng.unitigs(w, l, d2, n_edges=m2, skip_isolated=True).to_host()
        GC.assert_ring_facts(r, skipped)
    p = GC.PINNED[name]["after_cut"]
    i = got["info"]
    assert (got["n_pairs"], i["cycles_cut"], i["longest_nodes"], i["longest_bases"], len(got["edges"])) == \
        (p["pairs"], p["cycles_cut"], p["longest_nodes"], p["longest_bases"], p["unitig_edges"])


def test_ring_400k_three_ways():
    """option 0, option 1, and an engine whose option was never set (240 000 nodes >= 2^16: the ruling set by default): one result.
    The cut ring is ONE path of longest_nodes nodes, ranked by plain jumping after the cycle phase: ceil(log2(longest_nodes - 1))
    rounds for the node furthest from the head, and at least one round before the cut (the one that finds the cycle nodes open)."""
    name = "ring_400k"
    r = GC.reads_of(name)
    want = GC.checker(name, True)
    cut = GC.oracle_graphs(name)[1]
    res = {}
    for form, opt in (("jumping", 0), ("ruling", 1), ("unset", None)):
        e = alga_amd.Engine(0)
        try:
            if opt is not None:
                e.set_option("unitig_ruling", opt)
            u = e.unitigs(r.words, r.lens, cut)
            res[form] = (u.to_host(), u.info["rank_rounds"])
        finally:
            e.close()
        print(form, u.info)
        assert_same(res[form][0], want, form)
        GC.assert_ring_facts(r, res[form][0])
    assert_same(res["ruling"][0], res["jumping"][0])
    assert_same(res["unset"][0], res["jumping"][0])
    longest = want["info"]["longest_nodes"]
    assert longest == 120000
    assert res["jumping"][1] > math.ceil(math.log2(longest - 1))
    assert res["unset"][1] == res["ruling"][1] and res["unset"][1] != res["jumping"][1]


def _sorted_edges(e):
    return np.ascontiguousarray(e[np.lexsort((e[:, 2], e[:, 1], e[:, 0]))])


@pytest.mark.parametrize("name", RING_SETS + ["rings_and_linear"])
def test_gfa_of_cut_rings(eng, tmp_path, name):
    """unitig GFA (sequences on and off, 1 MB chunks) and the read-level GFA of the cut graph, byte for byte; a cut ring is a segment
    linked to itself: its two self-links are ONE L line"""
    r, w, l, (d2, m2), e2 = build_and_cut(eng, name)
    path = str(tmp_path / "u.gfa")
    try:
        eng.set_option("gfa_chunk_mb", 1)
        for skip in (False, True):
            want = GC.checker(name, True, skip)
            u = eng.unitigs(w, l, d2, n_edges=m2, skip_isolated=skip)
            for seqs in (True, False):
                info = eng.write_unitig_gfa(path, u, sequences=seqs)
                text, winfo = _unitig_gfa_want(want, seqs)
                got = open(path, "rb").read()
                os.unlink(path)
                assert got == text
                for k in ("segments", "links", "links_merged", "bytes"):
                    assert info[k] == winfo[k], k
                lines = got.split(b"\n")
                if GC.SETS[name]["rings_only"]:
                    rings = len(r.genomes)
                    assert sum(x.startswith(b"S\t") for x in lines) == rings and sum(x.startswith(b"L\t") for x in lines) == rings
                    assert info["links_merged"] == rings
                    for k in range(rings):                                   # L k - k - <L - G>M: the - strand's edge sorts first
                        G_ = int(want["edges"][2 * k, 2])
                        assert b"L\t%d\t-\t%d\t-\t%dM" % (k, k, int(want["len"][k]) - G_) in lines
        # the read-level graph after the cut (sorted by (src, dst, offset), as the writer wants it)
        es = _sorted_edges(e2)
        for seqs in (True, False):
            info = eng.write_gfa(path, w, l, es, sequences=seqs)
            text, winfo = G.gfa_bytes(r.words, r.lens, es, sequences=seqs)
            assert open(path, "rb").read() == text
            os.unlink(path)
            for k in ("segments", "links", "links_merged", "bytes"):
                assert info[k] == winfo[k], k
            assert info["links"] == info["links_merged"] == m2 // 2          # every overlap once
    finally:
        eng.set_option("gfa_chunk_mb", 256)


def test_cli_on_three_rings(tmp_path):
    """alga_hip --unitigs= --gfa= on a FASTA of the three-ring set (with a hundred records twice: the ingest stage drops them) against
    the oracle's ingest + build + cut of the same file and the checker"""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    codes = GC.read_codes(GC.reads_of("three_rings"))
    codes = np.concatenate([codes, codes[100:200]])
    fasta = str(tmp_path / "rings.fasta")
    workload.write_fasta_fast(fasta, codes)
    out, gfa = str(tmp_path / "unitigs.gfa"), str(tmp_path / "reads.gfa")
    r = subprocess.run([exe, "--file1=" + fasta, "--output=o.fasta", "--unitigs=" + out, "--gfa=" + gfa], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Unitigs written" in r.stderr
    nd = O.ingest(fasta)
    words, lens = nd["words"], nd["len"]
    assert int((lens > 0).sum()) == 2 * (len(codes) - 100)
    e, _, _ = O.prefsuf(words, lens, nd["min_overlap"], nd["rsoemo"])
    cut = O.cut_triangles(len(lens), e, max(250, int(1.75 * nd["LEN"])))
    want = U.unitigs(words, lens, cut, skip_isolated=True)
    assert (want["n_pairs"], want["info"]["cycles_cut"]) == (3, 3)          # (the end trimming leaves the rings closed)
    assert sorted(want["edges"][0::2, 2].tolist()) == [1200, 3000, 30000]
    text = open(out, "rb").read()
    assert text == _unitig_gfa_want(want, True)[0]
    assert text.count(b"\nS\t") == 3 and text.count(b"\nL\t") == 3
    assert open(gfa, "rb").read() == G.gfa_bytes(words, lens, e)[0]


@pytest.mark.parametrize("mopp", GC.DENSE_MOPP)
@pytest.mark.parametrize("name", sorted(GC.DENSE))
def test_dense_cut(cut_eng, name, mopp):
    """rows of hundreds of edges, several edges to one neighbour, self-loops, equal path sums by the thousand: host and device form
    equal the oracle (which equals the literal restatement: tests/test_graph_cases_cpu.py), list order included"""
    import torch
    n, e, _, _ = GC.dense_case(name)
    want = O.cut_triangles(n, e, mopp)
    got = cut_eng.cut_triangles_host(n, e, mopp)
    assert got.shape == want.shape and (got == want).all()
    d = torch.from_numpy(e).cuda()
    ptr, m, removed = cut_eng.cut_triangles_device(n, d.data_ptr(), len(e), mopp, stream=torch.cuda.current_stream().cuda_stream)
    dev = alga_amd.engine.device_edges_to_numpy(ptr, m)
    assert dev.shape == want.shape and (dev == want).all()
    assert removed == len(e) - m == len(e) - len(want)
    assert (d.cpu().numpy() == e).all()                                      # the input is untouched
    print(name, mopp, "edges", len(e), "removed", removed)


@pytest.mark.parametrize("name", sorted(GC.DENSE))
def test_dense_unitigs(eng, name):
    """every dense graph is a legal unitig input once each node has a row longer than the largest offset: before the cut, after it
    (device form, lists in the reference's order), and thinned to one edge in ten (where edges are compactable)"""
    import torch
    n, e, words, lens = GC.dense_case(name)
    w, l = _dev(eng, words, lens)
    unitigs_equal(eng, w, l, lambda skip: U.unitigs(words, lens, e, skip_isolated=skip), e, shuffle_seed=21)
    for mopp in (7, 250):
        d = torch.from_numpy(e).cuda()
        ptr, m, _ = eng.cut_triangles_device(n, d.data_ptr(), len(e), mopp, stream=torch.cuda.current_stream().cuda_stream)
        cut = alga_amd.engine.device_edges_to_numpy(ptr, m)
        assert (cut == O.cut_triangles(n, e, mopp)).all()
        unitigs_equal(eng, w, l, lambda skip: U.unitigs(words, lens, cut, skip_isolated=skip), cut, d_edges=(ptr, m), shuffle_seed=22)
    thin = GC.thinned(name)
    got = unitigs_equal(eng, w, l, lambda skip: U.unitigs(words, lens, thin, skip_isolated=skip), thin, shuffle_seed=23)
    assert got["info"]["compactable"] > 100
