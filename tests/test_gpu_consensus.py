"""The unitig consensus on the GPU (alga_unitig_consensus_device, alga_write_consensus_fasta_device, ALGA_GFA_CONSENSUS): every array equal
to the Python definition (tests/consensus_checker.py) on the reference's graph dumps, the rings and dense graphs of tests/graph_cases.py,
read paths whose genome is known, deep stacks and ties; the full chain from reads with 2 % errors; the FASTA and GFA text; the
reference's own contigs on f1 and f3; refusals; a set of 240 000 nodes with the grids cut down so that every kernel strides."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import consensus_cases as CC
import consensus_checker as S
import gen_reads
import gfa_writer as G
import graph_cases as GC
import oracle_lib as O
import unitig_cases as K
import unitig_checker as U

pytestmark = pytest.mark.gpu
KEYS = ("words", "trim_left", "len", "changed")
COUNTS = ("pairs", "pairs_kept", "columns", "trimmed_bases", "changed")


@pytest.fixture(scope="module", params=["jumping", "ruling_set"])
def eng(request):
    """every test with both forms of the unitig ranking (the consensus reads what either leaves behind)"""
    e = alga_amd.Engine(0)
    e.ruling = request.param == "ruling_set"
    e.set_option("unitig_ruling", 1 if e.ruling else 0)
    yield e
    e.close()


def _dev(eng, words, lens):
    import torch
    dev = torch.device("cuda", eng.device)
    w = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev)
    return w, torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)


def assert_same(got, want, what=""):
    assert got["n_pairs"] == want["n_pairs"], what
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    if got["votes"] is not None:
        assert got["votes"].dtype == np.uint8 and (got["votes"] == want["votes"]).all(), (what, "votes")
    for k in COUNTS:
        assert got["info"][k] == want["info"][k], (what, k)


def equals_checker(eng, words, lens, edges, skips=(False, True), min_votes=(0, 3, 1000)):
    """device == definition for every flag and threshold; -> (unitigs, consensus) of the last combination as host copies"""
    w, l = _dev(eng, words, lens)
    last = None
    for skip in skips:
        u = eng.unitigs(w, l, edges, skip_isolated=skip)
        uh = u.to_host()
        for mv in min_votes:
            want = S.consensus_pileup(words, lens, uh, mv)
            for votes in (False, True):
                c = eng.unitig_consensus(w, l, u, min_votes=mv, votes=votes)
                got = c.to_host()
                assert (got["votes"] is not None) == votes
                assert_same(got, want, "skip=%s min_votes=%d votes=%s" % (skip, mv, votes))
            if mv == 0:
                assert (got["trim_left"] == 0).all() and (got["len"] == uh["len"]).all()
            if mv == 1000:
                assert (got["len"] == 0).all() and (got["trim_left"] == 0).all() and got["info"]["pairs_kept"] == 0
            last = (uh, got)
        assert (u.to_host()["words"] == uh["words"]).all()                   # the unitig result is read, not written
    return last


# ---- (a) fixtures

@pytest.mark.parametrize("graph", ["f1_cfg1.aftercut.graph", "f1_cfg1.aftersimplifier.graph", "f2_err2.aftercut.graph", "f2_err2.aftersimplifier.graph",
                                   "f4_varlen.aftercut.graph", "f4_varlen.aftersimplifier.graph", "f5_messy.aftercut.graph", "f7_pkb.aftercut.graph"])
def test_reference_dump(eng, golden_dir, graph):
    words, lens, edges = K.golden(golden_dir, graph)
    u, c = equals_checker(eng, words, lens, edges)
    print(graph, c["info"])


@pytest.mark.parametrize("name", ["ring_20k", "three_rings", "rings_and_linear", "ring_with_repeat"])
def test_rings(eng, name):
    r = GC.reads_of(name)
    cut = GC.oracle_graphs(name)[1]
    u, c = equals_checker(eng, r.words, r.lens, cut, min_votes=(0, 3))
    # error-free reads: the vote changes nothing, and a ring's window is nearly the whole ring
    assert c["info"]["changed"] == 0 and (c["words"] == u["words"]).all()


@pytest.mark.parametrize("name", sorted(GC.DENSE))
def test_dense_graphs(eng, name):
    """random rows: one-node unitigs throughout the dense graph, paths of a few nodes of RANDOM bases in the thinned one (every column of
    an overlap is a disagreement: ties and 2-1 votes everywhere)"""
    n, e, words, lens = GC.dense_case(name)
    equals_checker(eng, words, lens, e, min_votes=(0, 3))
    u, c = equals_checker(eng, words, lens, GC.thinned(name), min_votes=(0, 1))
    assert c["info"]["changed"] > 0


# ---- (b) stated from the genome alone

@pytest.mark.parametrize("seed,n,err,step", CC.GENOME_CASES + [(11, 2000, 0.05, 10)])
def test_the_vote_restores_the_genome(eng, seed, n, err, step):
    case = CC.genome_path(seed, n, err, step)
    u = eng.unitigs(case.words, case.lens, case.edges)
    assert u.n_pairs == 1
    c = eng.unitig_consensus(case.words, case.lens, u, min_votes=3).to_host()
    uh = u.to_host()
    assert_same(c, S.consensus_pileup(case.words, case.lens, uh, 3))
    if (seed, n, err, step) in CC.GENOME_CASES:                             # (seed 11: see tests/consensus_cases.py)
        g = CC.oriented_genome(case, uh)
        t, L = int(c["trim_left"][0]), int(c["len"][0])
        assert L > len(g) - 200
        assert (CC.columns(uh, c["words"])[t: t + L] == g[t: t + L]).all()    # the window IS the genome ...
        assert (CC.columns(uh, uh["words"])[t: t + L] != g[t: t + L]).sum() > 0.5 * err * L     # ... and the spelled sequence is not


# ---- (c) deep stacks and ties

@pytest.mark.parametrize("n_reads,length,wide", [(400, 500, True), (255, 300, False), (256, 300, True), (400, 250, True), (300, 40, False)])
def test_deep_stacks(eng, n_reads, length, wide):
    """offset 1: 400 reads of 500 nt stand 400 deep; 255 reads fill the 8-bit counters to the brim and 256 are one too many; 400 reads of
    250 nt are never more than 250 deep in a column but up to 265 touch a word; 300 of 40 nt stay shallow"""
    case = CC.stack(40 + n_reads, n_reads, length)
    uh, c = equals_checker(eng, case.words, case.lens, case.edges, skips=(False,), min_votes=(3,))
    touching = min(n_reads, length + 15)                                     # reads that touch the fullest word
    assert c["info"]["max_depth"] == touching
    assert (c["info"]["wide_words"] > 0) == wide == (touching > 255)
    if n_reads == 400 and length == 500:
        assert c["votes"].max() == 255
        assert c["info"]["wide_words"] >= (500 - 400) // 16                  # at least the words under all 400 reads
    g = CC.oriented_genome(case, uh)
    t, L = int(c["trim_left"][0]), int(c["len"][0])
    assert (CC.columns(uh, c["words"])[t: t + L] == g[t: t + L]).all() and c["changed"][0] > 0


def test_ties_and_one_node_unitigs(eng):
    for make in (CC.ties, CC.four_way_tie):
        case, want = make()
        uh, c = equals_checker(eng, case.words, case.lens, case.edges, skips=(False,), min_votes=(0, 1))
        assert (CC.columns(uh, c["words"]) == want).all()
    words, lens = K.nodes_of([K.R[0], K.R[3], K.A8])
    uh, c = equals_checker(eng, words, lens, np.zeros((0, 3), np.int32), skips=(False,), min_votes=(3, 0))
    assert uh["n_pairs"] == 3 and (c["words"] == uh["words"]).all() and (c["changed"] == 0).all() and (c["len"] == 8).all()
    # nothing at all
    u = eng.unitigs(words, lens, np.zeros((0, 3), np.int32), skip_isolated=True)
    c = eng.unitig_consensus(words, lens, u)
    assert u.n_pairs == 0 and c.n_pairs == 0 and c.info["pairs"] == 0 and c.to_host()["words"].shape == (0,)


# ---- (d) the full chain

def _nodes(n, length, G_, seed, err):
    codes, lens = gen_reads.sample_reads(n, length, G_, seed, err, None)
    rc = np.zeros_like(codes)
    for i in range(n):
        rc[i, : lens[i]] = 3 - codes[i, : lens[i]][::-1]
    codes = np.stack([rc, codes], axis=1).reshape(2 * n, length)
    lens = np.repeat(lens, 2)
    return alga_amd.pack_reads(codes, lens), lens.astype(np.int32)


def test_full_chain_from_reads_with_errors(eng):
    """build -> supplement -> cut -> parallel paths -> clip -> unitigs -> consensus on 3000 reads of 150 nt with 2 % substitutions"""
    n, length, err = 3000, 150, 0.02
    words, lens = _nodes(n, length, 9000, 77, err)
    w, l = _dev(eng, words, lens)
    d, m = eng.prefsuf_device(w, l, 82, 116)
    p = eng.pkb_params(float(lens[lens > 0].mean()), err, min(2 * length // 3, 60))
    d, m = eng.pkb_supplement_device(w, l, d, m, p)
    mopp = max(250, int(1.75 * length))
    d, m, _ = eng.cut_triangles_device(len(lens), d, m, mopp)
    bound = int(mopp * float(length) / np.float32(100))
    e1, _ = eng.remove_short_parallel_paths(len(lens), d, bound, n_edges=m)
    e2, tips = eng.remove_dangling_branches(len(lens), e1, bound)
    edges = e2.cpu().numpy()
    u = eng.unitigs(w, l, e2, skip_isolated=True)
    c = eng.unitig_consensus(w, l, u, min_votes=3, votes=True)
    uh, got = u.to_host(), c.to_host()
    assert_same(got, S.consensus_pileup(words, lens, U.unitigs(words, lens, edges, skip_isolated=True), 3))
    print("full chain:", u.info, c.info)
    assert got["info"]["changed"] > 0                                        # a kernel that copies the spelled sequence would not get here
    assert (got["words"] != uh["words"]).any()


# ---- (e) text output

def _gfa_want(uh, rows_from, sequences=True):
    v = S.consensus_rows(uh, rows_from) if rows_from is not None else uh
    P = v["n_pairs"]
    rows = U.padded_rows(v)
    words2 = np.zeros((2 * P, rows.shape[1]), dtype=np.uint32)
    words2[1::2] = rows
    return G.gfa_bytes(words2, np.repeat(v["len"], 2), v["edges"], twins=True, sequences=sequences)


@pytest.mark.parametrize("graph,chunk_mb", [("f1_cfg1.aftersimplifier.graph", 256), ("f4_varlen.aftercut.graph", 1), ("f2_err2.aftersimplifier.graph", 1)])
def test_fasta_and_gfa_text(eng, golden_dir, tmp_path, graph, chunk_mb):
    words, lens, edges = K.golden(golden_dir, graph)
    w, l = _dev(eng, words, lens)
    fa, gfa = str(tmp_path / "c.fasta"), str(tmp_path / "u.gfa")
    try:
        eng.set_option("gfa_chunk_mb", chunk_mb)
        for skip in (False, True):
            u = eng.unitigs(w, l, edges, skip_isolated=skip)
            uh = u.to_host()
            plain = eng.write_unitig_gfa(gfa, u)
            before = open(gfa, "rb").read()
            assert before == _gfa_want(uh, None)[0]
            for mv in (3, 1, 0):
                c = eng.unitig_consensus(w, l, u, min_votes=mv)
                ch = c.to_host()
                for min_length in (200, 100, 1, 0, 10 ** 6):
                    info = eng.write_consensus_fasta(fa, u, c, min_length=min_length)
                    text, records = S.fasta_bytes(uh, ch, min_length)
                    assert open(fa, "rb").read() == text
                    assert info["segments"] == records and info["bytes"] == len(text) and info["links"] == 0
                    if min_length == 10 ** 6:
                        assert text == b"" and os.path.getsize(fa) == 0     # an empty selection is an empty file
                    os.unlink(fa)
                info = eng.write_unitig_gfa(gfa, u, consensus=c)
                text, winfo = _gfa_want(uh, ch)
                assert open(gfa, "rb").read() == text
                for k in ("segments", "links", "links_merged", "bytes"):
                    assert info[k] == winfo[k], k
                again = eng.write_unitig_gfa(gfa, u)
                assert open(gfa, "rb").read() == before and again["bytes"] == plain["bytes"]    # without consensus= the file is what it was
                assert eng.write_unitig_gfa(gfa, u, sequences=False)["bytes"] == len(_gfa_want(uh, None, False)[0])
    finally:
        eng.set_option("gfa_chunk_mb", 256)


def test_fasta_records_straddle_chunks(eng, tmp_path):
    """1 MB chunks and more than 2 MB of records: chunk borders fall between records, the window starts are not word-aligned.  300 000 reads of
    100 nt over 3 Mb stand 10 deep: after the triangle cut nearly every column of a contig has two votes or more, and the windows of at least
    200 nt together hold most of the genome (the CPU oracle's build and cut with the checker: 7 390 records, 2 931 624 bytes)"""
    words, lens = _nodes(300000, 100, 3000000, 79, 0.0)
    w, l = _dev(eng, words, lens)
    d, m = eng.prefsuf_device(w, l, 55, 77)
    d, m, _ = eng.cut_triangles_device(len(lens), d, m, 250)
    u = eng.unitigs(w, l, d, n_edges=m, skip_isolated=True)
    c = eng.unitig_consensus(w, l, u, min_votes=1)
    uh, ch = u.to_host(), c.to_host()
    assert_same(ch, S.consensus_pileup(words, lens, uh, 1))
    assert len(set((ch["trim_left"][ch["len"] > 0] % 16).tolist())) > 4
    path = str(tmp_path / "c.fasta")
    try:
        eng.set_option("gfa_chunk_mb", 1)
        info = eng.write_consensus_fasta(path, u, c, min_length=200)
    finally:
        eng.set_option("gfa_chunk_mb", 256)
    text, records = S.fasta_bytes(uh, ch, 200)
    print("straddle:", u.n_pairs, "pairs,", records, "records,", len(text), "bytes", info)
    assert info["bytes"] > 2 << 20 and info["segments"] == records
    assert open(path, "rb").read() == text


# ---- (f) the reference's own contigs

@pytest.mark.parametrize("fixture,nt", [("f1_cfg1", 19974), ("f3_paired", 14947)])
def test_reference_contig(eng, golden_dir, tmp_path, fixture, nt):
    words, lens, edges = K.golden(golden_dir, fixture + ".aftersimplifier.graph")
    u = eng.unitigs(words, lens, edges, skip_isolated=True)
    c = eng.unitig_consensus(words, lens, u, min_votes=3)
    path = str(tmp_path / "c.fasta")
    info = eng.write_consensus_fasta(path, u, c)
    assert info["segments"] == 1
    head, seq, rest = open(path).read().split("\n")
    with gzip.open(os.path.join(golden_dir, fixture + ".contigs.fasta.gz"), "rt") as f:
        contig = "".join(f.read().split("\n")[1:])
    assert head == ">unitig_0_length=%d" % nt and rest == "" and len(contig) == nt
    assert seq == contig or seq == S.revcomp(contig)


def test_cli_writes_the_consensus(golden_dir, tmp_path):
    """f1 through the command line: build, cut, unitigs, consensus -- the FASTA is the reference's contig, --unitigs= beside it is unchanged"""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    fx = O.Fixture(golden_dir, "f1_cfg1")
    try:
        f1, _ = fx.inputs()
        out = {}
        for name, args in (("both", ["--unitigs=u.gfa", "--consensus=c.fasta"]), ("alone", ["--consensus=c.fasta", "--consensus_min_length=100", "--consensus_min_votes=3"]),
                           ("unitigs", ["--unitigs=u.gfa"]), ("too_long", ["--consensus=c.fasta", "--consensus_min_length=30000"])):
            wd = tmp_path / name
            wd.mkdir()
            r = subprocess.run([exe, "--file1=" + f1, "--output=o.fasta"] + args, cwd=str(wd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            assert ("Consensus written" in r.stderr) == (name != "unitigs")
            out[name] = {f: open(str(wd / f), "rb").read() for f in ("u.gfa", "c.fasta") if (wd / f).exists()}
    finally:
        fx.cleanup()
    with gzip.open(os.path.join(golden_dir, "f1_cfg1.contigs.fasta.gz"), "rt") as f:
        contig = "".join(f.read().split("\n")[1:])
    head, seq, rest = out["both"]["c.fasta"].decode().split("\n")
    assert head == ">unitig_0_length=19974" and rest == "" and (seq == contig or seq == S.revcomp(contig))
    assert out["alone"] == {"c.fasta": out["both"]["c.fasta"]}
    assert out["both"]["u.gfa"] == out["unitigs"]["u.gfa"] and list(out["unitigs"]) == ["u.gfa"]
    assert out["too_long"] == {"c.fasta": b""}


# ---- (g) refusals

def test_refusals_leave_the_previous_result(eng, golden_dir):
    words, lens, edges = K.golden(golden_dir, "f4_varlen.aftercut.graph")
    w, l = _dev(eng, words, lens)
    stale = eng.unitigs(w, l, K.golden(golden_dir, "f4_varlen.graph")[2])   # the same reads before the cut: 3 223 pairs against 3 124
    u = eng.unitigs(w, l, edges, skip_isolated=True)
    c = eng.unitig_consensus(w, l, u)
    snap = c.to_host()

    def refused(*a, **k):
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.unitig_consensus(*a, **k)
        assert ei.value.code == -1
        assert_same(c.to_host(), snap)                                       # nothing was written

    assert stale.n_pairs != u.n_pairs
    refused(w, l, stale)                                                     # not the last unitig result
    refused(w, l, u, min_votes=-1)
    refused(w[:-1], l[:-1], u)                                               # an odd node count
    refused(w[:-2], l[:-2], u)                                               # another node set
    short = l.clone()
    short[int(u.path_node[int(u.path_off[1]) - 1])] -= 1                     # the last node of pair 0 one base shorter: not the layout of u
    refused(w, short, u)
    assert_same(eng.unitig_consensus(w, l, u).to_host(), snap)
    # a consensus does not outlive its unitigs
    u2 = eng.unitigs(w, l, edges, skip_isolated=True)
    with pytest.raises(alga_amd.AlgaError):
        eng.write_consensus_fasta("/dev/null", u2, c)
    with pytest.raises(alga_amd.AlgaError):
        eng.write_unitig_gfa("/dev/null", u2, consensus=c)


# ---- (h) size

def test_ring_400k_with_small_grids(eng):
    """240 000 nodes, one unitig of 400 kb after the cut, and grids of 8 workgroups: every kernel strides, and one wave scans the 25 000 mask
    words of the pair from both ends (with min_votes 1000 to no avail)"""
    r = GC.reads_of("ring_400k")
    cut = GC.oracle_graphs("ring_400k")[1]
    assert len(r.lens) >= 1 << 17
    try:
        eng.set_option("consensus_max_blocks", 8)
        uh, c = equals_checker(eng, r.words, r.lens, cut, skips=(True,), min_votes=(3, 1000))
    finally:
        eng.set_option("consensus_max_blocks", 0)
    assert uh["n_pairs"] == 1 and uh["len"][0] > 399000
    uh2, c2 = equals_checker(eng, r.words, r.lens, cut, skips=(True,), min_votes=(3,))
    assert (c2["words"] == uh2["words"]).all()
