"""The contigs on the GPU (alga_contigs_device): every array and every count equal to the Python definition (tests/contig_checker.py) on the
hand-made cases, the reference's graph dumps, the rings and dense graphs of tests/graph_cases.py, with both forms of the list ranking; a
chain of 2^16 + 3 nodes with a bubble; 240 000 nodes with small consensus grids; the consensus of a contig result; the FASTA against the
reference's own files; the f4 facts; the GFA of the contig graph; refusals; the cut's engine-owned output as input; unitigs afterwards."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import consensus_checker as S
import contig_cases as CC
import contig_checker as CT
import gfa_writer as G
import graph_cases as GC
import oracle_lib as O
import unitig_cases as K
import unitig_checker as U

pytestmark = pytest.mark.gpu
KEYS = ("words", "word_off", "len", "path_node", "path_pos", "path_off", "edges")
CONS_KEYS = ("words", "trim_left", "len", "changed")
DUMPS = ["f1_cfg1.aftercut.graph", "f1_cfg1.aftersimplifier.graph", "f2_err2.aftercut.graph", "f2_err2.aftersimplifier.graph",
         "f4_varlen.aftercut.graph", "f4_varlen.aftersimplifier.graph", "f5_messy.aftercut.graph", "f7_pkb.aftercut.graph"]


@pytest.fixture(scope="module", params=["jumping", "ruling_set"])
def eng(request):
    e = alga_amd.Engine(0)
    e.set_option("unitig_ruling", 1 if request.param == "ruling_set" else 0)
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
    for k, v in want["info"].items():
        assert got["info"][k] == v, (what, k, got["info"][k], v)


def equals_checker(eng, words, lens, edges, max_offset, consensus=True, what=""):
    """device == definition, and the consensus of the device's contigs == the pile-up on the checker's layout; -> (device, checker) as host copies"""
    w, l = _dev(eng, words, lens)
    want = CT.contigs(words, lens, edges, max_offset)
    u = eng.contigs(w, l, edges, max_offset)
    got = u.to_host()
    assert_same(got, want, what)
    if consensus:
        c = eng.unitig_consensus(w, l, u, min_votes=3).to_host()
        cw = S.consensus_pileup(words, lens, want, 3)
        for k in CONS_KEYS:
            assert c[k].dtype == cw[k].dtype and c[k].shape == cw[k].shape and (c[k] == cw[k]).all(), (what, "consensus", k)
        got["cons"] = c
    return got, want


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_hand_made_cases(eng, name):
    words, lens, edges, mo = CC.inputs(name)
    got, _ = equals_checker(eng, words, lens, edges, mo, what=name)
    CC.assert_equals_expected(got, name)


@pytest.mark.parametrize("graph", DUMPS)
def test_reference_dump(eng, golden_dir, graph):
    words, lens, edges = K.golden(golden_dir, graph)
    got, _ = equals_checker(eng, words, lens, edges, 262 if graph.startswith("f2") else 250, what=graph)
    print(graph, got["info"])


@pytest.mark.parametrize("name", ["ring_20k", "three_rings", "rings_and_linear", "ring_with_repeat"])
def test_rings(eng, name):
    r = GC.reads_of(name)
    for k, edges in enumerate(GC.oracle_graphs(name)):
        got, _ = equals_checker(eng, r.words, r.lens, edges, GC.MOPP, consensus=k == 1, what=name)
    # after the cut: a cycle of compactable edges is a cycle of path nodes and the other way round, so the unitig figures pinned on the CPU
    # hold here too (a ring with a repeat branches at the repeat: no cycle of path nodes, 0); every such cycle and its twin are closed chains
    cycles = GC.PINNED[name]["after_cut"]["cycles_cut"]
    assert got["info"]["cycles_cut"] == cycles and got["info"]["closed_chains"] >= 2 * cycles


@pytest.mark.parametrize("name", sorted(GC.DENSE))
def test_dense_graphs(eng, name):
    n, e, words, lens = GC.dense_case(name)
    for mo in GC.DENSE_MOPP:
        equals_checker(eng, words, lens, e, mo, consensus=False, what=(name, mo))
        equals_checker(eng, words, lens, GC.thinned(name), mo, consensus=mo == 7, what=(name, "thinned", mo))


def _long_chain(n_chain, bubble_at):
    """reads 0 .. n_chain - 1 in a chain (offset 10, 96 nt), and one more read beside read `bubble_at`: a heavier parallel chain"""
    n_reads = n_chain + 1
    lens = np.full(2 * n_reads, 96, dtype=np.int32)
    words = np.random.RandomState(5).randint(0, 1 << 32, size=(2 * n_reads, 6), dtype=np.uint64).astype(np.uint32)
    k = np.arange(n_chain - 1)
    e = np.stack([2 * k + 1, 2 * k + 3, np.full(len(k), 10)], axis=1)
    x = 2 * n_chain + 1
    extra = np.array([(2 * bubble_at - 1, x, 15), (x, 2 * bubble_at + 3, 15)])
    return words, lens, np.concatenate([e, extra]).astype(np.int32)


def test_long_chain_with_a_bubble(eng):
    """2^16 + 3 nodes a side: the ruling-set ranking and a second round both run at size; the result is the one chain"""
    n_chain = (1 << 16) + 3
    words, lens, edges = _long_chain(n_chain, n_chain // 2)
    got, _ = equals_checker(eng, words, lens, edges, 250, consensus=False)
    assert got["n_pairs"] == 1 and got["info"]["rounds"] == 2 and got["info"]["parallel_drops"] == [2, 0]
    assert got["info"]["longest_nodes"] == n_chain and got["path_node"].tolist() == list(range(1, 2 * n_chain, 2))


def test_ring_400k_with_small_grids(eng):
    """240 000 nodes, one closed chain of 400 kb after the cut; the consensus of the contig result with grids of 8 workgroups"""
    r = GC.reads_of("ring_400k")
    cut = GC.oracle_graphs("ring_400k")[1]
    assert len(r.lens) >= 1 << 17
    try:
        eng.set_option("consensus_max_blocks", 8)
        got, _ = equals_checker(eng, r.words, r.lens, cut, GC.MOPP)
    finally:
        eng.set_option("consensus_max_blocks", 0)
    assert got["n_pairs"] == 1 and got["len"][0] > 399000 and got["info"]["closed_chains"] == 2


def _reference_records(golden_dir, fixture):
    with gzip.open(os.path.join(golden_dir, fixture + ".contigs.fasta.gz"), "rt") as f:
        recs = [r for r in f.read().split(">") if r]
    return [(">" + r.split("\n")[0], "".join(r.split("\n")[1:])) for r in recs]


@pytest.mark.parametrize("fixture", ["f1_cfg1", "f3_paired"])
def test_fasta_is_the_reference_file(eng, golden_dir, tmp_path, fixture):
    words, lens, edges = K.golden(golden_dir, fixture + ".aftersimplifier.graph")
    u = eng.contigs(words, lens, edges, 250)
    c = eng.unitig_consensus(words, lens, u, min_votes=3)
    path = str(tmp_path / "c.fasta")
    info = eng.write_consensus_fasta(path, u, c)
    (ref_head, ref_seq), = _reference_records(golden_dir, fixture)
    head, seq, rest = open(path).read().split("\n")
    assert info["segments"] == 1 and rest == ""
    assert head == ref_head and (seq == ref_seq or seq == S.revcomp(ref_seq))


def test_f4_facts(eng, golden_dir, tmp_path):
    words, lens, edges = K.golden(golden_dir, "f4_varlen.aftersimplifier.graph")
    u = eng.contigs(words, lens, edges, 250)
    assert u.info["rounds"] == 2 and u.info["edges_sym"] == 2964 and u.info["final_edges"] == 2170
    c = eng.unitig_consensus(words, lens, u, min_votes=3)
    uh, ch = u.to_host(), c.to_host()
    k = int(np.argmax(np.diff(uh["path_off"].astype(np.int64))))
    assert int(np.diff(uh["path_off"].astype(np.int64))[k]) == 1077 and uh["len"][k] == 11932 and ch["len"][k] == 11849
    assert int((ch["len"] >= 200).sum()) == 1
    (_, ref), = _reference_records(golden_dir, "f4_varlen")
    win = S.window(uh, ch, k)
    assert win in ref or win in S.revcomp(ref)
    # the records are numbered as they are written: pair k is not pair 0, its record is contig_id=0
    path = str(tmp_path / "c.fasta")
    info = eng.write_consensus_fasta(path, u, c, min_length=200)
    assert k > 0 and info["segments"] == 1
    assert open(path).read() == ">contig_id=0_length=11849\n%s\n" % win
    info = eng.write_consensus_fasta(path, u, c, min_length=50)              # the windows: 84 nt (pair 5) and 11 849 nt (pair 6), the rest empty
    heads = [x for x in open(path).read().split("\n") if x.startswith(">")]
    kept = [int(L) for L in ch["len"] if L >= 50]
    assert kept == [84, 11849] and heads == [">contig_id=%d_length=%d" % (j, L) for j, L in enumerate(kept)] and info["segments"] == 2


def test_gfa_of_the_contig_graph(eng, golden_dir, tmp_path):
    words, lens, edges = K.golden(golden_dir, "f2_err2.aftersimplifier.graph")
    u = eng.contigs(words, lens, edges, 262)
    uh = u.to_host()
    path = str(tmp_path / "c.gfa")
    info = eng.write_unitig_gfa(path, u)
    text = open(path, "rb").read()
    P = uh["n_pairs"]
    rows = U.padded_rows(uh)
    words2 = np.zeros((2 * P, rows.shape[1]), dtype=np.uint32)
    words2[1::2] = rows
    want, winfo = G.gfa_bytes(words2, np.repeat(uh["len"], 2), uh["edges"], twins=True, sequences=True)
    assert text == want and info["segments"] == winfo["segments"] == P and info["links"] == winfo["links"]
    assert G.expand_links(text, np.repeat(uh["len"], 2)) == {tuple(x) for x in uh["edges"].tolist()}
    # the overlap of a link is the junction read's length
    last = uh["path_node"][uh["path_off"][1:].astype(np.int64) - 1]
    overlaps = {int(line.split(b"\t")[5][:-1]) for line in text.split(b"\n") if line.startswith(b"L")}
    assert len(uh["edges"]) > 0 and overlaps <= {int(x) for x in lens[last]} | {int(x) for x in lens[uh["path_node"][uh["path_off"][:-1].astype(np.int64)]]}
    for x, y, o in uh["edges"].tolist():
        k = x >> 1
        junction = uh["path_node"][int(uh["path_off"][k + 1]) - 1] if x & 1 else uh["path_node"][int(uh["path_off"][k])] ^ 1
        assert int(uh["len"][k]) - o == int(lens[junction])


def test_refusals_leave_the_previous_result(eng, golden_dir, tmp_path):
    words, lens, edges = K.golden(golden_dir, "f4_varlen.aftersimplifier.graph")
    w, l = _dev(eng, words, lens)
    u = eng.contigs(w, l, edges, 250)
    snap = u.to_host()
    c = eng.unitig_consensus(w, l, u)
    csnap = c.to_host()

    def refused(*a):
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.contigs(*a)
        assert ei.value.code == -1
        assert_same(u.to_host(), snap)
        assert (c.to_host()["words"] == csnap["words"]).all()
        assert eng.write_consensus_fasta(str(tmp_path / "c.fasta"), u, c)["segments"] == 1      # still the engine's current result

    refused(w, l, edges, -1)
    for name in K.REFUSALS:
        refused(*K.refusal_nodes(name), 250)
    bad = edges.copy()
    bad[5, 1] = len(lens)
    refused(w, l, bad, 250)


def test_the_cuts_own_output_as_input(eng, golden_dir):
    """d_edges is the triangle cut's engine-owned buffer: the call reads it before its own cut of H runs, and the cut's result stays valid"""
    words, lens, edges = K.golden(golden_dir, "f4_varlen.graph")
    w, l = _dev(eng, words, lens)
    import torch
    d = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int32)).to(w.device)
    dc, mc, _ = eng.cut_triangles_device(len(lens), d.data_ptr(), len(edges), 250)
    cut = alga_amd.engine.device_view(dc, (mc, 3), "cuda:%d" % eng.device).cpu().numpy().copy()
    u = eng.contigs(w, l, dc, 250, n_edges=mc)
    assert_same(u.to_host(), CT.contigs(words, lens, cut, 250))
    assert u.info["rounds"] >= 2
    assert (alga_amd.engine.device_view(dc, (mc, 3), "cuda:%d" % eng.device).cpu().numpy() == cut).all()


def test_unitigs_afterwards_write_what_they_wrote_before(eng, golden_dir, tmp_path):
    words, lens, edges = K.golden(golden_dir, "f4_varlen.aftersimplifier.graph")
    w, l = _dev(eng, words, lens)
    fa, gfa = str(tmp_path / "u.fasta"), str(tmp_path / "u.gfa")

    def unitig_files():
        u = eng.unitigs(w, l, edges, skip_isolated=True)
        c = eng.unitig_consensus(w, l, u, min_votes=3)
        eng.write_consensus_fasta(fa, u, c, min_length=100)
        eng.write_unitig_gfa(gfa, u)
        return open(fa, "rb").read(), open(gfa, "rb").read(), u.to_host(), c.to_host()

    before = unitig_files()
    u = eng.contigs(w, l, edges, 250)
    eng.write_consensus_fasta(fa, u, eng.unitig_consensus(w, l, u), min_length=100)
    assert open(fa, "rb").read().startswith(b">contig_id=0_length=")
    after = unitig_files()
    assert before[0] == after[0] and before[1] == after[1] and before[0].startswith(b">unitig_")
    assert before[0] == S.fasta_bytes(before[2], before[3], 100)[0]


def test_cli_writes_the_contigs(golden_dir, tmp_path):
    """f1 through the command line: build, cut, contigs, consensus -- the FASTA is the reference's file up to strand; without --contigs= nothing of it"""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    fx = O.Fixture(golden_dir, "f1_cfg1")
    try:
        f1, _ = fx.inputs()
        out = {}
        for name, args in (("contigs", ["--contigs=c.fasta", "--contigs_gfa=c.gfa", "--parallel_paths=1", "--clip_tips=1"]),
                           ("too_long", ["--contigs=c.fasta", "--contigs_min_length=30000"]), ("plain", [])):
            wd = tmp_path / name
            wd.mkdir()
            r = subprocess.run([exe, "--file1=" + f1, "--output=o.fasta"] + args, cwd=str(wd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            assert ("Contigs written" in r.stderr) == (name != "plain")
            out[name] = {f: open(str(wd / f), "rb").read() for f in ("c.fasta", "c.gfa") if (wd / f).exists()}
    finally:
        fx.cleanup()
    (ref_head, ref_seq), = _reference_records(golden_dir, "f1_cfg1")
    head, seq, rest = out["contigs"]["c.fasta"].decode().split("\n")
    assert head == ref_head and rest == "" and (seq == ref_seq or seq == S.revcomp(ref_seq))
    assert out["contigs"]["c.gfa"].startswith(b"H\tVN:Z:1.0\nS\t0\t")
    assert out["too_long"] == {"c.fasta": b""} and out["plain"] == {}
