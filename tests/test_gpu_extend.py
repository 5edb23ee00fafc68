"""Contigs extended through junctions that paired reads support, on the GPU (alga_extend_contigs_device): every array, the seam list and every
count equal to the Python definition (tests/extend_checker.py) on the hand-built contig graphs of tests/extend_cases.py -- window edges,
thresholds, mates, heads and tails of 1 .. 1100 entries, the shapes of L* --, on 20 seeded random contig graphs, with both forms of the list
ranking; the refusals of step 0, each leaving the contig result valid; the consensus and the final contig set of an extended result against
their checkers (a seam read shared with another pair among them); the f8_pbranch fixture from the reference's graph and through the command
line.  A path that holds a contig and its twin cannot occur (it would be its own twin, which needs a link V -> V^1, and that needs
last(V) == last(V)^1), so there is no case for it."""
import numpy as np
import pytest

import alga_amd
import consensus_checker as S
import extend_cases as XC
import extend_checker as X
import final_checker as F

pytestmark = pytest.mark.gpu
KEYS = ("words", "word_off", "len", "path_node", "path_pos", "path_off", "edges")
CONS_KEYS = ("words", "trim_left", "len", "changed")
FINAL_KEYS = ("verdict", "rank", "id", "new_reads", "trim_left", "begin", "len", "order")
COUNTS = ("candidates", "direct_links", "links", "joinable", "ambiguous", "cycles_cut", "pairs_in", "pairs_out", "head_max", "longest_nodes",
          "longest_bases", "total_bases")


@pytest.fixture(scope="module", params=["jumping", "ruling_set"])
def eng(request):
    e = alga_amd.Engine(0)
    e.set_option("unitig_ruling", 1 if request.param == "ruling_set" else 0)
    yield e
    e.close()


def _dev(eng, case):
    import torch
    dev = torch.device("cuda", eng.device)
    w = torch.from_numpy(np.ascontiguousarray(case["words"], dtype=np.uint32).view(np.int32)).to(dev)
    return w, torch.from_numpy(np.ascontiguousarray(case["lens"], dtype=np.int32)).to(dev), torch.from_numpy(case["pair_off"]).to(dev)


def host(x):
    got = x.to_host()
    got["seam_off"] = x.seams[0].cpu().numpy().copy().view(np.uint64)
    got["seam_entry"] = x.seams[1].cpu().numpy().copy()
    return got


def assert_same(got, want, what=""):
    assert got["n_pairs"] == want["n_pairs"], what
    for k in KEYS + ("seam_off", "seam_entry"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    for k in COUNTS:
        assert got["info"][k] == want["info"][k], (what, k, got["info"][k], want["info"][k])


def equals_checker(eng, case, what="", downstream=True):
    """device == definition for the extension, then for the consensus and the final set made from it -> (device, checker, contigs) as host copies"""
    w, l, po = _dev(eng, case)
    u = eng.contigs(w, l, case["edges"], 0)
    uh = u.to_host()
    want = X.extend(case["words"], case["lens"], case["pair_off"], uh, case["mcw"], case["mconn"], case["max_insert"])
    x = eng.extend_contigs(w, l, po, u, case["mcw"], case["mconn"], case["max_insert"])
    got = host(x)
    assert_same(got, want, what)
    assert got["info"]["head_passes"] == -(-want["info"]["head_max"] // XC.SLICE)
    if downstream:
        c = eng.unitig_consensus(w, l, x, min_votes=0)
        ch = c.to_host()
        cw = S.consensus_pileup(case["words"], case["lens"], want, 0)
        for k in CONS_KEYS:
            assert ch[k].dtype == cw[k].dtype and ch[k].shape == cw[k].shape and (ch[k] == cw[k]).all(), (what, "consensus", k)
        for percent in (95, 100):
            fin = eng.final_contigs(x, c, 0, percent, 0).to_host()
            fw = F.final_contigs(want, cw, 0, percent, 0)
            for k in FINAL_KEYS:
                assert fin[k].dtype == fw[k].dtype and fin[k].shape == fw[k].shape and (fin[k] == fw[k]).all(), (what, "final", percent, k)
        got["final"] = fin
    return got, want, uh


@pytest.mark.parametrize("name", sorted(XC.CASES))
def test_hand_built_cases(eng, name):
    case = XC.CASES[name]()
    got, want, uh = equals_checker(eng, case, name)
    for k, v in case["expect"].items():
        if v is not None:
            assert got["info"][k] == v, (name, k, got["info"])
    if got["info"]["links"] == 0:                                         # no link at all: the arrays equal the input
        for k in KEYS:
            assert (got[k] == uh[k]).all() and got[k].dtype == uh[k].dtype, (name, k)
    if "sizes" in case:
        assert got["info"]["head_max"] == case["sizes"][0] and got["info"]["head_passes"] == -(-case["sizes"][0] // XC.SLICE)
    print(name, got["info"])


@pytest.mark.parametrize("seed", range(20))
def test_random_contig_graphs(eng, seed):
    got, _, _ = equals_checker(eng, XC.random_case(seed), ("random", seed))
    print(seed, {k: got["info"][k] for k in COUNTS})


def test_shared_seam_read(eng):
    """X + Y joined, Z ends at the read that is now interior: Z, ranked later, has every read but that one new -- at 100 percent it is rejected"""
    case = XC.CASES["join"]()
    got, want, _ = equals_checker(eng, case, "join")
    fin = got["final"]                                                     # (percent = 100)
    counts = np.diff(got["path_off"].astype(np.int64))
    z = int(np.argmin(counts))
    assert counts[z] == 3 and fin["new_reads"][z] == 2 and fin["verdict"][z] == F.REJECTED
    assert fin["verdict"][1 - z] == F.ACCEPTED and fin["new_reads"][1 - z] == counts[1 - z]
    assert got["seam_entry"].tolist() == want["seam_entry"].tolist() and len(got["seam_entry"]) == 5


def test_no_pair_off_means_unpaired(eng):
    case = XC.CASES["join"]()
    w, l, _ = _dev(eng, case)
    u = eng.contigs(w, l, case["edges"], 0)
    uh = u.to_host()
    x = eng.extend_contigs(w, l, None, u, 0)
    got = host(x)
    want = X.extend(case["words"], case["lens"], None, uh, 0)
    assert_same(got, want, "no pair_off")
    assert got["info"]["head_max"] == want["info"]["head_max"] > 0
    for k in KEYS:
        assert (got[k] == uh[k]).all(), k
    counts = np.diff(uh["path_off"].astype(np.int64))
    assert x.info["candidates"] > 0 and x.info["links"] == 0 and sorted(counts.tolist()) == [3, 9, 9]
    assert got["seam_entry"].tolist() == [i for c in counts.tolist() for i in (0, c - 1)]


@pytest.mark.parametrize("what", ["value", "twin", "mate_range", "mate_back", "mcw", "mconn", "max_insert", "n", "not_contigs", "twice", "stale", "flags"])
def test_refusals(eng, what):
    """every refusal of step 0; the contig result stays the engine's current one: its consensus still runs"""
    import torch
    case = XC.CASES["join"]()
    w, l, po = _dev(eng, case)
    u = eng.contigs(w, l, case["edges"], 0)
    po_h = case["pair_off"].copy()
    args = dict(min_chain_weight=0, min_connections=5, max_insert=1000)
    ww, ll = w, l
    if what == "value":
        po_h[0] = po_h[1] = 3
    elif what == "twin":
        po_h[1] = 0
    elif what == "mate_range":
        po_h[-1] = po_h[-2] = 1
    elif what == "mate_back":
        po_h[2] = po_h[3] = 0
    elif what == "mcw":
        args["min_chain_weight"] = -1
    elif what == "mconn":
        args["min_connections"] = 0
    elif what == "max_insert":
        args["max_insert"] = -1
    elif what == "n":
        ww, ll, po_h = w[:-2], l[:-2], po_h[:-2]
        po_h[-2:] = 0; po_h[-4:-2] = 0
    elif what == "not_contigs":
        u = eng.unitigs(w, l, case["edges"])
    elif what == "twice":
        u = eng.extend_contigs(w, l, po, u, 0)
    elif what == "flags":
        import ctypes as C
        from alga_amd.engine import _Nodes, _ptr, UnitigsC, ExtendInfo
        nd = _Nodes(_ptr(w), int(w.shape[1]), _ptr(l), int(l.shape[0]), None, None)
        out, info = UnitigsC(), ExtendInfo()
        rc = eng._lib.alga_extend_contigs_device(eng._h, C.byref(nd), C.c_void_p(_ptr(po)), C.byref(u._c), 0, 5, 1000, 1, None, C.byref(out), C.byref(info))
        assert rc == -1
        eng.unitig_consensus(w, l, u, min_votes=0)
        return
    elif what == "stale":
        stale = u
        u = eng.contigs(w, l, case["edges"][:-1], 0)
        with pytest.raises(alga_amd.AlgaError):
            eng.extend_contigs(w, l, po, stale, 0)
        eng.unitig_consensus(w, l, u, min_votes=0)
        return
    before = {k: v.copy() for k, v in u.to_host().items() if k in KEYS}
    with pytest.raises(alga_amd.AlgaError):
        eng.extend_contigs(ww, ll, torch.from_numpy(po_h).to(w.device), u, **args)
    after = u.to_host()
    for k in KEYS:
        assert (after[k] == before[k]).all(), (what, k)
    eng.unitig_consensus(w, l, u, min_votes=0)                             # still the current result


def test_the_contig_result_is_replaced(eng):
    """after a successful call the contig result is no longer the engine's current one; the extended one goes through the GFA and the FASTA"""
    case = XC.CASES["three_chains_05"]()
    w, l, po = _dev(eng, case)
    u = eng.contigs(w, l, case["edges"], 0)
    x = eng.extend_contigs(w, l, po, u, 0)
    with pytest.raises(alga_amd.AlgaError):
        eng.unitig_consensus(w, l, u, min_votes=0)
    c = eng.unitig_consensus(w, l, x, min_votes=0)
    assert x.n_pairs == 3 and int(x.len.max()) == int(c.to_host()["len"].max())


def test_golden_pbranch_on_the_device(eng, golden_dir, tmp_path):
    """f8_pbranch from the reference's after-simplifier graph: contigs -> extension -> consensus -> final set on the device is the checker's
    result and the reference's paired o.fasta up to strand"""
    import test_extend_cpu as TC
    words, lens, pair_off, edges, mcw, min_len, mopp = TC.pbranch(golden_dir)
    case = dict(words=words, lens=lens, pair_off=pair_off)
    w, l, po = _dev(eng, case)
    u = eng.contigs(w, l, edges, mopp)
    want = X.extend(words, lens, pair_off, u.to_host(), mcw, 5, 1000)
    x = eng.extend_contigs(w, l, po, u, mcw)
    assert_same(host(x), want, "f8_pbranch")
    c = eng.unitig_consensus(w, l, x, min_votes=3)
    fin = eng.final_contigs(x, c, min_len, 95, 25)
    path = str(tmp_path / "f.fasta")
    assert eng.write_final_fasta(path, fin)["segments"] == 2
    assert TC.same_up_to_strand(open(path, "rb").read(), TC.reference_records(golden_dir, "f8_pbranch.contigs.fasta.gz"))
    print(x.info)


def test_cli_paired_extend(golden_dir, tmp_path):
    """f8_pbranch through the command line: with --paired_extend=1 the two records of the reference's paired run up to strand, without it
    (and with it but without --file2) the three of its single-file run"""
    import os
    import subprocess
    import oracle_lib as O
    import test_extend_cpu as TC
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    fx = O.Fixture(golden_dir, "f8_pbranch")
    out, err = {}, {}
    try:
        f1, f2 = fx.inputs()
        for name, args in (("extended", ["--file2=" + f2, "--paired_extend=1", "--contigs=c.fasta", "--contigs_gfa=c.gfa"]), ("plain", ["--file2=" + f2]),
                           ("off", ["--file2=" + f2, "--paired_extend=0"])):
            wd = tmp_path / name
            wd.mkdir()
            r = subprocess.run([exe, "--file1=" + f1, "--output=o.fasta", "--contigs_final=f.fasta"] + args, cwd=str(wd), stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            out[name], err[name] = open(str(wd / "f.fasta"), "rb").read(), r.stderr
        wd = tmp_path / "no_file2"
        wd.mkdir()
        r = subprocess.run([exe, "--file1=" + f1, "--output=o.fasta", "--contigs_final=f.fasta", "--paired_extend=1"], cwd=str(wd), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0 and "without --file2" in r.stderr and "Contigs extended" not in r.stderr, r.stderr[-2000:]
    finally:
        fx.cleanup()
    assert "Contigs extended by paired connections: 3 -> 2 contigs" in err["extended"] and "Contigs extended" not in err["plain"]
    assert TC.same_up_to_strand(out["extended"], TC.reference_records(golden_dir, "f8_pbranch.contigs.fasta.gz"))
    assert out["plain"] == out["off"] and TC.same_up_to_strand(out["plain"], TC.reference_records(golden_dir, "f8_pbranch.single.contigs.fasta.gz"))
    gfa = open(str(tmp_path / "extended" / "c.gfa")).read()
    assert sum(1 for line in gfa.split("\n") if line.startswith("S\t")) == 2
