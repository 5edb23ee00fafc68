"""The extension of contigs by paired connections, without a GPU: the Python definition (tests/extend_checker.py) on the hand-built contig
graphs of tests/extend_cases.py -- every case pins what it is about --, properties of every result (twin symmetry, seams, a layout the
consensus accepts), the refusals, the reference's own contigs of the f8_pbranch fixture with and without pairs, and the compiler's resource
report of the new kernels."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import consensus_checker as S
import contig_checker as CT
import extend_cases as XC
import extend_checker as X
import final_checker as F
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_ex_check", "k_ex_weights", "k_ex_count", "k_ex_outlinks", "k_ex_next", "k_ex_save", "k_ex_winners", "k_ex_pair_sizes", "k_ex_ids", "k_ex_layout",
           "k_ex_join_count", "k_ex_join_fill"]


def run(case):
    u = CT.contigs(case["words"], case["lens"], case["edges"], 0)
    return u, X.extend(case["words"], case["lens"], case["pair_off"], u, case["mcw"], case["mconn"], case["max_insert"])


def check_properties(case, u, x):
    lens = case["lens"].astype(np.int64)
    po, so = x["path_off"].astype(np.int64), x["seam_off"].astype(np.int64)
    upo = u["path_off"].astype(np.int64)
    assert x["info"]["pairs_in"] == u["n_pairs"] and x["info"]["pairs_out"] == x["n_pairs"]
    # every entry of u is an entry of x, once per seam it is shared at
    assert po[-1] == upo[-1] - (u["n_pairs"] - x["n_pairs"])
    assert so[-1] == x["n_pairs"] + u["n_pairs"]
    for k in range(x["n_pairs"]):
        nd, ps = x["path_node"][po[k]: po[k + 1]], x["path_pos"][po[k]: po[k + 1]].astype(np.int64)
        se = x["seam_entry"][so[k]: so[k + 1]]
        assert se[0] == 0 and se[-1] == len(nd) - 1 and (np.diff(se) > 0).all()
        assert ps[0] == 0 and (np.diff(ps) >= 0).all() and ps[-1] + lens[nd[-1]] == x["len"][k]
        assert (ps[1:] < ps[:-1] + lens[nd[:-1]]).all() and (ps[1:] + lens[nd[1:]] >= ps[:-1] + lens[nd[:-1]]).all(), "dovetails"
    e = {tuple(r) for r in x["edges"].tolist()}
    L = x["len"].astype(np.int64)
    for a, b, o in e:                                                      # twin symmetry of the graph
        la = lens[x["path_node"][po[a >> 1]]] if not a & 1 else lens[x["path_node"][po[(a >> 1) + 1] - 1]]
        assert o == L[a >> 1] - la
        assert any((b ^ 1, a ^ 1) == (p, q) for p, q, _ in e)
    S.consensus_pileup(case["words"], case["lens"], x, 3)                 # the layout covers every column


@pytest.mark.parametrize("name", sorted(XC.CASES))
def test_case(name):
    case = XC.CASES[name]()
    u, x = run(case)
    for k, v in case["expect"].items():
        if v is not None:
            assert x["info"][k] == v, (name, k, x["info"])
    check_properties(case, u, x)
    if x["info"]["links"] == 0:
        for k in ("words", "word_off", "len", "path_node", "path_pos", "path_off", "edges"):
            assert (x[k] == u[k]).all() and x[k].dtype == u[k].dtype, k


@pytest.mark.parametrize("name", XC.SIZE_CASES)
def test_sizes_are_what_the_names_say(name):
    """the head of Y and the tail of X have exactly the sizes the case was built for, and every pair is needed for the link"""
    case = XC.CASES[name]()
    k_head, k_tail = case["sizes"]
    if name.startswith(("head_", "tail_")) and name.split("_")[1].isdigit():
        assert int(name.split("_")[1]) == (k_head if name.startswith("head") else k_tail)
    u = CT.contigs(case["words"], case["lens"], case["edges"], 0)
    ent, _ = X.oriented(u, case["lens"])
    (ex, px), = [e for e in ent if e[0] == case["X"]]
    (ey, py), = [e for e in ent if e[0] == case["Y"]]
    assert len(X.tail_entries(ex, px, case["max_insert"])) == k_tail
    assert sum(1 for i in range(1, len(ey)) if py[i - 1] <= case["max_insert"]) == k_head == len(X.head_reads(ey, py, case["max_insert"]))
    x = X.extend(case["words"], case["lens"], case["pair_off"], u, case["mcw"], case["mconn"], case["max_insert"])
    assert x["info"]["head_max"] == k_head and x["info"]["joinable"] == 2
    more = X.extend(case["words"], case["lens"], case["pair_off"], u, case["mcw"], case["mconn"] + 1, case["max_insert"])
    assert more["info"]["direct_links"] == 0                              # one connection fewer than asked for: no link


def test_slice_is_the_engine_constant():
    import alga_amd.engine as E
    assert XC.SLICE == E.EXTEND_HEAD_SLICE
    hdr = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    assert re.search(r"#define ALGA_EXTEND_HEAD_SLICE (\d+)", hdr).group(1) == str(XC.SLICE)


def test_random_cases_have_links_of_every_kind():
    tot = dict(direct_links=0, joinable=0, ambiguous=0, cycles_cut=0)
    for seed in range(20):
        case = XC.random_case(seed)
        assert len(case["lens"]) <= 2000
        u, x = run(case)
        check_properties(case, u, x)
        for k in tot:
            tot[k] += x["info"][k]
    print(tot)
    assert tot["direct_links"] > 0 and tot["joinable"] > 0


def test_shared_seam_read_in_the_filter():
    """X + Y joined, Z ends at the read that is now interior: ranked later, Z has all its reads but that one new"""
    case = XC.CASES["join"]()
    u, x = run(case)
    cons = S.consensus_pileup(case["words"], case["lens"], x, 0)
    v = X.final_verdicts(x, cons["len"], 0, 95)
    counts = np.diff(x["path_off"].astype(np.int64))
    later = int(np.argmax(v["rank"]))
    assert v["new_reads"][later] == counts[later] - 1 and counts[later] == 3


@pytest.mark.parametrize("what", ["value", "twin", "mate_range", "mate_back", "mcw", "mconn", "max_insert"])
def test_refusals(what):
    case = XC.CASES["join"]()
    u = CT.contigs(case["words"], case["lens"], case["edges"], 0)
    po = case["pair_off"].copy()
    kw = dict(min_chain_weight=0, min_connections=5, max_insert=1000)
    if what == "value":
        po[0] = po[1] = 3
    elif what == "twin":
        po[1] = 0
    elif what == "mate_range":
        po[-1] = po[-2] = 1
    elif what == "mate_back":
        po[2] = po[3] = 0
    elif what == "mcw":
        kw["min_chain_weight"] = -1
    elif what == "mconn":
        kw["min_connections"] = 0
    else:
        kw["max_insert"] = -1
    with pytest.raises(ValueError):
        X.extend(case["words"], case["lens"], po, u, **kw)


def test_new_kernels_resources():
    """The compiler's resource report of extend_kernels.hip: no VGPR spill and no scratch in any kernel; k_ex_count keeps 32 KB of LDS a block
    (four tables of 2048 read indices)"""
    src = os.path.join(ROOT, "alga_amd", "csrc", "extend_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_extend_resources_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    finally:
        if os.path.exists(out):
            os.remove(out)
    lines = r.stderr.splitlines()
    reps = {}
    for i, s in enumerate(lines):
        m = re.search(r"Function Name: \S*?(k_ex_[a-z_]+?)E[A-Z]", s)
        if not m:
            continue
        rep = {}
        for t in lines[i + 1:]:
            if "Function Name:" in t:
                break
            mm = re.search(r"remark:\s+(.+?):\s+(\S+)\s+\[-Rpass", t)
            if mm:
                rep[mm.group(1)] = mm.group(2)
        reps[m.group(1)] = rep
    assert sorted(reps) == sorted(KERNELS), sorted(reps)
    for name, rep in reps.items():
        print(name, rep)
        assert int(rep["VGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, (name, rep)
    assert int(reps["k_ex_count"]["LDS Size [bytes/block]"]) == 4 * 2048 * 4


def pbranch(golden_dir):
    """the f8_pbranch fixture -> (words, lens, pair_off, edges of the reference's after-simplifier graph, min_chain_weight, min_length)"""
    fx = O.Fixture(golden_dir, "f8_pbranch")
    try:
        f1, f2 = fx.inputs()
        nd = O.ingest(f1, f2)
    finally:
        fx.cleanup()
    with gzip.open(os.path.join(golden_dir, "f8_pbranch.aftersimplifier.graph.gz"), "rb") as f:
        n, edges = O.parse_graph(f.read())
    assert n == len(nd["len"])
    live = np.zeros(n, dtype=bool)
    live[edges[:, 0]] = True
    live[edges[:, 1]] = True
    live &= nd["len"] > 0
    mcw = int(2 * nd["len"][live].astype(np.float64).mean())               # ContigCreatorSinglePath.cpp:274
    return nd["words"], nd["len"], nd["pair_off"], edges, mcw, max(200, int(1.75 * nd["LEN"])), max(250, int(1.75 * nd["LEN"]))


def reference_records(golden_dir, name):
    with gzip.open(os.path.join(golden_dir, name), "rt") as f:
        recs = [x for x in f.read().split(">") if x]
    return [(">" + x.split("\n")[0], "".join(x.split("\n")[1:])) for x in recs]


def same_up_to_strand(text, ref):
    got = [x for x in text.decode().split("\n") if x]
    heads, seqs = got[0::2], got[1::2]
    return heads == [h for h, _ in ref] and all(s == r or s == S.revcomp(r) for s, (_, r) in zip(seqs, ref))


def test_golden_pbranch(golden_dir):
    """the reference's after-simplifier graph through contigs -> extension -> consensus -> final set: the two records of the reference's paired
    run up to strand; without the extension the three records of its single-file run"""
    words, lens, pair_off, edges, mcw, min_len, mopp = pbranch(golden_dir)
    print("min_chain_weight", mcw, "min_length", min_len, "max_offset", mopp)
    u = CT.contigs(words, lens, edges, mopp)
    out = {}
    for name, res in (("single", u), ("paired", X.extend(words, lens, pair_off, u, mcw, 5, 1000))):
        cons = S.consensus_pileup(words, lens, res, 3)
        fin = F.final_contigs(res, cons, min_len, 95, 25)
        out[name] = F.fasta_bytes(res, cons, fin)
        if name == "paired":
            print(res["info"])
            assert res["info"]["direct_links"] == 1 and res["info"]["joinable"] == 2 and res["n_pairs"] == u["n_pairs"] - 1
    ref_p = reference_records(golden_dir, "f8_pbranch.contigs.fasta.gz")
    ref_s = reference_records(golden_dir, "f8_pbranch.single.contigs.fasta.gz")
    assert [len(s) for _, s in ref_p] == [19946, 3075] and [len(s) for _, s in ref_s] == [10081, 9876, 3075]
    assert out["paired"][1] == 2 and same_up_to_strand(out["paired"][0], ref_p)
    assert out["single"][1] == 3 and same_up_to_strand(out["single"][0], ref_s)
