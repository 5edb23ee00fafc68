"""The contigs without a GPU: the Python definition (tests/contig_checker.py) equals every hand-made case (tests/contig_cases.py), its results
are twin-symmetric and cover every final edge once, its triangle cut of H is the oracle's; on the reference's simplified graphs its windows are
the reference's contigs (f1, f3: the one contig; f4: a substring of the one contig; f2: one equal, one a prefix); the library exports the call;
the compiler's resource report of the new kernels."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import consensus_checker as S
import contig_cases as CC
import contig_checker as CT
import oracle_lib as O
import unitig_cases as K
import unitig_checker as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_golden = {}


def golden_contigs(golden_dir, graph, bound):
    """one checker run per dump, shared by the tests (read only)"""
    if graph not in _golden:
        words, lens, edges = K.golden(golden_dir, graph)
        u = CT.contigs(words, lens, edges, bound)
        _golden[graph] = (words, lens, edges, u, S.consensus_pileup(words, lens, u, 3))
    return _golden[graph]


def reference_records(golden_dir, fixture):
    with gzip.open(os.path.join(golden_dir, fixture + ".contigs.fasta.gz"), "rt") as f:
        recs = [r for r in f.read().split(">") if r]
    return {r.split("\n")[0]: "".join(r.split("\n")[1:]) for r in recs}


def test_library_exports_the_call_and_the_engine_has_the_method():
    lib = alga_amd.load_library()
    assert hasattr(lib, "alga_contigs_device") and "alga_contigs_device" in alga_amd.engine.EXPORTS
    assert callable(alga_amd.Engine.contigs)
    assert lib.alga_abi_version() == 7                                       # the call only adds to the ABI
    hdr = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    assert int(re.search(r"#define\s+ALGA_CONTIG_MAX_ROUNDS\s+(\d+)", hdr).group(1)) == alga_amd.engine.CONTIG_MAX_ROUNDS == CT.ROUNDS_KEPT
    # alga_contig_info: 3 counts, 4 x 64 per round, 9 counts, an int (padded), 6 times
    assert C.sizeof(alga_amd.engine.ContigInfo) == 8 * (3 + 4 * 64 + 9 + 1 + 6)
    binary = open(alga_amd.library_path(), "rb").read()
    for k in (b"k_ct_pflags", b"k_ct_chains", b"k_ct_groups", b"k_ct_cut_back", b"k_ct_edge_keep", b"k_ct_layout_ends", b"k_ct_join_fill"):
        assert k in binary


def test_new_kernels_resources():
    """The compiler's resource report of contig_kernels.hip: no VGPR spill and no scratch in any kernel"""
    src = os.path.join(ROOT, "alga_amd", "csrc", "contig_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_contig_resources_%d.o" % os.getpid())
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
        m = re.search(r"Function Name: \S*?(k_ct_[a-z_]+?)E[A-Z]", s)
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
    assert sorted(reps) == sorted(["k_ct_pflags", "k_ct_next", "k_ct_open_cycles", "k_ct_run_info", "k_ct_chains", "k_ct_open_keys", "k_ct_groups",
                                   "k_ct_cut_back", "k_ct_edge_keep", "k_ct_compact", "k_ct_winners", "k_ct_pair_sizes", "k_ct_layout_ends",
                                   "k_ct_layout_inner", "k_ct_join_count", "k_ct_join_fill", "k_ct_fasta_select"]), sorted(reps)
    for name, rep in reps.items():
        assert int(rep["VGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, (name, rep)


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_checker_equals_the_hand_made_case(name):
    words, lens, edges, mo = CC.inputs(name)
    CC.assert_equals_expected(CT.contigs(words, lens, edges, mo), name)


def assert_well_formed(u, lens):
    """twin-symmetric, every final edge in exactly one contig, the contig graph joins last nodes to first nodes"""
    B = u["final"]
    tw = np.stack([B[:, 1] ^ 1, B[:, 0] ^ 1, lens[B[:, 1]].astype(np.int64) - lens[B[:, 0]] + B[:, 2]], axis=1) if len(B) else B
    assert {tuple(x) for x in B.tolist()} == {tuple(x) for x in tw.tolist()}
    po = u["path_off"].astype(np.int64)
    used = []
    for k in range(u["n_pairs"]):
        nd, pp = u["path_node"][po[k]: po[k + 1]].tolist(), u["path_pos"][po[k]: po[k + 1]].tolist()
        fwd = [(nd[i], nd[i + 1], pp[i + 1] - pp[i]) for i in range(len(nd) - 1)]
        rev = [(b ^ 1, a ^ 1, int(lens[b]) - int(lens[a]) + o) for a, b, o in fwd]
        used += fwd if sorted(fwd) == sorted(rev) else fwd + rev           # a self-twin chain holds its twin edges itself
        assert u["len"][k] == pp[-1] + lens[nd[-1]]
    assert sorted(used) == sorted(tuple(x) for x in B.tolist())
    e = {tuple(x) for x in u["edges"].tolist()}
    assert len(e) == len(u["edges"])
    first = lambda X: int(u["path_node"][po[X >> 1]]) if X & 1 else int(u["path_node"][po[(X >> 1) + 1] - 1]) ^ 1
    last = lambda X: int(u["path_node"][po[(X >> 1) + 1] - 1]) if X & 1 else int(u["path_node"][po[X >> 1]]) ^ 1
    for x, y, o in e:
        assert last(x) == first(y) and int(u["len"][x >> 1]) - o == int(lens[last(x)])
        assert (y ^ 1, x ^ 1, int(u["len"][y >> 1]) - int(lens[last(x)])) in e


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_hand_made_results_are_well_formed(name):
    words, lens, edges, mo = CC.inputs(name)
    assert_well_formed(CT.contigs(words, lens, edges, mo), lens)


@pytest.mark.parametrize("graph,bound", [("f4_varlen.aftersimplifier.graph", 250), ("f2_err2.aftersimplifier.graph", 262), ("f5_messy.aftercut.graph", 250)])
def test_golden_results_are_well_formed(golden_dir, graph, bound):
    words, lens, edges, u, _ = golden_contigs(golden_dir, graph, bound)
    assert_well_formed(u, lens)


def test_the_checkers_cut_is_the_oracles(golden_dir):
    """cut_triangles of the checker against oracle_cut_triangles: on H of the first round of f4 / f5, and on whole graphs"""
    for graph in ("f4_varlen.graph", "f5_messy.graph", "f2_err2.graph"):
        words, lens, edges = K.golden(golden_dir, graph)
        star, _ = U.symmetrise(lens, edges)
        for bound in (250, 60):
            H = {(int(a), int(b)): int(o) for a, b, o in star}
            want = {(int(a), int(b)) for a, b, _ in O.cut_triangles(len(lens), star.astype(np.int32), bound)}
            assert CT.cut_triangles(H, bound) == want and len(want) < len(H)


@pytest.mark.parametrize("fixture,nt", [("f1_cfg1", 19974), ("f3_paired", 14947)])
def test_one_path_is_the_reference_contig(golden_dir, fixture, nt):
    words, lens, edges, u, c = golden_contigs(golden_dir, fixture + ".aftersimplifier.graph", 250)
    (head, contig), = reference_records(golden_dir, fixture).items()
    assert u["n_pairs"] == 1 and u["info"]["rounds"] == 1 and head == "contig_id=0_length=%d" % nt and len(contig) == nt
    win = S.window(u, c, 0)
    assert win == contig or win == S.revcomp(contig)


def test_f4_two_rounds_make_the_genome_long_contig(golden_dir):
    words, lens, edges, u, c = golden_contigs(golden_dir, "f4_varlen.aftersimplifier.graph", 250)
    info = u["info"]
    assert info["rounds"] == 2 and info["edges_sym"] == 2964 and info["final_edges"] == 2170
    counts = np.diff(u["path_off"].astype(np.int64))
    k = int(np.argmax(counts))
    assert counts[k] == 1077 == info["longest_nodes"] and u["len"][k] == 11932 == info["longest_bases"] and c["len"][k] == 11849
    assert int((c["len"] >= 200).sum()) == 1
    (contig,) = reference_records(golden_dir, "f4_varlen").values()
    win = S.window(u, c, k)
    assert len(contig) == 11875 and (win in contig or win in S.revcomp(contig))
    # the unitig path on the same graph: the longest window is 305 nt
    uu = U.unitigs(words, lens, edges, skip_isolated=True)
    assert int(S.consensus_pileup(words, lens, uu, 3)["len"].max()) == 305


def test_f2_nothing_to_remove(golden_dir):
    words, lens, edges, u, c = golden_contigs(golden_dir, "f2_err2.aftersimplifier.graph", 262)
    info = u["info"]
    assert info["rounds"] == 1 and info["base_edges_dropped"] == [0] and info["parallel_drops"] == [0] and info["groups_cut"] == [0] and u["n_pairs"] == 333
    ref = reference_records(golden_dir, "f2_err2")
    c0, c1 = ref["contig_id=0_length=361"], ref["contig_id=1_length=284"]
    wins = [S.window(u, c, k) for k in range(u["n_pairs"]) if c["len"][k] >= 200]
    both = lambda s: (s, S.revcomp(s))
    assert any(w in both(c1) for w in wins)
    assert any(len(w) == 318 and (c0.startswith(w) or c0.startswith(S.revcomp(w))) for w in wins)       # (a prefix up to strand)


def test_refusals():
    for name in K.REFUSALS:
        with pytest.raises(ValueError):
            CT.contigs(*K.refusal_nodes(name), 250)
    words, lens, edges, _ = CC.inputs("plain_chain")
    with pytest.raises(ValueError):
        CT.contigs(words, lens, edges, -1)
