"""The unitig consensus without a GPU: the two Python statements of the definition (tests/consensus_checker.py) agree with each other, with
answers worked out by hand and with the genome the reads were drawn from; the checker's consensus of the reference's simplified graph IS
the reference's contig on the two fixtures where that graph is one path; the library exports the calls; the compiler's resource report
of the new kernels."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import consensus_cases as CC
import consensus_checker as S
import unitig_cases as K
import unitig_checker as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("words", "trim_left", "len", "changed", "votes")


def same(a, b, what=""):
    assert a["n_pairs"] == b["n_pairs"], what
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and (a[k] == b[k]).all(), (what, k)
    assert a["info"] == b["info"], what


def test_library_exports_the_calls_and_the_engine_has_the_methods():
    lib = alga_amd.load_library()
    for name in ("alga_unitig_consensus_device", "alga_write_consensus_fasta_device"):
        assert hasattr(lib, name) and name in alga_amd.engine.EXPORTS
    for name in ("unitig_consensus", "write_consensus_fasta"):
        assert callable(getattr(alga_amd.Engine, name))
    assert lib.alga_abi_version() == 7                                       # the addition is additive
    hdr = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    assert int(re.search(r"#define\s+ALGA_CONSENSUS_VOTES\s+(\d+)", hdr).group(1)) == alga_amd.engine.CONSENSUS_VOTES
    assert int(re.search(r"#define\s+ALGA_GFA_CONSENSUS\s+(\d+)", hdr).group(1)) == alga_amd.engine.GFA_CONSENSUS == 4
    # alga_consensus_info: 7 counts and 3 times; alga_consensus: an int (padded) and 5 pointers
    assert C.sizeof(alga_amd.engine.ConsensusInfo) == 8 * 10 and C.sizeof(alga_amd.engine.ConsensusC) == 8 * 6
    binary = open(alga_amd.library_path(), "rb").read()
    for k in (b"k_cons_check", b"k_cons_vote", b"k_cons_vote_wide", b"k_cons_window"):
        assert k in binary


def test_new_kernels_resources():
    """The compiler's resource report of consensus_kernels.hip: no VGPR spill and no scratch in any kernel, 8 waves per SIMD in all of them
    (k_cons_vote holds its 64 bit-sliced counters of 8 bits in 16 registers)."""
    src = os.path.join(ROOT, "alga_amd", "csrc", "consensus_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_consensus_resources_%d.o" % os.getpid())
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
        m = re.search(r"Function Name: \S*?(k_cons_[a-z_]+?)E[A-Z]", s)
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
    assert sorted(reps) == ["k_cons_check", "k_cons_vote", "k_cons_vote_wide", "k_cons_window"], sorted(reps)
    for name, rep in reps.items():
        assert int(rep["VGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, (name, rep)
        assert int(rep["Occupancy [waves/SIMD]"]) == 8, (name, rep)


def test_the_literal_form_on_a_case_worked_out_by_hand():
    """ACGTACGT, CGTTCG two bases on, TTCGAA two more: columns 0..9 = A C [GC] [TG] [ATT] [CTT] [GCC] [TGG] A A"""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    reads = [[code[x] for x in r] for r in ("ACGTACGT", "CGTTCG", "TTCGAA")]
    s, freqs, p, q = S.consensus_literal([(reads[0], 0), (reads[1], 2), (reads[2], 2)], thr=1)
    assert "".join("ACGT"[c] for c in s) == "ACCGTTCGAA"                      # the ties [GC] and [TG] go to the smaller code
    assert freqs == [1, 1, 1, 1, 2, 2, 2, 2, 1, 1]
    assert (p, q) == (4, 7)
    assert S.consensus_literal([(reads[0], 0), (reads[1], 2), (reads[2], 2)], thr=2)[2:] == (10, 9)      # nothing left: p > q
    assert S.consensus_literal([(reads[0], 0), (reads[1], 2), (reads[2], 2)], thr=0)[2:] == (0, 9)


def _both_forms(case, min_votes):
    u = U.unitigs(case.words, case.lens, case.edges)
    assert u["n_pairs"] == 1
    a = S.consensus_pileup(case.words, case.lens, u, min_votes)
    same(S.consensus_by_the_literal_form(case.words, case.lens, u, min_votes), a, "literal against pile-up")
    return u, a


@pytest.mark.parametrize("seed", range(8))
def test_literal_equals_pileup_on_random_paths(seed):
    """lengths 5 .. 40, steps 0 .. 3 (offsets 0 and 1 among them), 30 % substitutions (ties are common), both strands"""
    rng = np.random.default_rng(900 + seed)
    n = int(rng.integers(2, 60))
    pos = np.concatenate([[0], np.cumsum(rng.integers(0, 4, size=n - 1))])
    ln = rng.integers(5, 41, size=n)
    for k in range(1, n):
        ln[k] = max(ln[k], pos[k - 1] + ln[k - 1] - pos[k])
    genome = rng.integers(0, 4, size=int(pos[-1] + ln[-1]), dtype=np.uint8)
    reads = []
    for k in range(n):
        r = genome[pos[k]: pos[k] + ln[k]].copy()
        hit = rng.random(len(r)) < 0.3
        r[hit] = rng.integers(0, 4, size=int(hit.sum()))
        reads.append(r)
    case = CC.chain(reads, pos, (rng.random(n) < 0.5).astype(np.int8), genome)
    for mv in (0, 1, 3, 1000):
        u, a = _both_forms(case, mv)
        if mv == 0:
            assert a["trim_left"][0] == 0 and a["len"][0] == u["len"][0]
        if mv == 1000:
            assert a["len"][0] == 0 and a["trim_left"][0] == 0


def test_literal_equals_pileup_beyond_depth_255():
    case = CC.stack(31, 330, 320)                                            # depth 320 in the middle, 10 % substitutions
    u, a = _both_forms(case, 3)
    assert a["votes"].max() == 255                                           # the byte saturates, the vote did not:
    g = CC.oriented_genome(case, u)
    t, L = int(a["trim_left"][0]), int(a["len"][0])
    assert L > len(g) - 20 and (CC.columns(u, a["words"])[t: t + L] == g[t: t + L]).all() and a["changed"][0] > 0


def test_ties_go_to_the_smallest_code():
    for make in (CC.ties, CC.four_way_tie):
        case, want = make()
        u, a = _both_forms(case, 0)
        assert (CC.columns(u, a["words"]) == want).all()
        assert a["len"][0] == len(want)


def test_one_node_unitigs_vote_with_their_own_row():
    words, lens = K.nodes_of([K.R[0], K.R[3]])
    u = U.unitigs(words, lens, np.zeros((0, 3), np.int32))
    assert u["n_pairs"] == 2
    a = S.consensus_pileup(words, lens, u, 0)
    assert (a["words"] == u["words"]).all() and (a["changed"] == 0).all() and (a["len"] == u["len"]).all()
    assert (S.consensus_pileup(words, lens, u, 3)["len"] == 0).all()          # one vote per column


@pytest.mark.parametrize("seed,n,err,step", CC.GENOME_CASES)
def test_the_vote_restores_the_genome(seed, n, err, step):
    """stated from the genome alone: the window of the consensus is the genome there, the spelled sequence is not"""
    case = CC.genome_path(seed, n, err, step)
    u = U.unitigs(case.words, case.lens, case.edges)
    assert u["n_pairs"] == 1
    a = S.consensus_pileup(case.words, case.lens, u, 3)
    g = CC.oriented_genome(case, u)
    t, L = int(a["trim_left"][0]), int(a["len"][0])
    assert L > len(g) - 200
    assert (CC.columns(u, a["words"])[t: t + L] == g[t: t + L]).all()
    wrong = int((CC.columns(u, u["words"]) != g).sum())
    assert wrong > 0.5 * err * len(g) and a["changed"][0] >= wrong - 20       # all but a few columns at the very ends are corrected
    print("seed %d err %.2f step %d: %d nt, spelled sequence %d wrong, consensus window [%d, %d) 0 wrong" % (seed, err, step, len(g), wrong, t, t + L))


@pytest.mark.parametrize("fixture,nt", [("f1_cfg1", 19974), ("f3_paired", 14947)])
def test_reference_pin(golden_dir, fixture, nt):
    """the reference's own contig (tools/make_golden_contigs.py) == the checker's consensus of the one unitig of the reference's graph
    after its simplifier, trimmed at votes > 3, up to strand"""
    words, lens, edges = K.golden(golden_dir, fixture + ".aftersimplifier.graph")
    u = U.unitigs(words, lens, edges, skip_isolated=True)
    assert u["n_pairs"] == 1
    a = S.consensus_pileup(words, lens, u, 3)
    with gzip.open(os.path.join(golden_dir, fixture + ".contigs.fasta.gz"), "rt") as f:
        records = [r for r in f.read().split(">") if r]
    assert len(records) == 1
    contig = "".join(records[0].split("\n")[1:])
    mine = S.window(u, a, 0)
    assert len(contig) == nt == int(a["len"][0])
    assert mine == contig or mine == S.revcomp(contig)
    same(S.consensus_by_the_literal_form(words, lens, u, 3), a)
    text, n = S.fasta_bytes(u, a, 200)
    assert n == 1 and text == (">unitig_0_length=%d\n%s\n" % (nt, mine)).encode()
    assert S.fasta_bytes(u, a, nt + 1) == (b"", 0)
