"""The scaffolds without a GPU: the two Python statements of the definition (tests/scaffold_checker.py) agree on the cases of
tests/scaffold_cases.py, the outcomes the cases were made for, the planted genome; the refusals of the checker; the library exports the
calls and the header declares them; the compiler's resource report of scaffold_kernels.hip and chain_kernels.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import place_cases as PC
import place_checker as P
import scaffold_cases as QC
import scaffold_checker as SC
import scaffold_invariants as INV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_sc_check", "k_sc_links", "k_sc_heads", "k_sc_bundle_fill", "k_sc_bundles", "k_sc_second", "k_sc_choice", "k_sc_joins", "k_sc_cycle_drop",
           "k_sc_rank_init", "k_sc_place", "k_sc_layout", "k_sc_fasta_sizes", "k_sc_fasta_write",
           "k_ch_cycle_init", "k_ch_cycle_jump", "k_ch_rank_jump"]   # (chain_kernels.hip: the jumps the scaffolder, the merge and the stitch stage share)
SYMBOLS = ("alga_scaffold_default_params", "alga_scaffold_placed_device", "alga_write_scaffold_fasta_device")
# (links, bundles_supported, ends_ambiguous, joins, joins_dropped_cycle, scaffolds, scaffolds_multi) of every variant of every case
OUTCOMES = {"two": [(5, 1, 0, 1, 0, 1, 1), (5, 0, 0, 0, 0, 2, 0), (5, 1, 0, 1, 0, 1, 1)],
            "orient": [(30, 5, 0, 5, 0, 1, 1)] * 2,
            "ambiguous": [(29, 4, 1, 1, 0, 5, 1), (29, 4, 2, 0, 0, 6, 0), (29, 4, 0, 2, 0, 4, 2), (29, 3, 1, 1, 0, 5, 1)],
            "tie": [(23, 4, 1, 1, 0, 5, 1), (23, 3, 1, 1, 0, 5, 1), (23, 0, 0, 0, 0, 6, 0), (23, 4, 2, 0, 0, 6, 0)],
            "mutual": [(17, 2, 0, 1, 0, 2, 1)], "ring3": [(26, 4, 0, 3, 1, 2, 2)], "ring2": [(15, 2, 0, 1, 1, 2, 1)],
            "too_far": [(8, 2, 0, 2, 0, 1, 1), (11, 2, 0, 2, 0, 1, 1), (6, 1, 0, 1, 0, 2, 1)],
            "neg_gap": [(11, 2, 0, 2, 0, 1, 1)] * 4, "long_chain": [(1495, 299, 0, 299, 0, 1, 1)],
            "big_bundle": [(3024, 1, 0, 1, 0, 25, 1), (3024, 25, 7, 7, 0, 19, 7)],
            "seams": [(30, 6, 0, 6, 0, 4, 2)] * 3, "no_pairs": [(0, 0, 0, 0, 0, 2, 0)], "one_target": [(0, 0, 0, 0, 0, 2, 0)], "n0": [(0, 0, 0, 0, 0, 2, 0)],
            "t0": [(0, 0, 0, 0, 0, 0, 0)]}


def assert_same(got, want, what=""):
    for k in SC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    assert got["info"] == want["info"], (what, got["info"], want["info"])


layout = INV.layout                                                            # the scaffolds as [[(contig, orient)]]


@pytest.mark.parametrize("name,i", QC.every())
def test_the_two_statements_agree(name, i):
    c, pl, want = QC.case(name), QC.placed(name), QC.checked(name, i)
    v = c["variants"][i]
    got = SC.scaffold_walk(*QC.scaffold_args(c, pl), **v)
    assert_same(got, want, (name, i))
    info = want["info"]
    assert tuple(info[k] for k in ("links", "bundles_supported", "ends_ambiguous", "joins", "joins_dropped_cycle", "scaffolds", "scaffolds_multi")) == OUTCOMES[name][i], info
    INV.every_result(c, pl["info"]["pairs_split"], want, v)                   # what holds for every result (tests/scaffold_invariants.py)
    print(name, i, info)


def test_every_case_is_listed():
    assert sorted(OUTCOMES) == sorted(QC.CASES) and all(len(OUTCOMES[n]) == len(QC.case(n)["variants"]) for n in QC.CASES)
    for need in ("two", "orient", "ambiguous", "tie", "mutual", "ring3", "ring2", "too_far", "neg_gap", "long_chain", "big_bundle", "seams", "no_pairs", "n0", "t0", "one_target"):
        assert need in QC.CASES


def test_outcomes_the_cases_were_made_for():
    w = QC.checked("two")
    assert w["b_links"].tolist() == [5] and w["b_state"].tolist() == [SC.B_SUPPORTED | SC.B_JOIN] and layout(w) == [[(0, 0), (1, 0)]]
    assert QC.checked("two", 1)["b_state"].tolist() == [0] and layout(QC.checked("two", 1)) == [[(0, 0)], [(1, 0)]]
    # all four combinations of ends in one chain; a `-` contig is written reverse-complemented
    c, w = QC.case("orient"), QC.checked("orient")
    assert layout(w) == [QC.ORIENT_CHAIN]
    ends = sorted((int(a) & 1, int(b) & 1) for a, b in zip(w["b_a"], w["b_b"]))
    assert set(ends) == {(0, 0), (0, 1), (1, 0), (1, 1)}                           # L-L, L-R, R-L, R-R, the end of the smaller contig first
    seq = SC.fasta(w, c["seqs"]).decode().split("\n")[1]
    at = int(w["start"][2])
    assert seq[at:at + 121] == "".join("ACGT"[x] for x in P.revcomp(c["seqs"][2])) and seq[:150] == "".join("ACGT"[x] for x in c["seqs"][0])
    assert seq[150:150 + int(w["gap_after"][0])] == "N" * int(w["gap_after"][0]) and w["gap_after"][5] == 0 and w["join_links"].tolist() == [6, 6, 6, 6, 6, 0]
    # 10 against 5 is ambiguous at 50 %, 10 against 4 is not
    w = QC.checked("ambiguous")
    assert w["b_links"].tolist() == [10, 5, 10, 4] and w["end_state"][1] == SC.E_HAS_SUPPORTED | SC.E_AMBIGUOUS and w["end_state"][7] == SC.E_HAS_SUPPORTED | SC.E_JOINED
    assert layout(w) == [[(0, 0)], [(1, 0)], [(2, 0)], [(3, 0), (4, 0)], [(5, 0)]] and w["b_state"].tolist() == [1, 1, 3, 1]
    assert QC.checked("ambiguous", 2)["end_state"][1] == SC.E_HAS_SUPPORTED | SC.E_JOINED              # 51 %: 5 of 10 is no rival any more
    # equal n: ambiguous at any percentage; 5 against 6 at 100 % is not; with min_links 6 the 5 is unsupported; with 7 nothing is supported
    w = QC.checked("tie")
    assert w["b_links"].tolist() == [6, 6, 6, 5] and w["end_state"][1] & SC.E_AMBIGUOUS and not w["end_state"][7] & SC.E_AMBIGUOUS and layout(w)[3] == [(3, 0), (4, 0)]
    assert QC.checked("tie", 1)["b_state"].tolist() == [1, 1, 3, 0] and not QC.checked("tie", 2)["end_state"].any() and QC.checked("tie", 3)["info"]["joins"] == 0
    # choice(R0) = L1 but choice(L1) = R2
    w = QC.checked("mutual")
    assert w["b_state"].tolist() == [SC.B_SUPPORTED, SC.B_SUPPORTED | SC.B_JOIN] and layout(w) == [[(0, 0)], [(1, 1), (2, 1)]]
    assert w["end_state"].tolist() == [0, 1, 1 | 4, 0, 0, 1 | 4]
    # the cycles are opened at the left end of their smallest contig
    w = QC.checked("ring3")
    dropped = [(int(a), int(b)) for a, b, s in zip(w["b_a"], w["b_b"], w["b_state"]) if s & SC.B_DROPPED_CYCLE]
    assert dropped == [(2 * 1, 2 * 3)] and layout(w) == [[(0, 0), (2, 0)], [(1, 0), (4, 0), (3, 1)]] and w["end_state"][2] == SC.E_HAS_SUPPORTED
    w = QC.checked("ring2")
    dropped = [(int(a), int(b)) for a, b, s in zip(w["b_a"], w["b_b"], w["b_state"]) if s & SC.B_DROPPED_CYCLE]
    assert dropped == [(2 * 1, 2 * 2 + 1)] and layout(w) == [[(0, 0)], [(1, 0), (2, 0)]] and w["join_links"].tolist() == [0, 9, 0]
    # spans at max_insert and one above
    w = QC.checked("too_far")
    assert (w["info"]["links"], w["info"]["links_too_far"]) == (8, 3) and w["b_links"].tolist() == [5, 3] and w["b_span"].tolist() == [300 + 299 + 298 + 297 + 296, 300 + 299 + 60]
    assert QC.checked("too_far", 1)["b_links"].tolist() == [7, 4] and QC.checked("too_far", 2)["b_links"].tolist() == [4, 2]
    # gaps below min_gap and below 0: the N run is min_gap
    w = QC.checked("neg_gap")
    assert w["b_gap"].tolist() == [100 - 152, 100 - 95] and w["gap_after"].tolist() == [10, 10, 0] and w["s_len"].tolist() == [620]
    assert QC.checked("neg_gap", 1)["gap_after"].tolist() == [1, 5, 0] and QC.checked("neg_gap", 2)["gap_after"].tolist() == [60, 60, 0]
    assert QC.checked("neg_gap", 3)["b_gap"].tolist() == [-152, -95]
    # 300 contigs in one path
    c, w = QC.case("long_chain"), QC.checked("long_chain")
    assert layout(w) == [QC.long_chain_truth()] and 0 < int(w["orient"].sum()) < 300 and (c["tlen"].min(), c["tlen"].max()) == (30, 129)
    assert w["rank"][[p[0] for p in QC.long_chain_truth()]].tolist() == list(range(300)) and (w["b_gap"] < 10).any() and (w["b_gap"] > 10).any()
    # one bundle of 3000 links beside bundles of one
    w = QC.checked("big_bundle")
    assert sorted(w["b_links"].tolist()) == [1] * 24 + [3000] and layout(w)[0] == [(0, 0), (1, 0)] and w["info"]["longest"] == 2900 + int(w["gap_after"][0])
    assert QC.checked("big_bundle", 1)["end_state"][0] == SC.E_HAS_SUPPORTED | SC.E_AMBIGUOUS
    # empty targets between the members, short contigs and short gaps
    c, w = QC.case("seams"), QC.checked("seams")
    assert layout(w) == [QC.SEAM_CHAIN, [(6, 0)], [(7, 0), (10, 1)], [(13, 0)]] and w["scaffold"][[1, 3, 4, 8, 11]].tolist() == [-1] * 5
    assert w["gap_after"][[0, 9, 2, 14, 5, 12]].tolist() == [3, 3, 3, 3, 3, 0] and QC.checked("seams", 1)["gap_after"][0] == 7 and QC.checked("seams", 2)["gap_after"][0] == 3
    assert "NNN" in SC.fasta(w, c["seqs"]).decode().split("\n")[1][40:46]


def test_n50():
    assert SC.n50([]) == 0 and SC.n50([0, 0]) == 0 and SC.n50([5]) == 5 and SC.n50([2, 2, 2, 3, 3, 4, 8, 8]) == 8 and SC.n50([1, 2, 3, 4, 5, 6, 7, 8, 9, 10]) == 7


def test_planted_genome():
    """three contigs of a 4000-base genome, 1000 pairs with outer inserts of 300 .. 400: one scaffold in the true order and orientations; the
    estimated gaps lie within 100 (the width of the insert range: every linking pair's span is its insert minus the true gap) of 80 and 60"""
    c, g = QC.planted_genome()
    pl = P.place(*PC.args(c))
    insert = pl["info"]["insert_median"]
    assert 300 <= insert <= 400
    w = SC.scaffold_dicts(*QC.scaffold_args(c, pl), insert=insert)
    assert_same(SC.scaffold_walk(*QC.scaffold_args(c, pl), insert=insert), w, "planted genome")
    print(insert, w["info"], w["b_links"], w["b_gap"])
    assert (w["b_links"] >= 5).all() and len(w["b_links"]) == 2
    assert layout(w) == [QC.PLANTED_TRUTH] and w["info"]["scaffolds"] == 1 and w["info"]["joins"] == 2
    assert abs(int(w["gap_after"][1]) - 80) <= 100 and abs(int(w["gap_after"][0]) - 60) <= 100
    assert (insert, w["gap_after"].tolist(), w["b_links"].tolist()) == PLANTED_PINNED
    # the scaffold read back is the genome, reverse-complemented (it starts at the contig of the genome's end), with the gaps as N
    seq = SC.fasta(w, c["seqs"]).decode().split("\n")[1]
    rc = "".join("ACGT"[x] for x in P.revcomp(g))
    assert seq.replace("N", "") == rc[:1420] + rc[1500:2740] + rc[2800:]
    assert w["info"]["n50_targets"] == 1240 and w["info"]["n50_scaffolds"] == w["info"]["longest"] == int(w["s_len"][0])


PLANTED_PINNED = (348, [46, 68, 0], [21, 30])                                 # (insert median, gap_after, b_links) from the checker


def test_refusals_of_the_checker():
    c, pl = QC.case("two"), QC.placed("two")
    args = QC.scaffold_args(c, pl)
    for kw in (dict(insert=-1), dict(insert=2 ** 20 + 1), dict(max_insert=0), dict(max_insert=2 ** 20 + 1), dict(min_links=0), dict(max_second_percent=0),
               dict(max_second_percent=101), dict(min_gap=0), dict(min_gap=2 ** 20 + 1)):
        with pytest.raises(ValueError):
            SC.scaffold_dicts(*args, **dict(QC.DEFAULT, **kw))
    for fn in (SC.scaffold_dicts, SC.scaffold_walk):
        with pytest.raises(ValueError):
            fn(c["rows"][:-2], c["lens"][:-2], c["pair_off"][:-2], pl, **QC.DEFAULT)
        bad = c["pair_off"].copy()
        bad[2] = bad[3] = 0                                                      # the mate of read 0 does not point back
        with pytest.raises(ValueError):
            fn(c["rows"], c["lens"], bad, pl, **QC.DEFAULT)
    c, pl = QC.case("seams"), QC.placed("seams")
    v = int(np.nonzero(pl["target"] == 9)[0][0])                                 # a read of 25 bases over all of a target of 25
    assert pl["state"][v] & P.UNIQUE and 16 * c["rows"].shape[1] == 32
    for fn in (SC.scaffold_dicts, SC.scaffold_walk):
        for length in (33, 0, -1, 26):                                           # past the stride, empty, removed, past the end of its target
            longer = c["lens"].copy()
            longer[2 * v] = longer[2 * v + 1] = length
            with pytest.raises(ValueError):
                fn(c["rows"], longer, c["pair_off"], pl, **QC.DEFAULT)


def test_library_exports_the_calls_and_the_header_declares_them():
    lib = alga_amd.load_library()
    header = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in alga_amd.engine.EXPORTS
        assert re.search(r"^(void|int)\s+%s\(" % sym, header, re.M), sym
    assert lib.alga_abi_version() == 7                                       # the calls only add to the ABI
    m = re.search(r"typedef struct \{\s*int32_t insert, max_insert, min_links, max_second_percent, min_gap, flags;\s*int32_t reserved\[2\];[^}]*\} alga_scaffold_params;", header)
    assert m
    for name, v in (("BUNDLE_SUPPORTED", 1), ("BUNDLE_JOIN", 2), ("BUNDLE_DROPPED_CYCLE", 4), ("END_HAS_SUPPORTED", 1), ("END_AMBIGUOUS", 2), ("END_JOINED", 4)):
        assert re.search(r"#define ALGA_SCAFFOLD_%s\s+%d\b" % (name, v), header) and getattr(alga_amd.engine, "SCAFFOLD_" + name) == v
    p = alga_amd.ScaffoldParams()
    lib.alga_scaffold_default_params(C.byref(p))
    assert (p.insert, p.max_insert, p.min_links, p.max_second_percent, p.min_gap, p.flags) == (0, 1000, 5, 50, 10, 0) and list(p.reserved) == [0] * 2
    assert dict(max_insert=p.max_insert, min_links=p.min_links, max_second_percent=p.max_second_percent, min_gap=p.min_gap) == SC.DEFAULT
    assert C.sizeof(alga_amd.ScaffoldParams) == 32 and C.sizeof(alga_amd.ScaffoldInfo) == 8 * (13 + 3) and C.sizeof(alga_amd.ScaffoldsC) == 8 * (4 + 16)
    assert [k for k, _ in alga_amd.ScaffoldInfo._fields_][:13] == list(SC.COUNTERS) and [k for k, _, _, _ in alga_amd.Scaffolds.KEYS] == list(SC.ARRAYS)
    assert callable(alga_amd.Engine.scaffold) and callable(alga_amd.Engine.write_scaffold_fasta) and callable(alga_amd.Scaffolds.to_host) and callable(alga_amd.Scaffolds.layout_tsv)
    w, c = QC.checked("orient"), QC.case("orient")
    assert alga_amd.engine.layout_tsv(w, c["tlen"]).encode() == SC.layout_tsv(w, c["tlen"]) == alga_amd.engine.layout_tsv(w).encode()
    for name in ("seams", "ring3", "n0"):                                    # the lengths taken from the result itself
        assert alga_amd.engine.layout_tsv(QC.checked(name)).encode() == SC.layout_tsv(QC.checked(name), QC.case(name)["tlen"])
    binary = open(alga_amd.library_path(), "rb").read()
    for k in KERNELS:
        assert k.encode() in binary


def test_new_kernels_resources():
    """The compiler's resource report of scaffold_kernels.hip and chain_kernels.hip: every k_sc_* and k_ch_* is there, no VGPR spill and no
    scratch in any of them"""
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_scaffold_resources_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    lines = []
    for name in ("scaffold_kernels.hip", "chain_kernels.hip"):
        src = os.path.join(ROOT, "alga_amd", "csrc", name)
        try:
            r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                               capture_output=True, text=True, check=True)
        finally:
            if os.path.exists(out):
                os.remove(out)
        lines += r.stderr.splitlines()
    reps = {}
    for i, s in enumerate(lines):
        m = re.search(r"Function Name: \S*?(k_(?:sc|ch)_[a-z_]+)E", s)
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
        assert int(rep["VGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, (name, rep)
    print(reps)
