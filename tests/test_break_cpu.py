"""The break stage without a GPU: the two Python statements of the definition (tests/break_checker.py) agree on the cases of
tests/break_cases.py, the outcomes the cases were made for, the planted chimera; the refusals of the checker; the library exports the calls
and the header declares them; the compiler's resource report of break_kernels.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import break_cases as QC
import break_checker as BC
import place_cases as PC
import place_checker as P
import scaffold_checker as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_br_check", "k_br_pairs", "k_br_flags", "k_br_runs", "k_br_closed", "k_br_cuts", "k_br_pieces", "k_br_copy", "k_br_fasta_sizes", "k_br_fasta_write"]
SYMBOLS = ("alga_break_default_params", "alga_break_placed_device", "alga_write_broken_fasta_device")
# (runs, runs_open, cuts) of every variant of every case
OUTCOMES = {"one_cut": [(1, 0, 1), (1, 0, 1), (0, 0, 0), (2, 0, 2)], "threshold": [(1, 0, 1), (0, 0, 0), (0, 0, 0), (1, 1, 0), (3, 2, 1)],
            "inset": [(3, 0, 3), (2, 0, 2), (4, 0, 4)], "midpoint": [(9, 0, 9), (9, 0, 9), (8, 0, 8)], "open": [(5, 4, 1), (7, 6, 1), (4, 4, 0)],
            "seams": [(13, 5, 8), (15, 7, 8), (8, 0, 8)], "many_cuts": [(338, 0, 338)], "not_proper": [(3, 2, 1)], "pile_up": [(1, 0, 1)], "no_pairs": [(2, 2, 0)],
            "n0": [(1, 1, 0)], "t0": [(0, 0, 0)], "all_empty": [(0, 0, 0)]}


def assert_same(got, want, what=""):
    for k in BC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    assert got["info"] == want["info"], (what, got["info"], want["info"])


def local_cuts(res):
    """[(target, cut, run_first, run_last)] in target-local columns"""
    return [tuple(int(x) for x in line.split("\t")) for line in BC.cuts_tsv(res).decode().splitlines()]


@pytest.mark.parametrize("name,i", QC.every())
def test_the_two_statements_agree(name, i):
    c, pl, want = QC.case(name), QC.placed(name), QC.checked(name, i)
    v = c["variants"][i]
    got = BC.break_columns(*QC.break_args(c, pl), **v)
    assert_same(got, want, (name, i))
    info = want["info"]
    assert (info["runs"], info["runs_open"], info["cuts"]) == OUTCOMES[name][i], info
    # what holds for every result
    tlen = c["tlen"].astype(np.int64)
    T = len(tlen)
    assert info["pairs_proper"] == pl["info"]["pairs_proper"] >= info["pairs_spanning"] and info["pieces"] == T + info["cuts"] == len(want["len"])
    assert info["runs"] == info["runs_open"] + info["cuts"] and int(want["t_cuts"].sum()) == info["cuts"] and info["targets_cut"] == int((want["t_cuts"] > 0).sum())
    assert (np.diff(want["cut_cols"].astype(np.int64)) > 0).all() and (np.diff(want["piece_off"].astype(np.int64)) >= 0).all()
    assert (want["cut_first"] <= want["cut_cols"]).all() and (want["cut_cols"] <= want["cut_last"]).all()
    assert (want["span"][want["cut_cols"]] < v["min_span"]).all() if info["cuts"] else True
    for t in range(T):                                                          # nothing is removed: the pieces of a target sum to its length
        assert int(want["len"][want["piece_target"] == t].sum()) == tlen[t]
    assert (want["begin"] == want["piece_off"][:-1]).all() and (want["len"] == np.diff(want["piece_off"].astype(np.int64))).all()
    assert int(want["piece_off"][-1]) == int(tlen.sum()) and sorted(want["piece_target"].tolist()) == want["piece_target"].tolist()
    seqs = BC.pieces_of(want)
    for t in range(T):
        parts = [seqs[j] for j in range(len(seqs)) if want["piece_target"][j] == t]
        assert (np.concatenate(parts) == c["seqs"][t]).all()
    # the rendered FASTA: one record per piece with a length; the cuts as text
    text = BC.fasta(want).decode().split("\n")
    assert text[-1] == "" and [len(s) for s in text[1::2]] == [int(n) for n in want["len"] if n > 0]
    assert len(local_cuts(want)) == info["cuts"]
    print(name, i, info)


def test_every_case_is_listed():
    assert sorted(OUTCOMES) == sorted(QC.CASES) and all(len(OUTCOMES[n]) == len(QC.case(n)["variants"]) for n in QC.CASES)
    for need in ("one_cut", "threshold", "inset", "midpoint", "open", "seams", "many_cuts", "not_proper", "pile_up", "no_pairs", "n0", "t0", "all_empty"):
        assert need in QC.CASES


def test_outcomes_the_cases_were_made_for():
    # with inset 20 the fragments of 40 columns span nothing: the run is 272 .. 319, its middle 296; with min_span 2 it is wider
    assert local_cuts(QC.checked("one_cut", 0)) == [(0, 296, 272, 319)]
    w = QC.checked("one_cut", 1)
    assert local_cuts(w)[0][1] == 296 and local_cuts(w)[0][2] < 272 and local_cuts(w)[0][3] > 319 and QC.checked("one_cut", 1)["info"]["pairs_spanning"] == 51
    assert QC.checked("one_cut", 2)["info"]["weak_columns"] == 0                      # whole fragments: the short ones bridge the gap
    assert local_cuts(QC.checked("one_cut", 3)) == [(0, 284, 273, 294), (0, 308, 297, 318)]   # inset 19: they span 295 and 296
    # span 2 is weak for min_span 3 and not for 2; span 5 is not weak for 5, span 3 is
    w = QC.checked("threshold", 0)
    assert local_cuts(w) == [(0, 205, 200, 209)] and w["span"][199] == 5 and w["span"][200] == 2 and w["span"][210] == 5 and w["span"][260] == 3
    assert QC.checked("threshold", 1)["info"]["weak_columns"] == 0 and QC.checked("threshold", 3)["info"]["weak_columns"] == 340
    assert local_cuts(QC.checked("threshold", 4)) == [(0, 205, 200, 209)]           # 30 .. 149 and 260 .. 369 (span 3) are open
    # a fragment of 2 * inset columns spans nothing, one of 2 * inset + 1 exactly one column
    w = QC.checked("inset", 0)
    assert w["info"]["pairs_spanning"] == 5 and local_cuts(w) == [(0, 150, 125, 174), (1, 137, 125, 149), (1, 163, 151, 174)] and w["span"][300 + 150] == 1
    assert local_cuts(QC.checked("inset", 1)) == [(0, 150, 124, 175), (1, 150, 124, 175)]
    # every run length at every position relative to a wave and a block; the cut is the middle, rounded up
    w = QC.checked("midpoint", 0)
    assert local_cuts(w) == [(0, (2 * s + n) // 2, s, s + n - 1) for s, n in QC.MID_RUNS]
    assert [c for _, c, _, _ in local_cuts(w)] == [63, 128, 193, 257, 352, 544, 735, 960, 1429]
    assert local_cuts(QC.checked("midpoint", 1)) == local_cuts(w) and local_cuts(QC.checked("midpoint", 2)) == local_cuts(w)[1:]   # margin 64: the run at 63 is open
    # the open runs cut nothing; the target of 2 * margin + 3 columns is cut at its middle
    w = QC.checked("open", 0)
    assert local_cuts(w) == [(6, 31, 31, 31)] and w["t_cuts"].tolist() == [0, 0, 0, 0, 0, 0, 1] and w["info"]["candidate_columns"] == 140 + 3 * 240 + 0 + 1 + 3
    assert w["info"]["weak_columns"] == 140 + 70 + 70 + 0 + 0 + 1 + 1
    w = QC.checked("open", 1)                                                          # margin 0: runs at a target's first or last column are open
    assert local_cuts(w) == [(6, 31, 31, 31)] and w["info"]["runs_open"] == 6
    assert QC.checked("open", 2)["info"]["cuts"] == 0                                   # margin 31: column 30 of target 6 is no candidate any more
    # weak columns at the end of one target and the start of the next are two runs; cuts in neighbouring targets
    c, w = QC.case("seams"), QC.checked("seams", 1)
    assert [t for t, _, _, _ in local_cuts(w)] == [0, 2, 5, 7, 9, 10, 12, 14] and all(cut == QC.SEAM_LENS[t] // 2 for t, cut, _, _ in local_cuts(w))
    assert w["len"][:6].tolist() == [70, 70, 0, 66, 67, 0] and len(w["len"]) == 15 + 8 and (c["tbegin"][1:] == c["tbegin"][:-1] + c["tlen"][:-1]).sum() >= 4
    # both bisections of the piece numbering: targets before and behind 300 cuts, cuts before and behind targets
    w = QC.checked("many_cuts")
    assert w["t_cuts"].tolist() == [t % 3 for t in range(20)] + [300] + [t % 3 for t in range(21, 41)]
    first = int(np.nonzero(w["piece_target"] == 20)[0][0])
    assert first == 20 + sum(t % 3 for t in range(20)) and (w["piece_target"][first:first + 301] == 20).all() and w["piece_target"][first + 301] == 21
    assert w["piece_start"][first:first + 301].tolist() == [0] + [66 * i + 1 for i in range(1, 301)]
    # reads that are no proper pair do not span
    w = QC.checked("not_proper")
    assert local_cuts(w) == [(0, 200, 180, 219)] and (QC.placed("not_proper")["cover"][180:220] > 0).all() and (w["span"][180:220] == 0).all()
    pi = QC.placed("not_proper")["info"]
    assert (pi["pairs_improper"], pi["pairs_split"], pi["pairs_not_unique"]) == (1, 1, 1)
    # contended adds beside columns of span 1
    w = QC.checked("pile_up")
    assert w["info"]["max_span"] == 3001 and w["span"][99] == 1 and w["span"][110] == 3000 and local_cuts(w) == [(0, 305, 300, 309)]
    # the judging mate is the `-` read in half of the pairs
    pl = QC.placed("one_cut")
    judges = pl["state"][0::2]
    assert 0 < int((judges & P.MINUS > 0).sum()) < len(judges)


def test_planted_chimera():
    """two contigs of a 4000-base genome, the second joined wrongly at its column 1300: one cut, on the chimera, within inset columns of the
    junction; the pieces scaffold into the genome's true order and orientation, the unbroken set into nothing; a second round cuts nothing"""
    c, g = QC.chimera()
    pl = P.place(*PC.args(c))
    median = pl["info"]["insert_median"]
    v = c["variants"][0]
    w = BC.break_pairs(*QC.break_args(c, pl), margin=median, **v)
    assert_same(BC.break_columns(*QC.break_args(c, pl), margin=median, **v), w, "chimera")
    print(pl["info"], w["info"], local_cuts(w))
    assert w["info"]["cuts"] == 1 and w["info"]["runs"] == 1 and w["t_cuts"].tolist() == [0, 1]
    (t, cut, first, last), = local_cuts(w)
    assert t == 1 and abs(cut - QC.CHIMERA_JUNCTION) <= v["inset"]
    assert (median, pl["info"]["pairs_proper"], pl["info"]["pairs_split"], first, last, cut) == CHIMERA_PINNED
    assert BC.break_pairs(*QC.break_args(c, pl), margin=median, min_span=1, inset=0)["info"]["cuts"] == 0   # why inset is in the rule
    # the unbroken set gives no join
    before = SC.scaffold_dicts(c["rows"], c["lens"], c["pair_off"], pl, insert=median)
    assert before["info"]["joins"] == 0 and before["info"]["scaffolds"] == 2 and before["info"]["links_too_far"] == pl["info"]["pairs_split"]
    # the pieces: piece 1 +, target 0 -, piece 2 +
    c2 = QC.pieces_case(c, w)
    pl2 = P.place(*PC.args(c2))
    after = SC.scaffold_dicts(c2["rows"], c2["lens"], c2["pair_off"], pl2, insert=pl2["info"]["insert_median"])
    layout = [(int(m), int(after["orient"][m])) for m in after["s_members"]]
    assert layout == [(1, 0), (0, 1), (2, 0)] and after["info"]["joins"] == 2 and after["info"]["scaffolds"] == 1
    assert (pl2["info"]["pairs_proper"], pl2["info"]["pairs_split"], after["join_links"].tolist()) == CHIMERA_PINNED_AFTER
    assert (w["info"]["n50_targets"], w["info"]["n50_pieces"], after["info"]["n50_scaffolds"]) == (2600, 1303, 4020)
    seq = SC.fasta(after, c2["seqs"]).decode().split("\n")[1]
    truth = "".join("ACGT"[x] for x in g)
    # (the cut falls 3 columns before the junction: those 3 bases go with the second piece)
    assert seq.replace("N", "") == truth[:cut] + truth[QC.CHIMERA_JUNCTION:2700] + truth[cut:QC.CHIMERA_JUNCTION] + truth[2700:]
    again = BC.break_pairs(c2["rows"], c2["lens"], c2["pair_off"], pl2, c2["seqs"], margin=pl2["info"]["insert_median"], **v)
    assert again["info"]["cuts"] == 0


CHIMERA_PINNED = (351, 815, 79, 1280, 1314, 1297)                             # (median, proper, split, run first, run last, cut) from the checker
CHIMERA_PINNED_AFTER = (813, 76, [38, 38, 0])                                 # (proper, split, join links by piece) on the pieces


def test_refusals_of_the_checker():
    c, pl = QC.case("one_cut"), QC.placed("one_cut")
    args = QC.break_args(c, pl)
    for kw in (dict(min_span=0), dict(min_span=2 ** 31), dict(inset=-1), dict(inset=2 ** 20 + 1), dict(margin=-1), dict(margin=2 ** 20 + 1)):
        for fn in (BC.break_columns, BC.break_pairs):
            with pytest.raises(ValueError):
                fn(*args, **dict(QC.DEFAULT, **kw))
    for fn in (BC.break_columns, BC.break_pairs):
        with pytest.raises(ValueError):
            fn(c["rows"][:-2], c["lens"][:-2], c["pair_off"][:-2], pl, c["seqs"], **QC.DEFAULT)
        bad = c["pair_off"].copy()
        bad[2] = bad[3] = 0                                                      # the mate of read 0 does not point back
        with pytest.raises(ValueError):
            fn(c["rows"], c["lens"], bad, pl, c["seqs"], **QC.DEFAULT)
        big = c["pair_off"].copy()
        big[0] = big[1] = 3
        with pytest.raises(ValueError):
            fn(c["rows"], c["lens"], big, pl, c["seqs"], **QC.DEFAULT)
    c, pl = QC.case("open"), QC.placed("open")
    v = int(np.nonzero((pl["target"] == 6) & (pl["pos"] == 38))[0][0])           # the `-` read of the pair (6, 32, 63): it ends at the target's end
    assert pl["state"][v] & P.UNIQUE and 16 * c["rows"].shape[1] == 32
    for fn in (BC.break_columns, BC.break_pairs):
        for length in (33, 0, -1, 26):                                           # past the stride, empty, removed, past the end of its target
            longer = c["lens"].copy()
            longer[2 * v] = longer[2 * v + 1] = length
            with pytest.raises(ValueError):
                fn(c["rows"], longer, c["pair_off"], pl, c["seqs"], **QC.DEFAULT)
        for key, value in (("target", len(c["tlen"])), ("target", -1), ("pos", -1), ("pos", 39)):
            moved = dict(pl, **{key: pl[key].copy()})
            moved[key][v] = value
            with pytest.raises(ValueError):
                fn(c["rows"], c["lens"], c["pair_off"], moved, c["seqs"], **QC.DEFAULT)


def test_library_exports_the_calls_and_the_header_declares_them():
    lib = alga_amd.load_library()
    header = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in alga_amd.engine.EXPORTS
        assert re.search(r"^(void|int)\s+%s\(" % sym, header, re.M), sym
    assert lib.alga_abi_version() == 7                                       # the calls only add to the ABI
    assert re.search(r"typedef struct \{\s*int32_t min_span, inset, margin, flags;\s*int32_t reserved\[4\];[^}]*\} alga_break_params;", header)
    m = re.search(r"typedef struct \{([^}]*)\} alga_break_info;", header)
    assert m and re.findall(r"\b([a-z_0-9]+)[,;]", re.sub(r"/\*.*?\*/", "", m.group(1))) == [k for k, _ in alga_amd.BreakInfo._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} alga_broken;", header)
    assert m and [x.lstrip("*") for x in re.findall(r"(\*?\b[a-z_0-9]+)[,;]", re.sub(r"/\*.*?\*/", "", m.group(1)))] == [k for k, _ in alga_amd.BrokenC._fields_]
    p = alga_amd.BreakParams()
    lib.alga_break_default_params(C.byref(p))
    assert (p.min_span, p.inset, p.margin, p.flags) == (1, 21, 0, 0) and list(p.reserved) == [0] * 4
    assert dict(min_span=p.min_span, inset=p.inset) == BC.DEFAULT
    assert C.sizeof(alga_amd.BreakParams) == 32 and C.sizeof(alga_amd.BreakInfo) == 8 * (13 + 3) and C.sizeof(alga_amd.BrokenC) == 8 * (4 + 11)
    assert [k for k, _ in alga_amd.BreakInfo._fields_][:13] == list(BC.COUNTERS) and [k for k, _, _, _ in alga_amd.Broken.KEYS] == list(BC.ARRAYS)
    for fn in (alga_amd.Engine.break_contigs, alga_amd.Engine.write_broken_fasta, alga_amd.Broken.to_host, alga_amd.Broken.targets, alga_amd.Broken.cuts_tsv):
        assert callable(fn)
    for name in ("many_cuts", "seams", "n0", "inset"):
        assert alga_amd.engine.cuts_tsv(QC.checked(name)).encode() == BC.cuts_tsv(QC.checked(name))
    binary = open(alga_amd.library_path(), "rb").read()
    for k in KERNELS:
        assert k.encode() in binary


def test_new_kernels_resources():
    """The compiler's resource report of break_kernels.hip: every k_br_* is there, no VGPR spill and no scratch in any of them"""
    src = os.path.join(ROOT, "alga_amd", "csrc", "break_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_break_resources_%d.o" % os.getpid())
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
        m = re.search(r"Function Name: \S*?(k_br_[a-z_]+)E", s)
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
