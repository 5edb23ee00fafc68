"""The polish without a GPU: the two Python statements of the definition (tests/polish_checker.py) agree on the cases of
tests/polish_cases.py, the outcomes the cases were made for, the cover against the placement's, the whole chain on the checkers of every stage
(the seed of the GPU test's chain); the library exports the calls and the header declares them; the compiler's resource report of
polish_kernels.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import consensus_checker as S
import contig_checker as K
import final_checker as F
import graph_cases as GC
import oracle_lib as O
import place_checker as P
import polish_cases as QC
import polish_checker as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_po_check", "k_po_keys", "k_po_vote", "k_po_vote_wide", "k_po_changes", "k_po_fasta_sizes", "k_po_fasta_write"]
SYMBOLS = ("alga_polish_default_params", "alga_polish_placed_device", "alga_write_polished_fasta_device")
# (changed, ambiguous) of every variant of every case
OUTCOMES = {"planted": [(49, 0)], "ties": [(2, 4), (5, 1), (3, 4), (4, 1), (1, 5), (7, 0)], "deep": [(3, 1)], "long_among_short": [(33, 0), (29, 0)],
            "seams": [(31, 0), (47, 0)], "seams16": [(31, 0), (47, 0)], "minus_only": [(5, 0)], "multi": [(2, 0), (3, 0)],
            "nobody_unplaced": [(0, 0)] * 2, "nobody_n0": [(0, 0)] * 2, "nobody_t0": [(0, 0)] * 2}


def assert_same(got, want, what=""):
    for k in Q.ARRAYS + ("counts", "cover", "seq"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    assert got["info"] == want["info"], (what, got["info"], want["info"])


@pytest.mark.parametrize("name,i", QC.every())
def test_the_two_statements_agree(name, i):
    c = QC.case(name)
    v = c["variants"][i]
    pl = QC.placed(name, v["multi"])
    want = QC.checked(name, i)
    got = Q.polish_gather(*QC.polish_args(c, pl), min_cover=v["min_cover"], min_percent=v["min_percent"], flags=QC.polish_flags(v))
    assert_same(got, want, (name, i))
    assert (want["info"]["changed"], want["info"]["ambiguous"]) == OUTCOMES[name][i], (name, i, want["info"])
    # the depth mode of the placement agrees with the voters: its cover is the polish's
    assert (want["cover"] == pl["cover"]).all() and want["info"]["votes"] == int(pl["t_bases"].sum()) == int(want["counts"].sum())
    assert (want["col_off"] == pl["col_off"]).all() and len(want["words"]) == (want["info"]["columns"] + 15) // 16 + 2
    n = want["info"]["columns"]
    assert not want["words"][n // 16:].any() if n % 16 == 0 else want["words"][n // 16] >> (2 * (n % 16)) == 0 and not want["words"][n // 16 + 1:].any()
    assert int(want["t_changed"].sum()) == want["info"]["changed"] == len(want["changed_cols"]) and int(want["t_ambiguous"].sum()) == want["info"]["ambiguous"]
    assert ((want["changed_bases"] & 3) != (want["changed_bases"] >> 2)).all() and (np.diff(want["changed_cols"].astype(np.int64)) > 0).all()
    print(name, i, want["info"])


def test_every_case_is_listed():
    assert sorted(OUTCOMES) == sorted(QC.CASES) and all(len(OUTCOMES[n]) == len(QC.case(n)["variants"]) for n in QC.CASES)


def test_planted():
    """the recipe of the case: 353 reads, 344 unique, mm up to 4; of the 55 planted columns 49 change back to the truth and the 6 that stay are
    exactly those with a cover below 3; nothing else changes"""
    c, pl, w = QC.case("planted"), QC.placed("planted"), QC.checked("planted")
    assert (pl["info"]["reads"], pl["info"]["unique"], int(pl["mm"].max())) == (353, 344, 4)
    off = w["col_off"].astype(np.int64)
    planted = np.concatenate([off[t] + np.array(QC.planted_columns(n), np.int64) for t, n in enumerate(QC.PLANTED_LENS)])
    truth = np.concatenate(c["truths"])
    assert len(planted) == 55 and len(truth) == 2050 == w["info"]["columns"]
    deep = w["cover"][planted] >= 3
    assert sorted(w["cover"][planted][~deep].tolist()) == [0, 0, 1, 1, 1, 1] and deep.sum() == 49
    assert w["changed_cols"].tolist() == planted[deep].tolist()
    assert (w["seq"][w["cover"] >= 3] == truth[w["cover"] >= 3]).all() and (w["seq"] != truth).sum() == 6
    assert ((w["changed_bases"] >> 2) == truth[w["changed_cols"]]).all()
    # the second round: placed on the polished targets, every planted column that changed has reads without a mismatch over it and is unanimous, nothing changes
    tw, tb, tl = Q.targets_of(w)
    pl2 = P.place(c["rows"], c["lens"], None, tw, tb, tl, **c["params"])
    w2 = Q.polish_scatter(c["rows"], c["lens"], pl2, tw, tb, tl)
    assert w2["info"]["changed"] == 0 and (w2["words"] == w["words"]).all()
    for g in planted[deep]:
        over = [r for r in range(len(pl2["state"])) if pl2["state"][r] & P.UNIQUE and 0 <= g - (off[pl2["target"][r]] + pl2["pos"][r]) < c["lens"][2 * r]]
        # (a read over it may still cover one of the six columns that stayed, as the read at 0 covers column 2: not every read has mm 0)
        assert len(over) >= 3 and any(pl2["mm"][r] == 0 for r in over) and w2["counts"][g].max() == w2["cover"][g], g


def test_outcomes_the_cases_were_made_for():
    c = QC.case("ties")
    off = QC.checked("ties")["col_off"].astype(np.int64)
    col = lambda t: int(off[t]) + 70

    def at(i):
        w = QC.checked("ties", i)
        return [("C" if col(t) in w["changed_cols"] else "A" if col(t) in w["ambiguous_cols"] else ".") for t in range(len(QC.TIES))]
    assert "".join(at(0)) == ".AA.CCAA" and "".join(at(1)) == ".CC.CCCA" and "".join(at(2)) == ".AACCCAA"
    assert "".join(at(3)) == ".CC..CCA" and "".join(at(4)) == ".AA.CAAA" and "".join(at(5)) == ".CCCCCCC"
    w = QC.checked("ties", 1)
    cur = np.concatenate([P.codes_of(c["twords"], c["tbegin"][t], 120) for t in range(len(QC.TIES))])
    new = {int(g): int(b) >> 2 for g, b in zip(w["changed_cols"], w["changed_bases"])}
    assert new[col(1)] == min((cur[col(1)] + 1) & 3, (cur[col(1)] + 2) & 3) and new[col(2)] == min((cur[col(2)] + 1) & 3, (cur[col(2)] + 3) & 3)
    assert w["counts"][col(7)].tolist().count(3) == 2 and w["cover"][[col(t) for t in range(8)]].tolist() == [4, 4, 4, 2, 3, 5, 7, 7]
    w = QC.checked("deep")
    off = w["col_off"].astype(np.int64)
    assert w["cover"][100:140].min() >= 301 and w["cover"][99] == 1 and w["cover"][140] == 2 and w["cover"][150] == 1 and w["cover"][[125, 130, 135]].tolist() == [301, 302, 302]
    assert w["changed_cols"].tolist() == [130, int(off[1]) + 60, int(off[2]) + 60] and w["ambiguous_cols"].tolist() == [125]
    assert sorted(w["counts"][125].tolist()) == [0, 0, 150, 151] and sorted(w["counts"][130].tolist()) == [0, 0, 102, 200]
    assert int(w["cover"][off[1]:off[2]].max()) == 255 and int(w["cover"][off[2]:].max()) == 256
    c, w = QC.case("long_among_short"), QC.checked("long_among_short")
    assert sorted(c["lens"].tolist())[-3:] == [100, 2800, 2800] and (w["seq"][w["cover"] >= 3] == c["truths"][0][w["cover"] >= 3]).all()
    assert (w["cover"][150:2950] >= 4).all()
    for name, rest in (("seams", 1), ("seams16", 0)):
        c, w = QC.case(name), QC.checked(name)
        assert w["info"]["columns"] % 16 == rest and int((c["tlen"] == 0).sum()) >= 15
        seams = w["col_off"][1:-1]
        assert len(set((seams >> 4).tolist())) < len(set(seams.tolist()))               # several seams inside one word
        w2 = QC.checked(name, 1)
        truth = np.concatenate(c["truths"])
        assert (w2["seq"][w2["cover"] >= 2] == truth[w2["cover"] >= 2]).all() and w2["info"]["changed"] > w["info"]["changed"] > 0
    pl = QC.placed("minus_only")
    assert (pl["state"] == P.PLACED | P.UNIQUE | P.MINUS).all() and QC.checked("minus_only")["info"]["voters"] == 62
    pl = QC.placed("multi")
    assert (pl["state"][:5] & (P.PLACED | P.UNIQUE) == P.PLACED).all() and (pl["pos"][:5] < 200).all() and (pl["hits"][:5] == 2).all()
    assert QC.checked("multi", 0)["changed_cols"].tolist() == [60, 350] and QC.checked("multi", 1)["changed_cols"].tolist() == [60, 195, 350]
    assert QC.checked("multi", 1)["seq"][545] != QC.case("multi")["truths"][0][545]                                  # the second copy got no votes


def test_refusals_of_the_checker():
    c, pl = QC.case("planted"), QC.placed("planted")
    for kw in (dict(min_cover=0), dict(min_percent=0), dict(min_percent=101), dict(flags=4)):
        with pytest.raises(ValueError):
            Q.polish_scatter(*QC.polish_args(c, pl), **kw)
    with pytest.raises(ValueError):
        Q.polish_scatter(c["rows"][:-2], c["lens"][:-2], pl, c["twords"], c["tbegin"], c["tlen"])
    v = int(np.nonzero((pl["state"] & P.UNIQUE).astype(bool) & (pl["target"] == 4))[0][-1])
    for length in (16 * c["rows"].shape[1], 16 * c["rows"].shape[1] + 1, 0):      # past the end of its target (130 bases), past the stride, empty
        longer = c["lens"].copy()
        longer[2 * v] = longer[2 * v + 1] = length
        with pytest.raises(ValueError):
            Q.polish_gather(c["rows"], longer, pl, c["twords"], c["tbegin"], c["tlen"])


def test_whole_chain_on_the_checkers():
    """the chain of the GPU test on the checkers of every stage: the polished contigs are no further from the genome than the unpolished ones
    (the condition the seed was chosen under)"""
    words, lens, genome = QC.chain_reads()
    e, _, _ = O.prefsuf(words, lens, GC.MIN_OVERLAP, GC.RSOEMO)
    u = K.contigs(words, lens, O.cut_triangles(len(lens), e, GC.MOPP), GC.MOPP)
    cons = S.consensus_pileup(words, lens, u, 0)
    fin = F.final_contigs(u, cons, 150, 95, 25)
    tw, tb, tl = QC.final_targets(u, cons, fin)
    pl = P.place(words, lens, None, tw, tb, tl)
    w = Q.polish_scatter(words, lens, pl, tw, tb, tl)
    before = sum(QC.distance_to(genome, P.codes_of(tw, tb[j], int(tl[j]))) for j in range(len(tl)))
    after = sum(QC.distance_to(genome, s) for s in Q.sequences(w))
    print(fin["n_accepted"], w["info"], before, after)
    assert fin["n_accepted"] >= 3 and w["info"]["changed"] > 0 and after <= before and before > 0


def test_library_exports_the_calls_and_the_header_declares_them():
    lib = alga_amd.load_library()
    header = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in alga_amd.engine.EXPORTS
        assert re.search(r"^(void|int)\s+%s\(" % sym, header, re.M), sym
    assert lib.alga_abi_version() == 7                                       # the calls only add to the ABI
    m = re.search(r"typedef struct \{\s*int32_t min_cover, min_percent, flags;\s*int32_t reserved\[5\];[^}]*\} alga_polish_params;", header)
    assert m and re.search(r"#define ALGA_POLISH_MULTI\s+1\b", header) and re.search(r"#define ALGA_POLISH_COUNTS\s+2\b", header)
    p = alga_amd.PolishParams()
    lib.alga_polish_default_params(C.byref(p))
    assert (p.min_cover, p.min_percent, p.flags) == (3, 60, 0) and list(p.reserved) == [0] * 5
    assert C.sizeof(alga_amd.PolishParams) == 32 and C.sizeof(alga_amd.PolishInfo) == 8 * (7 + 3) and C.sizeof(alga_amd.PolishedC) == 8 * (3 + 7)
    assert callable(alga_amd.Engine.polish) and callable(alga_amd.Polished.targets) and callable(alga_amd.Polished.to_host)
    assert (alga_amd.engine.POLISH_MULTI, alga_amd.engine.POLISH_COUNTS) == (Q.MULTI, Q.COUNTS)
    binary = open(alga_amd.library_path(), "rb").read()
    for k in KERNELS:
        assert k.encode() in binary


def test_new_kernels_resources():
    """The compiler's resource report of polish_kernels.hip: every k_po_* is there, no VGPR spill and no scratch in any of them"""
    src = os.path.join(ROOT, "alga_amd", "csrc", "polish_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_polish_resources_%d.o" % os.getpid())
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
        m = re.search(r"Function Name: \S*?(k_po_[a-z_]+?)E[A-Z]", s)
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
