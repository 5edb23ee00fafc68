"""The polish with the gapped reads without a GPU: the two Python statements of the definition (tests/ipolish_checker.py) agree on every variant of
the cases of tests/ipolish_cases.py and on hand-made scripts no real gapped placement gives (a gap directly behind a gap); the outcomes the cases
were made for; the planted set on the checker alone; the checker's refusals; the library exports the calls and the header declares them; the
compiler's resource report of ipolish_kernels.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import gapped_checker as GC
import ipolish_cases as XC
import ipolish_checker as IC
import place_checker as P
import polish_checker as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_ip_check", "k_ip_vote_gapped", "k_ip_span", "k_ip_ins_pick", "k_ip_decide", "k_ip_words", "k_ip_events", "k_ip_targets", "k_ip_fasta_sizes",
           "k_ip_fasta_write", "k_ip_tsv_sizes", "k_ip_tsv_write"]
SYMBOLS = ("alga_ipolish_default_params", "alga_polish_indels_device", "alga_write_ipolished_fasta_device", "alga_write_ipolish_events_tsv_device")


def assert_same(got, want, what=""):
    for k in IC.ARRAYS + (("counts", "span") if "counts" in want else ()):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    assert got["info"] == want["info"], (what, got["info"], want["info"])


@pytest.mark.parametrize("name,i", XC.every())
def test_the_two_statements_agree(name, i):
    c, want = XC.case(name), XC.checked(name, i, True)
    pl, gp = XC.placed(name)
    got = IC.ipolish_gather(c["rows"], c["lens"], pl, gp, *XC.targets(c), flags=IC.COUNTS, **c["variants"][i])
    assert_same(got, want, (name, i))
    assert IC.fasta(got) == IC.fasta(want) and IC.events_tsv(got) == IC.events_tsv(want)
    assert (want["counts"].sum(axis=1) == gp["cover"]).all()                          # rule 3: the cover is the gapped cover
    n = len(gp["cover"])
    assert len(want["new_col"]) == n + 1 and int(want["new_col"][-1]) == want["info"]["columns_after"] == int(want["len"].sum())
    assert (np.diff(want["ev_col"].astype(np.int64)) >= 0).all()
    print(name, i, want["info"])


def synthetic(reads_and_scripts, target, unique_h=()):
    """a placement and a gapped placement written by hand: read r lies at pos with the given script (None: an H voter at pos) on one target"""
    reads = [r for r, _, _ in reads_and_scripts]
    rows, lens = P.nodes_of(reads)
    tw, tb, tl = P.ragged([target], [5])
    R = len(reads)
    pl = dict(state=np.zeros(R, np.uint8), target=np.full(R, -1, np.int32), pos=np.full(R, -1, np.int32), col_off=np.array([0, len(target)], np.uint32))
    gp = dict(state=np.zeros(R, np.uint8), target=np.full(R, -1, np.int32), pos=np.full(R, -1, np.int32), end=np.full(R, -1, np.int32), cover=np.zeros(len(target), np.uint32),
              t_reads=np.zeros(1, np.uint64))
    cig, off = [], [0]
    for r, (_, pos, script) in enumerate(reads_and_scripts):
        if script is None:
            pl["state"][r], pl["target"][r], pl["pos"][r] = P.PLACED | P.UNIQUE, 0, pos
        else:
            gp["state"][r], gp["target"][r], gp["pos"][r] = GC.PLACED | GC.UNIQUE | GC.INDEL, 0, pos
            gp["end"][r] = pos + sum(n for op, n in script if op != IC.OP_I)
            cig += [(n << 2) | op for op, n in script]
        off.append(len(cig))
    gp["cigar"], gp["cigar_off"] = np.array(cig, np.uint32), np.array(off, np.uint32)
    return rows, lens, pl, gp, tw, tb, tl


def test_hand_made_scripts():
    """what no canonical script holds, on both statements: a gap directly behind a gap (m = 0: it stays; the gap in front of it moves and leaves
    M cells between the two), a deleted column directly beside an inserted slot, a D run as the last run, a shift stopped by m and one stopped
    by the script's first column"""
    M, I, D = IC.OP_M, IC.OP_I, IC.OP_D
    A, Cc, G, T = 0, 1, 2, 3
    t = np.array([G, T, A, A, A, A, Cc, G, T, Cc, A, G, G, T, Cc, A, T, G], np.uint8)
    #             0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16 17
    v1 = np.array([G, T, A, A, A, A, A, T, Cc, A, G, G, T], np.uint8)          # 6M 1I 2D 6M on t from 0: an A more, then C G deleted
    s1 = [(M, 6), (I, 1), (D, 2), (M, 6)]
    v2 = np.array([A, A, A, A, Cc, G], np.uint8)                                # from column 3: 3M 1I 2M -- the shift would pass the first column: s = 3 = m
    s2 = [(M, 3), (I, 1), (M, 2)]
    v3 = np.array([T, Cc, A, G, G], np.uint8)                                   # from column 8: 5M 2D as the last run
    s3 = [(M, 5), (D, 2)]
    cases = [(v1, 0, s1)] * 3 + [(v2, 3, s2)] * 2 + [(v3, 8, s3)] + [(t[4:16].copy(), 4, None)]
    rows, lens, pl, gp, tw, tb, tl = synthetic(cases, t)
    for kw in (dict(min_cover=1), dict(min_cover=3), dict(min_cover=1, min_percent=30, max_ins=1)):
        a = IC.ipolish_scatter(rows, lens, pl, gp, tw, tb, tl, flags=IC.COUNTS, **kw)
        b = IC.ipolish_gather(rows, lens, pl, gp, tw, tb, tl, flags=IC.COUNTS, **kw)
        assert_same(b, a, kw)
    # v1: the I run has m = 6 and moves over the four A to the slot before column 2 (the M run shrinks to 2, four M cells stand behind the I run,
    # in front of the D run); the D run behind it has m = 0 and stays at columns 6, 7
    runs, sr, sb = IC.normalise_runs(s1, v1, t, 0)
    assert runs == [(M, 2), (I, 1), (M, 4), (D, 2), (M, 6)] and (sr, sb) == (1, 4)
    ev, er, eb = IC.gap_events(s1, v1, t, 0)
    assert [e[:4] for e in ev] == [[I, 2, 2, 1], [D, 6, 7, 2]] and (er, eb) == (1, 4)
    runs, sr, sb = IC.normalise_runs(s2, v2, t, 3)
    assert runs == [(M, 0), (I, 1), (M, 3), (M, 2)] and (sr, sb) == (1, 3)
    a = IC.ipolish_scatter(rows, lens, pl, gp, tw, tb, tl, min_cover=1, flags=IC.COUNTS)
    assert a["info"]["ins_votes"] == 5 and a["info"]["shifted_runs"] == 5 and a["info"]["ins_edge"] == 0 and a["info"]["del_votes"] == 3 * 2 + 2
    # slot 2 takes v1's three votes; v2's script begins at column 3 and its gap stops there (s = m = 3); columns 6 and 7 are deleted by v1 directly
    # behind the M cells its I run left; the edge D run of v3 votes `-` on columns 13 and 14
    assert a["counts"][6, 4] == 3 and a["counts"][7, 4] == 3 and a["counts"][13, 4] == 1 and a["counts"][14, 4] == 1 and a["counts"][:, 4].sum() == 8
    assert IC.events_tsv(a).split("\n")[0] == "0\t2\tI\t1\t-\tA\t3\t3"


def test_outcomes_the_cases_were_made_for():
    tsv = lambda name, i=0: IC.events_tsv(XC.checked(name, i)).splitlines()
    # the votes of reads with the gap in seed 0 (the run's last base) and further in (its first) pool at the run's first column; AC before ACACAC
    w, c = XC.checked("normalise"), XC.case("normalise")
    pl, gp = XC.placed("normalise")
    cig = GC.cigar_strings(gp)
    assert any(s.endswith("1I89M") or s.endswith("1I%dM" % n) for s in cig for n in range(80, 100)) and w["info"]["shifted_runs"] == 12 and w["info"]["ambiguous_slots"] == 0
    lines = tsv("normalise")
    assert lines[0].startswith("0\t200\tI\t1\t-\tA\t") and lines[1].startswith("0\t399\tD\t1\tT\t-\t") and lines[2].startswith("0\t600\tI\t2\t-\tAC\t")
    assert len(lines) == 5 and [x.split("\t")[2] for x in lines] == ["I", "D", "I", "D", "I"]
    g = XC.plain(101, 900)                                                           # the truth of that case comes back
    seq = IC.sequences(w)[0]
    assert len(seq) == 900 and int((seq != _truth_normalise()).sum()) == 0
    # ties: (`-`, cur, another base) per site
    c = XC.case("ties")
    col = c["cols"]
    kinds = lambda i: {int(x.split("\t")[1]): x.split("\t")[2] for x in tsv("ties", i)}
    assert kinds(0) == {col[2]: "D", col[4]: "D"} and XC.checked("ties", 0)["info"]["ambiguous_columns"] == 3     # 2:2 with cur stays; 3 of 3; 2 of 2 is below the cover; 3 of 5
    assert kinds(1) == {col[1]: "S", col[2]: "D", col[4]: "D", col[6]: "S"}                                      # at 50 %: the base wins the tie against `-`
    assert kinds(2) == kinds(0) and kinds(3) == {col[2]: "D"} and XC.checked("ties", 3)["info"]["ambiguous_columns"] == 4     # 3 of 5: 59 and 60 pass, 61 does not
    assert kinds(4) == {col[1]: "S", col[2]: "D", col[3]: "D", col[4]: "D", col[5]: "S", col[6]: "S"}             # cover 2 at min_cover 2; the three-way vote at 40 %
    assert XC.checked("ties", 0, True)["counts"][col[0]].tolist().count(2) == 2 and XC.checked("ties", 0, True)["counts"][col[5]].sum() == 5
    # insert_vote
    w = XC.checked("insert_vote")
    assert w["info"]["ins_edge"] == 6 and w["info"]["ins_too_long"] == 6 and w["info"]["voters_hamming"] == 0
    l0 = tsv("insert_vote")
    assert l0[0].split("\t")[2:4] == ["I", "1"] and l0[0].endswith("\t3\t5")                                       # 3 of 5 against another string
    assert w["ev_len"].tolist() == [1, 1, 2] and w["info"]["ambiguous_slots"] == 4                                 # the 7 and the 13 bases are counted, do not vote, and leave the slot ambiguous
    assert XC.checked("insert_vote", 2)["info"]["ins_too_long"] == 11 and XC.checked("insert_vote", 3)["info"]["ins_too_long"] == 0
    assert XC.checked("insert_vote", 3)["ev_len"].tolist() == [1, 1, 2, 7, 13] and tsv("insert_vote", 3)[-1].split("\t")[5] == "T" * 13
    assert XC.checked("insert_vote", 4)["ev_len"].tolist() == [1, 1, 1, 2, 7]                                       # span 2 at min_cover 2
    tie = [x for x in tsv("insert_vote", 1) if x.endswith("\t2\t4")]                                             # the two ties, decided at 50 %
    assert len(tie) == 2 and tie[0].split("\t")[3] == "1" and tie[1].split("\t")[3] == "1"                        # n = 1 before n = 2; of two strings of one base the smaller
    g, site = XC.plain(103, 1700), 150 + 170 * 2
    d = int(g[site])
    assert "ACGT".index(tie[1].split("\t")[5]) == min(d, d ^ 1 if (d ^ 1) != g[site - 1] and (d ^ 1) != g[site + 1] else d ^ 2)
    # adjacent
    w = XC.checked("adjacent")
    assert w["len"].tolist() == [320, 257] and XC.case("adjacent")["tlen"].tolist() == [324, 256]
    ev = list(zip(w["ev_col"].tolist(), w["ev_kind"].tolist()))
    assert ev[:3] == [(58, 2), (59, 2), (60, 2)] and (324 + 172, 1) in ev and (324 + 172) % 16 == 0 and (199, 0) in ev and (204, 2) in ev and 199 // 16 == 204 // 16
    assert int(w["col_off"][1]) == 320 and int(w["new_col"][324]) == 320
    # seams
    w, c = XC.checked("seams"), XC.case("seams")
    assert len(c["tlen"]) == 61 and int((c["tlen"] == 0).sum()) == 16 and [int(b) & 15 for b in c["tbegin"][:6]] == [0, 3, 6, 9, 12, 15]
    assert all(len(s) == len(t) and (s == t).all() for s, t in zip(IC.sequences(w), c["truths"])) and w["info"]["deleted"] == 14 and w["info"]["inserted_slots"] == 13
    assert (w["col_off"].astype(np.int64) != XC.placed("seams")[0]["col_off"].astype(np.int64)).any()
    # deep
    w = XC.checked("deep", 0, True)
    assert w["counts"][150, 4] == 300 and sorted(set(w["counts"].sum(axis=1).tolist()) & {255, 256, 300}) == [255, 256, 300]
    # no gapped voter: the polish
    c = XC.case("no_gapped")
    pl, gp = XC.placed("no_gapped")
    assert gp["info"]["unique"] == 0
    for i, v in enumerate(c["variants"]):
        w, po = XC.checked("no_gapped", i), PC.polish_scatter(c["rows"], c["lens"], pl, *XC.targets(c), **v)
        assert (w["words"] == po["words"]).all() and (w["ev_col"] == po["changed_cols"]).all() and (w["ev_bases"] == po["changed_bases"]).all()
    for name in ("no_voters", "no_reads", "no_targets"):
        w = XC.checked(name)
        assert len(w["ev_col"]) == 0 and w["info"]["columns_after"] == w["info"]["columns"] == int(XC.case(name)["tlen"].sum())


def test_a_deleted_column_beside_an_inserted_slot():
    """two read populations (tests/ipolish_cases.py: beside): `-` wins column g with 4 of 7, the slot before column g + 1 gets a base with 3 of 7"""
    c = XC.case("beside")
    g = c["g"]
    w = XC.checked("beside", 0, True)
    assert list(zip(w["ev_col"].tolist(), w["ev_kind"].tolist(), w["ev_votes"].tolist(), w["ev_cover"].tolist())) == [(g, IC.EV_D, 4, 7), (g + 1, IC.EV_I, 3, 7)]
    assert w["new_col"][g:g + 3].tolist() == [g, g, g + 2] and w["len"].tolist() == [400] and w["counts"][g].tolist().count(0) == 3
    w = XC.checked("beside", 1)                                                       # at 60 per cent neither passes: the column is ambiguous, the slot is not (3 of 7 votes)
    assert len(w["ev_col"]) == 0 and w["info"]["ambiguous_columns"] == 1 and w["info"]["ambiguous_slots"] == 0
    assert len(XC.checked("beside", 2)["ev_col"]) == 0 and XC.checked("beside", 2)["info"]["voted_columns"] == 0


def test_a_deleted_column_that_carries_an_insertion():
    """tests/ipolish_cases.py: carries: the slot before column g takes a base with 3 of 8 and column g leaves with 5 of 8: the insertion's event
    comes first, the old column's width is the inserted base alone"""
    c = XC.case("carries")
    g = c["g"]
    w = XC.checked("carries", 0)
    assert list(zip(w["ev_col"].tolist(), w["ev_kind"].tolist(), w["ev_votes"].tolist(), w["ev_cover"].tolist())) == [(g, IC.EV_I, 3, 8), (g, IC.EV_D, 5, 8)]
    assert w["new_col"][g:g + 2].tolist() == [g, g + 1] and w["len"].tolist() == [400] and g % 16 == 0
    w = XC.checked("carries", 1)                                                      # at 60 per cent only the column passes (5 of 8)
    assert w["ev_kind"].tolist() == [IC.EV_D] and w["len"].tolist() == [399] and w["info"]["ambiguous_slots"] == 0


def test_no_canonical_script_has_a_gap_behind_a_gap():
    """why `a gap directly behind another gap` is held on hand-made scripts only: with unit costs an I run next to a D run costs 2 where one
    substitution costs at most 1, so no optimal alignment holds the pair, and the gapped placement traces optimal parts joined by k M cells of
    the seed.  Every script of every case here and of the gapped placement's own cases bears it out"""
    import gapped_cases as QC
    scripts = [s for name in XC.CASES for s in GC.cigar_strings(XC.placed(name)[1]) if s]
    scripts += [s for name, i in QC.every() for s in GC.cigar_strings(QC.checked(name, i)) if s]
    assert len(scripts) > 500
    for s in scripts:
        ops = re.findall(r"[MID]", s)
        assert all(a == "M" or b == "M" for a, b in zip(ops, ops[1:])), s


def test_the_large_planted_set_is_what_its_planting_says():
    """tests/ipolish_cases.py: many, at 2 targets and 3 copies (default parameters) and 1 copy (min_cover 1, as the one-block test on the GPU
    runs it): the texts written from the planting alone are the checker's, on both statements"""
    for copies, kw in ((3, {}), (1, dict(min_cover=1))):
        m = XC.many(2, 10000, copies, 141)
        tw, tb, tl = m["targets"]
        pl = P.place(m["rows"], m["lens"], None, tw, tb, tl, **m["place"])
        gp = GC.gapped_banded(m["rows"], m["lens"], pl, tw, tb, tl)
        assert pl["info"]["unique"] == 2 * 199 * copies - 8 * copies and gp["info"]["unique"] == 8 * copies
        fa, tsv = XC.many_texts(m)
        for fn in (IC.ipolish_scatter, IC.ipolish_gather):
            r = fn(m["rows"], m["lens"], pl, gp, tw, tb, tl, **kw)
            assert IC.fasta(r) == fa and IC.events_tsv(r) == tsv
            assert all((s == t).all() for s, t in zip(IC.sequences(r), m["truths"])) and r["info"]["shifted_runs"] == 0


def _truth_normalise():
    g = XC.plain(101, 900)
    g[200:206], g[199], g[206] = 0, 1, 2
    g[400:406], g[399], g[406] = 3, 0, 1
    g[600:608], g[599], g[608] = [0, 1] * 4, 2, 2
    g[752:758], g[751], g[758] = 2, 1, 3
    return g


def test_planted_set_on_the_checker():
    """the condition of the planted set on the checker alone, default parameters: the new target is the genome; both statements"""
    seed, c, g, pl, gp, res = XC.planted()
    print("seed", seed, res["info"])
    seq = IC.sequences(res)[0]
    assert len(seq) == len(g) == 6000 and (seq == g).all() and len(c["lens"]) // 2 == 1800
    assert res["info"]["substituted"] == 2 and res["info"]["deleted"] >= 5 and res["info"]["inserted_bases"] >= 5 and res["info"]["shifted_runs"] > 0
    assert_same(IC.ipolish_gather(c["rows"], c["lens"], pl, gp, *XC.targets(c)), res, "planted")
    tw, tb, tl = IC.targets_of(res)                                                   # a second round: every read exact, nothing left to do
    pl2 = P.place(c["rows"], c["lens"], None, tw, tb, tl, **c["place"])
    assert pl2["info"]["placed"] == 1800 and int(pl2["mm"].max()) == 0


def test_refusals_of_the_checker():
    c = XC.case("normalise")
    pl, gp = XC.placed("normalise")
    for fn in (IC.ipolish_scatter, IC.ipolish_gather):
        for kw in (dict(min_cover=0), dict(min_cover=2 ** 31), dict(min_percent=0), dict(min_percent=101), dict(max_ins=0), dict(max_ins=14), dict(flags=2), dict(reserved=1)):
            with pytest.raises(ValueError):
                fn(c["rows"], c["lens"], pl, gp, *XC.targets(c), **kw)
        fn(c["rows"], c["lens"], pl, gp, *XC.targets(c), min_cover=2 ** 31 - 1, min_percent=100, max_ins=13, flags=1)       # the bounds themselves are taken
        fn(c["rows"], c["lens"], pl, gp, *XC.targets(c), min_cover=1, min_percent=1, max_ins=1)
        with pytest.raises(ValueError):
            fn(c["rows"][:-2], c["lens"][:-2], pl, gp, *XC.targets(c))
        with pytest.raises(ValueError):
            fn(c["rows"], c["lens"], pl, XC.placed("ties")[1], *XC.targets(c))      # a gapped result of another placement
        rows = c["rows"].copy()
        rows[0, 0] ^= 1
        with pytest.raises(ValueError):
            fn(rows, c["lens"], pl, gp, *XC.targets(c))
        r = int(np.nonzero(gp["state"] & GC.UNIQUE)[0][0])
        for key, delta in (("end", 1), ("pos", -200), ("cigar", 4)):
            bad = dict(gp)
            bad[key] = gp[key].copy()
            bad[key][int(gp["cigar_off"][r]) if key == "cigar" else r] += delta
            with pytest.raises(ValueError):
                fn(c["rows"], c["lens"], pl, bad, *XC.targets(c))


def test_library_exports_the_calls_and_the_header_declares_them():
    lib = alga_amd.load_library()
    header = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in alga_amd.engine.EXPORTS
        assert re.search(r"^(void|int)\s+%s\(" % sym, header, re.M), sym
    assert lib.alga_abi_version() == 7                                       # the calls only add to the ABI
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} alga_ipolish_params;", header)
    assert m and re.findall(r"\b([a-z_0-9]+)(?:\[4\])?[,;]", strip(m.group(1))) == [k for k, _ in alga_amd.IpolishParams._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} alga_ipolish_info;", header)
    assert m and re.findall(r"\b([a-z_0-9]+)[,;]", strip(m.group(1))) == [k for k, _ in alga_amd.IpolishInfo._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} alga_ipolished;", header)
    assert m and [x.lstrip("*") for x in re.findall(r"(\*?\b[a-z_0-9]+)[,;]", strip(m.group(1)))] == [k for k, _ in alga_amd.IpolishedC._fields_]
    p = alga_amd.IpolishParams()
    lib.alga_ipolish_default_params(C.byref(p))
    assert {k: getattr(p, k) for k in IC.DEFAULT} == IC.DEFAULT == dict(min_cover=3, min_percent=60, max_ins=6) and p.flags == 0 and list(p.reserved) == [0] * 4
    assert C.sizeof(alga_amd.IpolishParams) == 32 and C.sizeof(alga_amd.IpolishInfo) == 8 * (19 + 4) and C.sizeof(alga_amd.IpolishedC) == 8 * (4 + 17)
    assert [k for k, _ in alga_amd.IpolishInfo._fields_][:19] == list(IC.COUNTERS) and [k for k, _, _, _ in alga_amd.IndelPolished.KEYS] == list(IC.ARRAYS)
    E = alga_amd.engine
    assert E.IPOLISH_COUNTS == IC.COUNTS == 1 and E.IPOLISH_MAX_INS == IC.MAX_INS == 13 and (E.EVENT_S, E.EVENT_I, E.EVENT_D) == (IC.EV_S, IC.EV_I, IC.EV_D) == (0, 1, 2)
    for name, value in (("IPOLISH_COUNTS", 1), ("IPOLISH_MAX_INS", 13)):
        assert re.search(r"#define ALGA_%s\s+%d\b" % (name, value), header), name
    for fn in (alga_amd.Engine.polish_indels, alga_amd.Engine.write_ipolished_fasta, alga_amd.Engine.write_ipolish_events_tsv, alga_amd.IndelPolished.to_host):
        assert callable(fn)
    assert isinstance(alga_amd.IndelPolished.targets, property)
    binary = open(alga_amd.library_path(), "rb").read()
    for k in KERNELS:
        assert k.encode() in binary


def test_new_kernels_resources():
    """The compiler's resource report of ipolish_kernels.hip: every k_ip_* is there, no VGPR spill and no scratch in any of them"""
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_ipolish_resources_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    src = os.path.join(ROOT, "alga_amd", "csrc", "ipolish_kernels.hip")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    finally:
        if os.path.exists(out):
            os.remove(out)
    lines = r.stderr.splitlines()
    reps = {}
    for i, s in enumerate(lines):
        m = re.search(r"Function Name: \S*?(k_ip_[a-z_]+)E", s)
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
    print({k: (v["VGPRs"], v["Occupancy [waves/SIMD]"], v["LDS Size [bytes/block]"]) for k, v in reps.items()})
