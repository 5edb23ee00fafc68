"""The grow stage without a GPU: the two Python statements of the definition (tests/grow_checker.py) agree on the cases of
tests/grow_cases.py, the outcomes the cases were made for, the planted genome; the refusals of the checker; the library exports the calls
and the header declares them; the compiler's resource report of grow_kernels.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import grow_cases as QC
import grow_checker as GC
import place_checker as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_gr_check", "k_gr_candidates", "k_gr_compact", "k_gr_end_lens", "k_gr_ends", "k_gr_place", "k_gr_vote", "k_gr_decide", "k_gr_lens", "k_gr_build",
           "k_gr_fasta_sizes", "k_gr_fasta_write"]
SYMBOLS = ("alga_grow_default_params", "alga_grow_placed_device", "alga_write_grown_fasta_device")
# (candidates, overhanging, voting, bases_added) of every variant of every case
OUTCOMES = {"word_seams": [(10, 10, 10, 172)], "h_extremes": [(6, 4, 4, 74)], "a_equals_w": [(4, 3, 3, 60)], "partial_word": [(5, 5, 5, 36)], "mm_bound": [(5, 3, 3, 60)], "tiny_targets": [(5, 3, 3, 104)],
            "period3": [(2, 2, 1, 30)], "equal_ends": [(2, 2, 0, 0), (2, 0, 0, 0)], "second_chunk": [(4, 3, 3, 10), (4, 1, 1, 10)],
            "cover": [(3, 3, 3, 10), (3, 3, 3, 20), (3, 3, 3, 8)], "percent": [(5, 5, 5, 8), (5, 5, 5, 5), (5, 5, 5, 30)], "minus_only": [(3, 3, 3, 20)],
            "left_grow": [(3, 3, 3, 20)], "both_ends": [(6, 6, 6, 20)], "n0": [(0, 0, 0, 0)], "t0": [(1, 0, 0, 0)], "all_placed": [(0, 0, 0, 0)]}


def assert_same(got, want, what=""):
    for k in GC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    assert got["info"] == want["info"], (what, got["info"], want["info"])


@pytest.mark.parametrize("name,i", QC.every())
def test_the_two_statements_agree(name, i):
    c, pl, want = QC.case(name), QC.placed(name), QC.checked(name, i)
    v = c["variants"][i]
    got = GC.grow_bruteforce(c["rows"], c["lens"], pl, c["seqs"], **v)
    assert_same(got, want, (name, i))
    info = want["info"]
    assert (info["candidates"], info["overhanging"], info["voting"], info["bases_added"]) == OUTCOMES[name][i], info
    # what holds for every result
    T, R = len(c["tlen"]), len(c["lens"]) // 2
    G = dict(GC.DEFAULT, **v)["max_grow"]
    assert info["candidates"] >= info["overhanging"] >= info["voting"] and info["multi"] == info["overhanging"] - info["voting"]
    assert info["stops_cover"] + info["stops_percent"] + info["stops_max"] == 2 * T and info["columns_before"] == int(c["tlen"].sum())
    assert info["columns_after"] == info["columns_before"] + info["bases_added"] == int(want["col_off"][-1]) and int(want["e_voters"].sum()) == info["voting"]
    assert ((want["end"] >= 0) == (want["state"] & GC.OVERHANGS > 0)).all() and ((want["over"] > 0) == (want["end"] >= 0)).all() and len(want["end"]) == R
    assert ((want["state"] & GC.VOTES > 0) == (want["hits"] == 1)).all() and (want["left"] <= G).all() and (want["right"] <= G).all()
    assert (want["len"] == c["tlen"] + want["left"].astype(np.int64) + want["right"]).all() and (want["begin"] == want["col_off"][:-1]).all()
    assert (want["left"][c["tlen"] < dict(GC.DEFAULT, **v)["min_anchor"]] == 0).all() and (want["right"][c["tlen"] < dict(GC.DEFAULT, **v)["min_anchor"]] == 0).all()
    assert (want["count"].reshape(2 * T, G, 4).sum(axis=(1, 2)) == [int(np.minimum(want["over"][(want["end"] == e) & (want["hits"] == 1)], G).sum()) for e in range(2 * T)]).all()
    new = GC.sequences(want)
    for t in range(T):                                                          # the old target lies at `left` in the new one
        assert (new[t][int(want["left"][t]):int(want["left"][t]) + int(c["tlen"][t])] == c["seqs"][t]).all()
    # the rendered FASTA: one record per target with a length; the growth as text
    text = GC.fasta(want).decode().split("\n")
    assert text[-1] == "" and [len(s) for s in text[1::2]] == [int(n) for n in want["len"] if n > 0]
    assert len(GC.grow_tsv(want).decode().splitlines()) == T
    print(name, i, info)


def test_every_case_is_listed():
    assert sorted(OUTCOMES) == sorted(QC.CASES) and all(len(OUTCOMES[n]) == len(QC.case(n)["variants"]) for n in QC.CASES)


def grown_window(name, i, t):
    """the window of the case's genome that grown target t should be"""
    c, w = QC.case(name), QC.checked(name, i)
    return w, GC.sequences(w)[t]


def test_outcomes_the_cases_were_made_for():
    # h = 1 and h = L - min_anchor are placed, h = L - min_anchor + 1 is not; a forward read at a left end is the `-` strand of the mirrored end
    w, s = grown_window("h_extremes", 0, 0)
    assert w["over"].tolist() == [1, 37, 0, 1, 37, 0] and w["end"].tolist() == [1, 1, -1, 0, 0, -1] and w["state"].tolist() == [3, 3, 0, 7, 7, 0]
    assert (s == QC.case("h_extremes")["g"][163:537]).all()
    # a = W = the whole target of 80 bases, at both of its ends; one base more does not exist
    w, s = grown_window("a_equals_w", 0, 0)
    assert w["over"].tolist() == [20, 0, 20, 20] and w["end"].tolist() == [1, -1, 0, 3] and w["state"].tolist() == [3, 0, 3, 3]
    assert (s == QC.case("a_equals_w")["g"][80:200]).all() and w["len"].tolist() == [120, 420]
    # every a mod 16 with mm at the bound: the last partial word is masked
    w, s = grown_window("partial_word", 0, 0)
    assert w["over"].tolist() == [100 - a for a in QC.PARTIAL_A] and w["mm"].tolist() == [2] * 5 and sorted(a % 16 for a in QC.PARTIAL_A) == [0, 0, 1, 1, 15]
    assert (s == QC.case("partial_word")["g"][100:536]).all()
    # mm 2 is placed and 3 is not; the first overhanging base, which differs from what lies behind the end, does not count
    w = QC.checked("mm_bound", 0)
    assert w["mm"].tolist() == [2, 0, 2, 2, 0] and w["over"].tolist() == [30, 0, 30, 30, 0] and w["end"].tolist() == [1, -1, 1, 2, -1]
    # targets of 0 and 62 bases never grow, the one of 63 grows at both ends
    w, s = grown_window("tiny_targets", 0, 3)
    assert w["left"].tolist() == [0, 0, 0, 37, 0] and w["right"].tolist() == [0, 0, 0, 37, 30] and w["len"].tolist() == [300, 0, 62, 137, 330]
    assert (s == QC.case("tiny_targets")["g"][463:600]).all() and (QC.case("tiny_targets")["tbegin"][1:4] == QC.case("tiny_targets")["tbegin"][:3] + [300, 0, 62]).all()
    # ten placements at mm 0: the smallest h is the best, nobody votes there
    w = QC.checked("period3", 0)
    assert (w["end"][0], w["over"][0], w["hits"][0], w["state"][0]) == (1, 10, 10, GC.OVERHANGS) and w["e_voters"].tolist() == [0, 0, 0, 1]
    # a tie across two ends; every seed over max_occ
    w = QC.checked("equal_ends", 0)
    assert w["end"].tolist() == [1, 1] and w["hits"].tolist() == [2, 2] and w["state"].tolist() == [GC.OVERHANGS, GC.OVERHANGS | GC.MINUS] and w["info"]["multi"] == 2
    w = QC.checked("equal_ends", 1)
    assert w["info"]["seeds_over_max_occ"] == 6 and w["info"]["overhanging"] == 0
    # found only through seeds 64 and 65
    w = QC.checked("second_chunk", 0)
    assert w["mm"].tolist() == [0, 64, 64, 0] and w["state"].tolist() == [3, 3, 7, 0] and w["info"]["seeds"] == 4 * 2 * 66
    assert QC.checked("second_chunk", 1)["end"].tolist() == [1, -1, -1, -1]
    # cover 3 -> 2 stops the growth at min_cover 3, 2 -> 1 at 2; max_grow cuts it (stop reason 2)
    assert [(int(QC.checked("cover", i)["right"][0]), int(QC.checked("cover", i)["e_stop"][1])) for i in range(3)] == [(10, 0), (20, 0), (8, 2)]
    # 4 of 5 passes at 80 %, 3 of 5 does not (stop reason 1); at 81 % column 5 stops it, at 60 % nothing does
    assert [(int(QC.checked("percent", i)["right"][0]), int(QC.checked("percent", i)["e_stop"][1])) for i in range(3)] == [(8, 1), (5, 1), (30, 0)]
    w = QC.checked("percent", 0)
    assert sorted(w["count"].reshape(2, 64, 4)[1, 5].tolist()) == [0, 0, 1, 4] and sorted(w["count"].reshape(2, 64, 4)[1, 8].tolist())[-1] == 3
    # voters of the minus strand only; growth at a left end: the reverse complement in the words
    w, s = grown_window("minus_only", 0, 0)
    assert w["state"].tolist() == [7, 7, 7] and (s == QC.case("minus_only")["g"][100:420]).all()
    w, s = grown_window("left_grow", 0, 0)
    assert w["left"].tolist() == [20] and w["state"].tolist() == [7, 7, 3] and (s == QC.case("left_grow")["g"][80:400]).all()
    w, s = grown_window("both_ends", 0, 0)
    assert (w["left"].tolist(), w["right"].tolist()) == ([10], [10]) and (s == QC.case("both_ends")["g"][90:180]).all()
    assert QC.placed("all_placed")["info"]["placed"] == 10 and QC.checked("t0")["words"].tolist() == [0, 0]


def test_planted_genome():
    """the checker's place -> grow loop on two contigs of a 3 kb genome with a gap of 120 between them: every grown base is the genome's in every
    round, round 1 adds at least 10 bases at each of the four ends, the inner ends overlap after at most four rounds, and an error-free read
    that lies inside a contig is placed and so never a candidate"""
    c, g, meta = QC.planted()
    lo, hi = [s for s, _ in QC.PLANTED_BOUNDS], [e for _, e in QC.PLANTED_BOUNDS]
    rounds = []
    for rnd in range(1, 5):
        pl = P.place(*QC.place_args(c))
        w = GC.grow_index(c["rows"], c["lens"], pl, c["seqs"])
        if rnd == 1:
            assert_same(GC.grow_bruteforce(c["rows"], c["lens"], pl, c["seqs"]), w, "planted, round 1")
            assert min(w["left"].tolist() + w["right"].tolist()) >= 10
        for r, (a, clean) in enumerate(meta):
            if clean and any(lo[t] <= a and a + 100 <= hi[t] for t in range(2)):
                assert pl["state"][r] & P.PLACED and w["end"][r] == -1, (rnd, r)
        lo = [lo[t] - int(w["left"][t]) for t in range(2)]
        hi = [hi[t] + int(w["right"][t]) for t in range(2)]
        assert min(lo) >= 0 and max(hi) <= len(g)
        for t, s in enumerate(GC.sequences(w)):
            assert (s == g[lo[t]:hi[t]]).all(), (rnd, t)
        rounds.append((w["left"].tolist(), w["right"].tolist(), w["info"]["candidates"], w["info"]["voting"]))
        c = QC.next_round(c, w)
        if hi[0] > lo[1]:
            break
    print(rounds)
    assert hi[0] > lo[1] and rounds == PLANTED_PINNED


PLANTED_PINNED = [([30, 29], [32, 34], 133, 56), ([9, 30], [34, 8], 80, 38)]   # (left, right, candidates, voting) per round, from the checker


def test_refusals_of_the_checker():
    c, pl = QC.case("cover"), QC.placed("cover")
    args = (c["rows"], c["lens"], pl, c["seqs"])
    bad = (dict(k=7), dict(k=32), dict(max_mismatches=-1), dict(max_mismatches=255), dict(max_occ=0), dict(max_occ=65536), dict(min_anchor=20), dict(min_anchor=2 ** 20 + 1),
           dict(min_cover=0), dict(min_cover=2 ** 31), dict(min_percent=50), dict(min_percent=101), dict(max_grow=0), dict(max_grow=4097))
    for fn in (GC.grow_index, GC.grow_bruteforce):
        for kw in bad:
            with pytest.raises(ValueError):
                fn(*args, **kw)
        with pytest.raises(ValueError):
            fn(c["rows"][:-2], c["lens"][:-2], pl, c["seqs"])                     # n / 2 != the placement's reads
        with pytest.raises(ValueError):
            fn(c["rows"], c["lens"], pl, [c["seqs"][0][:-1]])                     # not the placement's columns
        odd = c["lens"].copy()
        odd[0] = 99
        with pytest.raises(ValueError):
            fn(c["rows"], odd, pl, c["seqs"])                                     # twin lengths
        flipped = c["rows"].copy()
        flipped[0, 0] ^= 1
        with pytest.raises(ValueError):
            fn(flipped, c["lens"], pl, c["seqs"])                                 # not the reverse complement
        long_ = c["lens"].copy()
        long_[0] = long_[1] = 16 * c["rows"].shape[1] + 1
        with pytest.raises(ValueError):
            fn(c["rows"], long_, pl, c["seqs"])


def test_library_exports_the_calls_and_the_header_declares_them():
    lib = alga_amd.load_library()
    header = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in alga_amd.engine.EXPORTS
        assert re.search(r"^(void|int)\s+%s\(" % sym, header, re.M), sym
    assert lib.alga_abi_version() == 7                                       # the calls only add to the ABI
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} alga_grow_params;", header)
    assert m and re.findall(r"\b([a-z_0-9]+)(?:\[4\])?[,;]", strip(m.group(1))) == [k for k, _ in alga_amd.GrowParams._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} alga_grow_info;", header)
    assert m and re.findall(r"\b([a-z_0-9]+)[,;]", strip(m.group(1))) == [k for k, _ in alga_amd.GrowInfo._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} alga_grown;", header)
    assert m and [x.lstrip("*") for x in re.findall(r"(\*?\b[a-z_0-9]+)[,;]", strip(m.group(1)))] == [k for k, _ in alga_amd.GrownC._fields_]
    p = alga_amd.GrowParams()
    lib.alga_grow_default_params(C.byref(p))
    got = {k: getattr(p, k) for k in GC.DEFAULT}
    assert got == GC.DEFAULT == dict(k=21, max_mismatches=2, max_occ=256, min_anchor=63, min_cover=3, min_percent=80, max_grow=64) and p.flags == 0 and list(p.reserved) == [0] * 4
    assert p.min_anchor == p.k * (p.max_mismatches + 1)
    assert C.sizeof(alga_amd.GrowParams) == 48 and C.sizeof(alga_amd.GrowInfo) == 8 * (19 + 4) and C.sizeof(alga_amd.GrownC) == 8 * (4 + 14)
    assert [k for k, _ in alga_amd.GrowInfo._fields_][:19] == list(GC.COUNTERS) and [k for k, _, _, _ in alga_amd.Grown.KEYS] == list(GC.ARRAYS)
    assert (alga_amd.engine.GROW_OVERHANGS, alga_amd.engine.GROW_VOTES, alga_amd.engine.GROW_MINUS) == (GC.OVERHANGS, GC.VOTES, GC.MINUS) == (1, 2, 4)
    for name, value in (("OVERHANGS", 1), ("VOTES", 2), ("MINUS", 4)):
        assert re.search(r"#define ALGA_GROW_%s\s+%d\b" % (name, value), header)
    for fn in (alga_amd.Engine.grow_ends, alga_amd.Engine.write_grown_fasta, alga_amd.Grown.to_host, alga_amd.Grown.targets, alga_amd.Grown.grow_tsv):
        assert callable(fn)
    for name in ("tiny_targets", "percent", "t0", "both_ends"):
        assert alga_amd.engine.grow_tsv(QC.checked(name)).encode() == GC.grow_tsv(QC.checked(name))
    binary = open(alga_amd.library_path(), "rb").read()
    for k in KERNELS:
        assert k.encode() in binary


def test_new_kernels_resources():
    """The compiler's resource report of grow_kernels.hip: every k_gr_* is there, no VGPR spill and no scratch in any of them"""
    src = os.path.join(ROOT, "alga_amd", "csrc", "grow_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_grow_resources_%d.o" % os.getpid())
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
        m = re.search(r"Function Name: \S*?(k_gr_[a-z_]+)E", s)
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
