"""The gapped placement without a GPU: the two Python statements of the definition (tests/gapped_checker.py) agree on the cases of
tests/gapped_cases.py, the outcomes the cases were made for, banded tables equal full ones, the planted set; the refusals of the checker; the
library exports the calls and the header declares them; the compiler's resource report of gapped_kernels.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import gapped_cases as QC
import gapped_checker as GC
import gapped_invariants as GI
import place_checker as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_gp_target_check", "k_gp_flag", "k_gp_scatter", "k_gp_score", "k_gp_trace", "k_gp_cigar", "k_gp_depth_add", "k_gp_cover", "k_gp_tsv_sizes", "k_gp_tsv_write"]
SYMBOLS = ("alga_gapped_default_params", "alga_place_gapped_device", "alga_write_gapped_tsv_device")
# (tried, placed, unique, with_indel, edits) of every variant of every case
OUTCOMES = {"indel_positions": [(12, 12, 12, 12, 32), (12, 12, 12, 12, 32)], "homopolymer": [(4, 4, 4, 4, 4)], "edit_bound": [(18, 3, 3, 2, 3), (18, 9, 9, 6, 18), (18, 15, 15, 10, 75)],
            "cigar_runs": [(2, 2, 2, 2, 6), (2, 0, 0, 0, 0)], "overhang": [(7, 5, 5, 5, 10)], "seams": [(3, 3, 3, 3, 3), (3, 3, 3, 3, 3)], "uniqueness": [(3, 3, 1, 3, 3)],
            "read_lengths": [(5, 5, 5, 5, 5), (5, 5, 5, 5, 5)], "participation": [(2, 0, 0, 0, 0), (2, 1, 0, 0, 0)], "empty_pass": [(0, 0, 0, 0, 0)], "no_reads": [(0, 0, 0, 0, 0)],
            "no_targets": [(2, 0, 0, 0, 0)], "short_targets": [(2, 0, 0, 0, 0)]}


def assert_same(got, want, what=""):
    for k in GC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    assert got["info"] == want["info"], (what, got["info"], want["info"])


@pytest.mark.parametrize("name,i", QC.every())
def test_the_two_statements_agree(name, i):
    c, want, pl = QC.case(name), QC.checked(name, i), QC.placed(name)
    v = dict(GC.DEFAULT, **c["variants"][i])
    assert_same(GC.gapped_full(c["rows"], c["lens"], pl, *QC.targets(c), **c["variants"][i]), want, (name, i))
    info = want["info"]
    assert (info["tried"], info["placed"], info["unique"], info["with_indel"], info["edits"]) == OUTCOMES[name][i], info
    GI.assert_invariants(c, pl, want, v)
    print(name, i, info)


def test_every_case_is_listed():
    assert sorted(OUTCOMES) == sorted(QC.CASES) and all(len(OUTCOMES[n]) == len(QC.case(n)["variants"]) for n in QC.CASES)


def test_outcomes_the_cases_were_made_for():
    cg = lambda name, i=0: GC.cigar_strings(QC.checked(name, i))
    # one deleted / inserted base inside seed 0, inside the last seed, on a seed boundary, in the last L mod k bases, next to the only exact seed
    w = QC.checked("indel_positions")
    assert cg("indel_positions") == ["11M1D139M", "10M1I139M", "135M1D15M", "135M1I14M", "42M1D108M", "42M1I107M", "147M1D3M", "147M1I2M", "62M1D88M", "62M1I87M",
                                     "85M1D65M", "84M1I65M"]
    assert (w["pos"] == 100).all() and w["edits"].tolist() == [1] * 8 + [6] * 4 and (w["state"] == 11).all() and w["info"]["candidates"] == 15
    assert QC.placed("indel_positions")["info"]["placed"] == 0
    # the canonical script puts the indel at the first base of the run of six; the minus strand mirrors the read, not the script
    w = QC.checked("homopolymer")
    assert cg("homopolymer") == ["60M1D80M", "60M1I79M"] * 2 and w["state"].tolist() == [11, 11, 15, 15] and (w["pos"] == 80).all()
    # E edits are placed and E + 1 are not, as substitutions and as one run of deleted or inserted bases
    for i, E in enumerate((1, 3, 15)):
        w = QC.checked("edit_bound", i)
        want = [n <= E for n in (1, 2, 3, 4, 15, 16) for _ in range(3)]
        assert ((w["state"] & GC.PLACED) > 0).tolist() == want and [int(x) for x in w["edits"][want]] == [n for n in (1, 2, 3, 4, 15, 16) for _ in range(3) if n <= E]
    assert cg("edit_bound", 2)[12] == "150M" and max(len(re.findall(r"[MID]", s)) for s in cg("edit_bound", 2)) <= 31
    # 2 E + 1 runs
    assert cg("cigar_runs") == ["30M1D26M1I43M1D49M", "25M1I50M1D47M1I27M"] and cg("cigar_runs", 1) == ["", ""]
    # over the first and the last column by 1 and by E: insertions at the edge; by E + 1: not placed; a target shorter than the read
    w = QC.checked("overhang")
    assert cg("overhang") == ["1I99M", "99M1I", "3I97M", "97M3I", "", "", "1I98M1I"] and w["pos"].tolist() == [0, 201, 0, 203, -1, -1, 0]
    assert w["end"].tolist() == [99, 300, 97, 300, -1, -1, 98] and w["target"].tolist() == [0, 0, 0, 0, -1, -1, 1]
    # nothing is laid across the seam of targets 0 and 1 (column 200, inside a word); the reads lie on target 4, behind two empty targets
    w, c = QC.checked("seams"), QC.case("seams")
    assert c["tlen"].tolist() == [200, 200, 0, 0, 390] and int(c["tbegin"][1]) == int(c["tbegin"][0]) + 200 and int(c["tbegin"][1]) & 15 == 8
    assert w["target"].tolist() == [4, 4, 4] and w["pos"].tolist() == [145, 189, 115] and cg("seams") == ["20M1D80M", "60M1D40M", "29M1I72M"] and w["info"]["candidates"] == 11
    # two loci; one locus on two diagonals; both strands
    w = QC.checked("uniqueness")
    assert w["state"].tolist() == [9, 11, 9] and w["target"].tolist() == [0, 1, 2] and w["pos"].tolist() == [20, 0, 60] and w["info"]["candidates"] == 10
    assert w["t_reads"].tolist() == [0, 1, 0] and w["t_bases"].tolist() == [0, 121, 0] and w["t_edits"].tolist() == [0, 1, 0]
    # the block and word edges, the cap, two chunks of seeds
    for i in range(2):
        w = QC.checked("read_lengths", i)
        assert cg("read_lengths", i) == ["32M1D32M", "32M1D33M", "64M1D64M", "64M1D65M", "500M1D524M", ""] and w["info"]["skipped_long"] == 1 and w["info"]["tried"] == 5
    assert QC.case("read_lengths")["lens"][1::2].tolist() == [64, 65, 128, 129, GC.MAX_READ, GC.MAX_READ + 1] and QC.checked("read_lengths", 1)["info"]["seeds"] == 2 * (8 + 8 + 16 + 16 + 128)
    # who takes part
    pl, w = QC.placed("participation"), QC.checked("participation")
    assert pl["state"].tolist() == [3, 0, 0, 0, 3] and pl["mm"][0] == 2 and pl["target"][0] == 0                     # a gapped placement with one edit lies on target 1
    assert (w["state"] == 0).all() and w["info"]["tried"] == 2 and w["info"]["seeds_over_max_occ"] == 4 and w["info"]["candidates"] == 0
    w1 = QC.checked("participation", 1)
    assert w1["state"].tolist() == [0, 0, 1, 0, 0] and w1["info"]["seeds_over_max_occ"] == 0 and (w1["cover"] == pl["cover"]).all()
    w, pl = QC.checked("empty_pass"), QC.placed("empty_pass")
    assert pl["info"]["placed"] == 2 and (w["target"] == -1).all() and (w["cover"] == pl["cover"]).all() and w["cigar_off"].tolist() == [0] * 4 and len(w["cigar"]) == 0
    assert QC.checked("no_reads")["cigar_off"].tolist() == [0]
    for name, columns in (("no_targets", 0), ("short_targets", 30)):
        w = QC.checked(name)
        assert len(w["cover"]) == columns and w["info"]["seeds"] == 2 * (4 + 2) and w["info"]["candidates"] == 0 and (w["state"] == 0).all()


def test_banded_equals_full():
    """rule 5 of the definition on both parts of every candidate of every case: inside the band a value <= E is the full table's, the trace stays
    on cells <= E, the end and the script are the same"""
    parts = 0
    for name, i in QC.every():
        c, pl = QC.case(name), QC.placed(name)
        v = dict(GC.DEFAULT, **c["variants"][i])
        k, E = v["k"], v["max_edits"]
        index = P._index(c["seqs"], k)
        for r in range(len(c["lens"]) // 2):
            L = int(c["lens"][2 * r + 1])
            if not GC.takes_part(pl, c["lens"], r, k) or L > 200:
                continue
            for node in (2 * r + 1, 2 * r):
                codes = P.codes_of(c["rows"][node], 0, L)
                for j, x in enumerate(P.kmer_values(codes, k)[::k][:L // k]):
                    for t, q in index.get(int(x), ())[:4]:
                        tc = c["seqs"][t]
                        GC.banded_equals_full(codes[j * k + k:], tc[q + k:], E)
                        GC.banded_equals_full(codes[:j * k][::-1], tc[:q][::-1], E)
                        parts += 2
    assert parts > 500
    rng = np.random.default_rng(5)
    for E in (1, 2, 6, 15):                                                       # and on parts that share nothing
        for _ in range(20):
            GC.banded_equals_full(rng.integers(0, 4, size=int(rng.integers(0, 40)), dtype=np.uint8), rng.integers(0, 4, size=int(rng.integers(0, 60)), dtype=np.uint8), E)


def test_planted_set():
    """a 6 kb genome, 30x reads of 100 nt with one planted 1-base indel each: every read that keeps a seed whose k-mer is unique in the genome comes
    back UNIQUE at its true locus and strand, its start within E of the true one"""
    c, start, minus = QC.planted()
    pl = P.place(c["rows"], c["lens"], None, *QC.targets(c), **c["place"])
    w = GC.gapped_banded(c["rows"], c["lens"], pl, *QC.targets(c))
    E, k = GC.DEFAULT["max_edits"], GC.DEFAULT["k"]
    occ = {x: len(v) for x, v in P._index(c["seqs"], k).items()}
    held = 0
    for r in range(len(start)):
        if pl["state"][r] & P.PLACED:
            continue
        seeds = [int(x) for node in (2 * r + 1, 2 * r) for x in P.kmer_values(P.codes_of(c["rows"][node], 0, int(c["lens"][node])), k)[::k]]
        if any(occ.get(x, 0) == 1 for x in seeds):
            held += 1
            assert w["state"][r] & GC.UNIQUE and w["target"][r] == 0 and bool(w["state"][r] & GC.MINUS) == bool(minus[r]) and abs(int(w["pos"][r]) - int(start[r])) <= E, r
    print(w["info"], held)
    assert held > 1700 and w["info"]["placed"] >= held and w["info"]["with_indel"] > 1500


def test_refusals_of_the_checker():
    c, pl = QC.case("homopolymer"), QC.placed("homopolymer")
    for fn in (GC.gapped_banded, GC.gapped_full):
        for kw in (dict(k=7), dict(k=32), dict(max_edits=0), dict(max_edits=16), dict(max_occ=0), dict(max_occ=65536), dict(flags=1)):
            with pytest.raises(ValueError):
                fn(c["rows"], c["lens"], pl, *QC.targets(c), **kw)
        fn(c["rows"], c["lens"], pl, *QC.targets(c), k=8, max_edits=1, max_occ=1)       # the bounds themselves are taken
        fn(c["rows"], c["lens"], pl, *QC.targets(c), k=31, max_edits=15, max_occ=65535)
        other = QC.placed("overhang")                                               # a placement of other reads on other targets
        with pytest.raises(ValueError):
            fn(c["rows"], c["lens"], other, *QC.targets(c))
        shorter = c["tlen"].copy()
        shorter[0] -= 1
        with pytest.raises(ValueError):
            fn(c["rows"], c["lens"], pl, c["twords"], c["tbegin"], shorter)
        rows = c["rows"].copy()
        rows[0, 0] ^= 1
        with pytest.raises(ValueError):
            fn(rows, c["lens"], pl, *QC.targets(c))


def test_library_exports_the_calls_and_the_header_declares_them():
    lib = alga_amd.load_library()
    header = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in alga_amd.engine.EXPORTS
        assert re.search(r"^(void|int)\s+%s\(" % sym, header, re.M), sym
    assert lib.alga_abi_version() == 7                                       # the calls only add to the ABI
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} alga_gapped_params;", header)
    assert m and re.findall(r"\b([a-z_0-9]+)(?:\[4\])?[,;]", strip(m.group(1))) == [k for k, _ in alga_amd.GappedParams._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} alga_gapped_info;", header)
    assert m and re.findall(r"\b([a-z_0-9]+)[,;]", strip(m.group(1))) == [k for k, _ in alga_amd.GappedInfo._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} alga_gapped;", header)
    assert m and [x.lstrip("*") for x in re.findall(r"(\*?\b[a-z_0-9]+)[,;]", strip(m.group(1)))] == [k for k, _ in alga_amd.GappedC._fields_]
    p = alga_amd.GappedParams()
    lib.alga_gapped_default_params(C.byref(p))
    assert {k: getattr(p, k) for k in GC.DEFAULT} == GC.DEFAULT == dict(k=21, max_edits=6, max_occ=256) and p.flags == 0 and list(p.reserved) == [0] * 4
    assert C.sizeof(alga_amd.GappedParams) == 32 and C.sizeof(alga_amd.GappedInfo) == 8 * (11 + 5) and C.sizeof(alga_amd.GappedC) == 8 * (4 + 11)
    assert [k for k, _ in alga_amd.GappedInfo._fields_][:11] == list(GC.COUNTERS) and [k for k, _, _, _ in alga_amd.Gapped.KEYS] == list(GC.ARRAYS)
    E = alga_amd.engine
    assert (E.GAPPED_PLACED, E.GAPPED_UNIQUE, E.GAPPED_MINUS, E.GAPPED_INDEL) == (GC.PLACED, GC.UNIQUE, GC.MINUS, GC.INDEL) == (1, 2, 4, 8)
    assert (E.CIGAR_M, E.CIGAR_I, E.CIGAR_D) == (GC.OP_M, GC.OP_I, GC.OP_D) == (0, 1, 2) and E.GAPPED_MAX_READ == GC.MAX_READ >= 1024
    for name, value in (("GAPPED_PLACED", 1), ("GAPPED_UNIQUE", 2), ("GAPPED_MINUS", 4), ("GAPPED_INDEL", 8), ("CIGAR_M", 0), ("CIGAR_I", 1), ("CIGAR_D", 2),
                        ("GAPPED_MAX_READ", GC.MAX_READ)):
        assert re.search(r"#define ALGA_%s\s+%d\b" % (name, value), header), name
    for fn in (alga_amd.Engine.place_gapped, alga_amd.Engine.write_gapped_tsv, alga_amd.Gapped.to_host, alga_amd.Gapped.cigar_strings):
        assert callable(fn)
    for name in ("indel_positions", "overhang", "empty_pass"):
        assert alga_amd.engine.cigar_strings(QC.checked(name)) == GC.cigar_strings(QC.checked(name))
    binary = open(alga_amd.library_path(), "rb").read()
    for k in KERNELS:
        assert k.encode() in binary


def test_new_kernels_resources():
    """The compiler's resource report of gapped_kernels.hip: every k_gp_* is there, no VGPR spill and no scratch in any of them"""
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_gapped_resources_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    src = os.path.join(ROOT, "alga_amd", "csrc", "gapped_kernels.hip")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    finally:
        if os.path.exists(out):
            os.remove(out)
    lines = r.stderr.splitlines()
    reps = {}
    for i, s in enumerate(lines):
        m = re.search(r"Function Name: \S*?(k_gp_[a-z_]+)E", s)
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
