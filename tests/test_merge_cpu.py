"""The merge stage without a GPU: the two Python statements of the definition (tests/merge_checker.py) agree on the cases of
tests/merge_cases.py, the outcomes the cases were made for, the planted genome; the refusals of the checker; the library exports the calls
and the header declares them; the compiler's resource report of merge_kernels.hip, seed_index.hip and chain_kernels.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import grow_cases as GQ
import grow_checker as GC
import merge_cases as QC
import merge_checker as MC
import merge_invariants as MI
import place_checker as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_mg_check", "k_mg_end_lens", "k_mg_ends", "k_mg_overlap", "k_mg_joins", "k_mg_cycle_drop", "k_mg_rank_init", "k_mg_place", "k_mg_layout", "k_mg_build",
           "k_mg_fasta_sizes", "k_mg_fasta_write",
           "k_seed_keys", "k_seed_dir",                         # (seed_index.hip: the index the placement, the grow and the merge stage build)
           "k_ch_cycle_init", "k_ch_cycle_jump", "k_ch_rank_jump"]   # (chain_kernels.hip: the jumps the scaffolder, the merge and the stitch stage share)
SYMBOLS = ("alga_merge_default_params", "alga_merge_targets_device", "alga_write_merged_fasta_device")
# (ends_with_overlap, ends_ambiguous, joins, joins_dropped_cycle, merged) of every variant of every case
OUTCOMES = {"word_seams": [(4, 0, 2, 0, 9)], "pairings": [(8, 0, 4, 0, 5), (0, 0, 0, 0, 9)], "half_length": [(2, 0, 1, 0, 3)], "max_overlap": [(2, 0, 1, 0, 3)], "partial_word": [(6, 0, 3, 0, 9)],
            "seeds64": [(2, 0, 1, 0, 1), (0, 0, 0, 0, 2)], "one_sided": [(1, 0, 0, 0, 3), (2, 0, 1, 0, 2)], "two_partners": [(3, 1, 0, 0, 3)], "periodic": [(2, 2, 0, 0, 2)],
            "mismatch_column": [(2, 0, 1, 0, 1)], "path5": [(8, 0, 4, 0, 1)], "ring3": [(6, 0, 2, 1, 1)], "ring2": [(4, 0, 1, 1, 1)], "self_overlap": [(0, 0, 0, 0, 2)],
            "t0": [(0, 0, 0, 0, 0)], "all_empty": [(0, 0, 0, 0, 0)], "one": [(0, 0, 0, 0, 1)], "short": [(0, 0, 0, 0, 4)]}


def assert_same(got, want, what=""):
    for k in MC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    assert got["info"] == want["info"], (what, got["info"], want["info"])


@pytest.mark.parametrize("name,i", QC.every())
def test_the_two_statements_agree(name, i):
    c, want = QC.case(name), QC.checked(name, i)
    v = c["variants"][i]
    assert_same(MC.merge_bruteforce(c["seqs"], **v), want, (name, i))
    info = want["info"]
    assert (info["ends_with_overlap"], info["ends_ambiguous"], info["joins"], info["joins_dropped_cycle"], info["merged"]) == OUTCOMES[name][i], info
    MI.assert_invariants(c, want, v)                                             # what holds for every result
    print(name, i, info)


def test_every_case_is_listed():
    assert sorted(OUTCOMES) == sorted(QC.CASES) and all(len(OUTCOMES[n]) == len(QC.case(n)["variants"]) for n in QC.CASES)


def test_outcomes_the_cases_were_made_for():
    # o = min_overlap in the four pairings of ends: right-left, right-right, left-left, left-right; the empty target and the single base between them
    w = QC.checked("pairings")
    assert w["partner"].tolist() == [-1, 2, 1, -1, -1, -1, -1, 9, -1, 7, -1, -1, 14, -1, 12, -1, 19, -1, -1, 16]
    assert sorted(set(w["olen"].tolist())) == [0, 42] and w["merged"].tolist() == [0, 0, -1, 1, 1, 2, 3, 3, 4, 4] and w["orient"].tolist() == [0, 0, 0, 0, 1, 0, 1, 0, 1, 1]
    assert (QC.checked("pairings", 1)["partner"] == -1).all()                    # the same targets at min_overlap - 1
    # n = 2 o joins, n = 2 o - 1 does not: its window has 49 bases
    w = QC.checked("half_length")
    assert w["partner"].tolist() == [-1, 2, 1, -1, -1, -1, -1, -1] and QC.case("half_length")["tlen"].tolist() == [300, 100, 300, 99]
    # o = max_overlap and max_overlap + 1
    w = QC.checked("max_overlap")
    assert w["olen"].tolist() == [0, 64, 64, 0, 0, 0, 0, 0]
    # o mod 16 in 0, 1, 15: mm 1 joins, mm 2 does not
    w, c = QC.checked("partial_word"), QC.case("partial_word")
    assert sorted(int(o) % 16 for o in w["olen"] if o) == [0, 0, 1, 1, 15, 15] and [int(m) for m, o in zip(w["mm"], w["olen"]) if o] == [1] * 6
    assert [int(x) for x in np.nonzero(w["hits"])[0]] == [1, 2, 9, 11, 16, 18] and w["len"].tolist() == [362, 200, 210, 361, 200, 210, 363, 200, 210]
    # 64 seeds; the mismatch is allowed or not
    w = QC.checked("seeds64")
    assert w["olen"].tolist() == [0, 512, 512, 0] and w["mm"].tolist() == [0, 1, 1, 0] and w["info"]["seeds"] == 4 * 64
    # visible from one end only: the other end's one clean seed is over max_occ
    w = QC.checked("one_sided")
    assert w["partner"].tolist() == [-1, -1, 1, -1, -1, -1] and w["info"]["seeds_over_max_occ"] == 1 and w["end_state"].tolist() == [0, 0, 1, 0, 0, 0]
    assert QC.checked("one_sided", 1)["partner"].tolist() == [-1, 2, 1, -1, -1, -1]
    # two partners: ambiguous; both of them choose it, it chooses the smaller end: a choice that is not mutual
    w = QC.checked("two_partners")
    assert w["partner"].tolist() == [-1, 2, 1, -1, 1, -1] and w["hits"].tolist() == [0, 2, 1, 0, 1, 0] and w["end_state"].tolist() == [0, 3, 1, 0, 1, 0]
    # a periodic end: four o at one partner, the longest is the best
    w = QC.checked("periodic")
    assert w["hits"].tolist() == [0, 4, 4, 0] and w["olen"].tolist() == [0, 80, 80, 0] and w["end_state"].tolist() == [0, 3, 3, 0]
    # the overlapped bases are the earlier contig's
    w, c = QC.checked("mismatch_column"), QC.case("mismatch_column")
    s = MC.sequences(w)[0]
    assert (s == np.concatenate([c["seqs"][0], c["seqs"][1][50:]])).all() and s[c["at"]] == c["seqs"][0][c["at"]] != c["seqs"][1][10]
    # five in a row: the path starts at contig 1, the terminal of smaller id; the middle member is covered twice over its whole length
    w, c = QC.checked("path5"), QC.case("path5")
    assert w["m_members"].tolist() == [1, 4, 2, 0, 3] and w["orient"].tolist() == [1, 0, 0, 0, 1] and w["start"].tolist() == [500, 0, 450, 740, 250]
    assert w["overlap_after"].tolist() == [60, 50, 50, 0, 50] and (MC.sequences(w)[0] == c["g"]).all()
    # rings: opened at contig 0, whose left end loses its join
    w, c = QC.checked("ring3"), QC.case("ring3")
    assert w["end_state"].tolist() == [9, 5, 5, 5, 5, 9] and w["m_members"].tolist() == [0, 1, 2] and (MC.sequences(w)[0] == np.concatenate([c["g"], c["g"][:50]])).all()
    w = QC.checked("ring2")
    assert w["end_state"].tolist() == [9, 5, 9, 5] and w["orient"].tolist() == [0, 1] and w["len"].tolist() == [450]
    # a ring of one counts nowhere
    assert (QC.checked("self_overlap")["hits"] == 0).all()
    assert QC.checked("t0")["words"].tolist() == [0, 0] and QC.checked("all_empty")["merged"].tolist() == [-1, -1, -1] and QC.checked("short")["info"]["ends"] == 0


def test_planted_genome():
    """the planted genome of the grow stage through three checker rounds of place -> grow, then merged with the defaults: one contig, the genome's
    window 11 .. 2992, from one join of 58 bases without a mismatch; a fourth round would grow nothing"""
    c, g, meta = GQ.planted()
    grown = []
    for rnd in range(3):
        w = GC.grow_index(c["rows"], c["lens"], P.place(*GQ.place_args(c)), c["seqs"])
        grown.append((w["left"].tolist(), w["right"].tolist()))
        c = GQ.next_round(c, w)
    assert grown[2] == ([0, 27], [26, 0])                                         # (left, right) of the two contigs
    assert (c["seqs"][0] == g[11:1292]).all() and (c["seqs"][1] == g[1234:2992]).all()
    assert GC.grow_index(c["rows"], c["lens"], P.place(*GQ.place_args(c)), c["seqs"])["info"]["bases_added"] == 0
    w = MC.merge_index(c["seqs"])
    assert_same(MC.merge_bruteforce(c["seqs"]), w, "planted")
    i = w["info"]
    assert (i["joins"], i["bases_removed"], i["longest_overlap"], i["join_mismatches"], i["merged"], i["ends_ambiguous"]) == (1, 58, 58, 0, 1, 0)
    assert w["partner"].tolist() == [-1, 2, 1, -1] and w["olen"].tolist() == [0, 58, 58, 0] and w["mm"].tolist() == [0, 0, 0, 0]
    assert len(w["len"]) == 1 and (MC.sequences(w)[0] == g[11:2992]).all()


def test_refusals_of_the_checker():
    c = QC.case("path5")
    bad = (dict(k=7), dict(k=32), dict(max_mismatches=-1), dict(max_mismatches=255), dict(max_occ=0), dict(max_occ=65536), dict(min_overlap=20), dict(min_overlap=513),
           dict(max_overlap=41), dict(max_overlap=4097), dict(k=8, min_overlap=8, max_overlap=513), dict(k=31, min_overlap=31, max_overlap=1985))
    for fn in (MC.merge_index, MC.merge_bruteforce):
        for kw in bad:
            with pytest.raises(ValueError):
                fn(c["seqs"], **kw)
        fn(c["seqs"], k=8, min_overlap=8, max_overlap=512)                       # the bounds themselves are taken
        fn(c["seqs"], k=31, min_overlap=1984, max_overlap=1984)
    with pytest.raises(ValueError):
        MC.check_lengths([10, -1])
    with pytest.raises(OverflowError):
        MC.check([range(2 ** 31 - 1)] * 3, **MC.DEFAULT)                         # the column sum above 2^32 - 2


def test_library_exports_the_calls_and_the_header_declares_them():
    lib = alga_amd.load_library()
    header = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in alga_amd.engine.EXPORTS
        assert re.search(r"^(void|int)\s+%s\(" % sym, header, re.M), sym
    assert lib.alga_abi_version() == 7                                       # the calls only add to the ABI
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} alga_merge_params;", header)
    assert m and re.findall(r"\b([a-z_0-9]+)(?:\[2\])?[,;]", strip(m.group(1))) == [k for k, _ in alga_amd.MergeParams._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} alga_merge_info;", header)
    assert m and re.findall(r"\b([a-z_0-9]+)[,;]", strip(m.group(1))) == [k for k, _ in alga_amd.MergeInfo._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} alga_merged;", header)
    assert m and [x.lstrip("*") for x in re.findall(r"(\*?\b[a-z_0-9]+)[,;]", strip(m.group(1)))] == [k for k, _ in alga_amd.MergedC._fields_]
    p = alga_amd.MergeParams()
    lib.alga_merge_default_params(C.byref(p))
    got = {k: getattr(p, k) for k in MC.DEFAULT}
    assert got == MC.DEFAULT == dict(k=21, max_mismatches=1, max_occ=256, min_overlap=42, max_overlap=512) and p.flags == 0 and list(p.reserved) == [0] * 2
    assert p.min_overlap == p.k * (p.max_mismatches + 1)
    assert C.sizeof(alga_amd.MergeParams) == 32 and C.sizeof(alga_amd.MergeInfo) == 8 * (19 + 4) and C.sizeof(alga_amd.MergedC) == 8 * (4 + 16)
    assert [k for k, _ in alga_amd.MergeInfo._fields_][:19] == list(MC.COUNTERS) and [k for k, _, _, _ in alga_amd.Merged.KEYS] == list(MC.ARRAYS)
    E = alga_amd.engine
    assert (E.MERGE_END_HAS_OVERLAP, E.MERGE_END_AMBIGUOUS, E.MERGE_END_JOINED, E.MERGE_END_DROPPED_CYCLE) == (MC.HAS_OVERLAP, MC.AMBIGUOUS, MC.JOINED, MC.DROPPED_CYCLE) == (1, 2, 4, 8)
    for name, value in (("HAS_OVERLAP", 1), ("AMBIGUOUS", 2), ("JOINED", 4), ("DROPPED_CYCLE", 8)):
        assert re.search(r"#define ALGA_MERGE_END_%s\s+%d\b" % (name, value), header)
    for fn in (alga_amd.Engine.merge_ends, alga_amd.Engine.write_merged_fasta, alga_amd.Merged.to_host, alga_amd.Merged.targets, alga_amd.Merged.merge_tsv):
        assert callable(fn)
    for name in ("pairings", "path5", "ring3", "t0", "partial_word"):
        assert alga_amd.engine.merge_tsv(QC.checked(name), QC.case(name)["tlen"]).encode() == MC.merge_tsv(QC.checked(name), QC.case(name)["tlen"])
    binary = open(alga_amd.library_path(), "rb").read()
    for k in KERNELS:
        assert k.encode() in binary


def test_new_kernels_resources():
    """The compiler's resource report of merge_kernels.hip, seed_index.hip and chain_kernels.hip: every k_mg_*, k_seed_* and k_ch_* is there, no
    VGPR spill and no scratch in any of them"""
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_merge_resources_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    lines = []
    for name in ("merge_kernels.hip", "seed_index.hip", "chain_kernels.hip"):
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
        m = re.search(r"Function Name: \S*?(k_(?:mg|seed|ch)_[a-z_]+)E", s)
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
