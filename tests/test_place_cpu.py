"""The read placement without a GPU: the two Python statements of the definition (tests/place_checker.py) agree on the cases of
tests/place_cases.py, the outcomes the cases were made for, the sums on the random set; the library exports the calls; the compiler's resource
report of place_kernels.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import consensus_checker as S
import final_checker as F
import place_cases as PC
import place_checker as P
import unitig_checker as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_pl_node_check", "k_pl_target_check", "k_pl_final_targets", "k_pl_gather", "k_pl_place", "k_pl_depth_add",
           "k_pl_uncovered", "k_pl_pairs", "k_pl_fasta_sizes", "k_pl_fasta_write"]


def assert_same(got, want, what=""):
    for k in P.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    assert got["info"] == want["info"], (what, got["info"], want["info"])


@pytest.mark.parametrize("name", [n for n in sorted(PC.CASES) if n != "rand"])
def test_the_two_statements_agree(name):
    c = PC.case(name)
    for flags in (0, P.DEPTH_MULTI):
        assert_same(PC.checked(name, flags), P.place_bruteforce(*PC.args(c), flags=flags, **c["params"]), (name, flags))
    print(name, PC.checked(name)["info"])


def test_the_two_statements_agree_on_a_cut_of_rand():
    c = PC.rand_cut()
    got = P.place(*PC.args(c), **c["params"])
    assert_same(got, P.place_bruteforce(*PC.args(c), **c["params"]), "rand cut")
    assert got["info"]["multi"] > 0 and got["info"]["unplaced"] > 0 and got["info"]["pairs_proper"] > 0


def test_the_two_statements_agree_on_many_reads():
    c = PC.many_reads(600)
    got = P.place(*PC.args(c), **c["params"])
    assert_same(got, P.place_bruteforce(*PC.args(c), **c["params"]), "many_reads(600)")
    assert got["state"][:8].tolist() == [3, 7] * 4 and (c["lens"][:16] == 1400).all() and c["lens"][16:].max() <= 48      # 67 seeds, then one or two
    i, short = got["info"], got["state"][8:]
    assert i["pairs"] == 300 and i["placed"] > 300 and (short == 0).sum() > 100 and (short & P.MINUS).astype(bool).sum() > 100
    assert (got["t_reads"] > 0).tolist() == [True, False, True, True, True]


def test_outcomes_the_cases_were_made_for():
    w = PC.checked("exact")
    assert (w["hits"] == 1).all() and (w["mm"] == 0).all() and w["pos"].tolist() == list(range(0, 501, 50)) * 2
    assert (w["state"][:11] == P.PLACED | P.UNIQUE).all() and (w["state"][11:] == P.PLACED | P.UNIQUE | P.MINUS).all()
    w = PC.checked("bound")
    assert w["state"].tolist() == [3, 0, 7, 0, 3, 3] and w["mm"].tolist() == [4, 0, 4, 0, 2, 0]
    w = PC.checked("last_seed_only")
    assert w["state"].tolist() == [3, 7, 3] and w["mm"].tolist() == [3, 3, 3]
    w = PC.checked("every_seed_hit")
    assert w["state"].tolist() == [0, 0, 0, 3]                                  # within the Hamming bound, no seed left: the seeded rule
    w = PC.checked("ends")
    assert w["target"].tolist() == [0, 0, 1, 1, 2, 2, 0, 1] + [-1] * 7 and w["pos"][:8].tolist() == [0, 200, 0, 200, 0, 103, 0, 200]
    w = PC.checked("unaligned")
    for idx in range(40):                                                       # read idx: length i, target j, (i + j) % 3 substitutions
        i, j = divmod(idx, 5)
        if (i + j) % 3 == 0 or i >= 3:                                          # none, or S >= 3 seeds for at most 2 substitutions
            assert w["state"][idx] & P.PLACED and w["target"][idx] == j and bool(w["state"][idx] & P.MINUS) == bool((i + j) & 1), idx
    assert w["mm"][40] == 3 and w["state"][40] == 3 and w["state"][41] == 7 and w["pos"][40:42].tolist() == [211, 211] and w["state"][42:].tolist() == [0, 0, 0, 0]
    w = PC.checked("repeat")
    assert w["hits"][:4].tolist() == [2, 2, 3, 2] and w["target"][:2].tolist() == [0, 0] and w["state"][1] == P.PLACED | P.MINUS
    assert w["state"][4:9].tolist() == [3, 3, 0, 1, 7] and w["hits"][7] == 4 and w["info"]["seeds_over_max_occ"] == 6            # the two y seeds of three nodes (the other strand of y is not indexed)
    w = PC.checked("palindrome")
    assert w["hits"].tolist() == [2, 1] and w["state"].tolist() == [P.PLACED, P.PLACED | P.UNIQUE]
    w = PC.checked("saturate")
    assert w["hits"].tolist() == [255, 0] and w["info"]["hits_saturated"] == 1 and w["pos"][0] == 0
    w = PC.checked("pairs")["info"]
    assert (w["pairs"], w["pairs_proper"], w["pairs_improper"], w["pairs_split"], w["pairs_not_unique"]) == (17, 9, 5, 1, 2)
    assert w["insert_median"] == 300 and PC.checked("pairs")["insert_hist"][400] == 1
    w = PC.checked("many_seeds")                                                # 133 seeds: chunks of 64 seeds, see the case
    assert w["target"].tolist() == [0, 0, 0, 0, -1, 2, 2, 0, 0, 0, 0, 1] and w["pos"].tolist() == [137, 137, 137, 137, -1, 80, 80, 237, 237, 237, 237, 55]
    assert w["mm"].tolist() == [0, 64, 128, 128, 0, 0, 0, 64, 63, 63, 64, 64] and w["hits"].tolist() == [1, 1, 1, 1, 0, 1, 1, 2, 2, 2, 2, 1]
    assert w["state"].tolist() == [3, 3, 3, 7, 0, 3, 7, 1, 1, 1, 5, 3] and w["info"]["seeds_over_max_occ"] == 128
    assert (PC.case("many_seeds")["lens"][1::2] // PC.K).tolist() == [133, 133, 133, 133, 133, 133, 133, 65, 64, 64, 65, 133]
    c = PC.case("many_seeds")
    w = P.place(*PC.args(c), **dict(c["params"], k=8))                          # 350 seeds; read 4 has a seed left
    assert w["state"].tolist() == [3, 3, 3, 7, 3, 3, 7, 1, 1, 1, 5, 3] and w["mm"][4] == 133 and w["hits"].tolist() == [1] * 7 + [2] * 4 + [1]
    w = P.place(*PC.args(c), **dict(c["params"], k=31))
    assert w["state"].tolist() == [3, 3, 3, 7, 0, 3, 7, 0, 1, 1, 0, 3]
    w = PC.checked("mm_limit")
    assert w["mm"].tolist() == [254, 0, 254] and w["state"].tolist() == [3, 0, 7] and w["hits"].tolist() == [1, 0, 1]
    for flags in (0, P.DEPTH_MULTI):
        w, tl = PC.checked("tiny_targets", flags), PC.case("tiny_targets")["tlen"]
        un = w["t_uncovered"].astype(np.int64)
        assert (w["info"]["reads"], w["info"]["unique"], len(w["cover"]), int(w["cover"].max())) == (87, 87, 4959, 2)
        assert [int((tl > 0).sum()), int(((tl > 0) & (un == 0)).sum()), int(((un > 0) & (un < tl)).sum()), int(((tl > 0) & (un == tl)).sum())] == [111, 53, 10, 48]
    assert P.place(*PC.args(PC.case("tiny_targets")), k=8)["info"]["index_positions"] > w["info"]["index_positions"]             # the 16- and 20-base targets
    for name in ("empty_targets", "empty_reads", "empty_short"):
        w = PC.checked(name)
        assert w["info"]["placed"] == 0 and w["info"]["index_positions"] == (250 if name == "empty_reads" else 0) and (w["cover"] == 0).all()


def test_sums_on_rand():
    for flags in (0, P.DEPTH_MULTI):
        w = PC.checked("rand", flags)
        i = w["info"]
        assert int(w["cover"].sum()) == int(w["t_bases"].sum())
        assert i["pairs"] == 750 == i["pairs_proper"] + i["pairs_improper"] + i["pairs_split"] + i["pairs_not_unique"]
        assert int(w["insert_hist"].sum()) == i["pairs_proper"] > 300 and i["placed"] + i["unplaced"] == i["reads"] == 1500
        assert int(w["t_reads"].sum()) == (i["placed"] if flags else i["unique"])
        assert i["multi"] > 20 and i["unplaced"] > 20 and 200 <= i["insert_median"] <= 500
    print(i)


def test_depth_headers_the_header_case_was_made_for():
    """the contig set of the GPU test's header case by the checkers of the earlier stages (every read its own accepted contig, ids by
    descending length), and the header ends the reads of PC.header_reads were chosen for"""
    words, lens = PC.header_nodes()
    u = U.unitigs(words, lens, np.zeros((0, 3), np.int32), skip_isolated=False)
    cons = S.consensus_pileup(words, lens, u, 0)
    fin = F.final_contigs(u, cons, 1, 95, 0)
    order = fin["order"].astype(np.int64)
    assert fin["n_accepted"] == fin["n_written"] == 14 and fin["len"][order].tolist() == sorted(PC.HEADER_LENS, reverse=True)
    begin = 16 * np.asarray(u["word_off"]).astype(np.int64)[order] + fin["begin"][order]
    tlen = fin["len"][order].astype(np.int32)
    contigs = [P.codes_of(cons["words"], begin[j], int(tlen[j])) for j in range(14)]
    rows, rlens = P.nodes_of(PC.header_reads(contigs))
    w = P.place(rows, rlens, None, cons["words"], begin, tlen)
    assert w["info"]["unique"] == w["info"]["reads"] == len(rlens) // 2 == 11 + 120 + 1000 + 11 + 3 + 3
    minus = (w["state"] & P.MINUS).astype(bool)
    for j in range(14):
        h = P.depth_header(j, int(tlen[j]), w["t_reads"][j], w["t_bases"][j])
        assert h.startswith(">contig_id=%d_length=%d_reads=" % (j, tlen[j])) and PC.HEADER_ENDS[int(tlen[j])] in h, h
        if tlen[j] != 1200:
            assert h.endswith(PC.HEADER_ENDS[int(tlen[j])]), h
        assert minus[w["target"] == j].all() == (tlen[j] == 480) or w["t_reads"][j] == 0
    assert tlen[10:].tolist() == [64, 50, 40, 21]                                # the two-digit ids have two-digit lengths


def test_refusals_of_the_checker():
    c = PC.case("pairs")
    for kw in (dict(k=7), dict(k=32), dict(max_mismatches=-1), dict(max_mismatches=255), dict(max_occ=0), dict(max_occ=65536), dict(max_insert=0),
               dict(max_insert=(1 << 20) + 1), dict(flags=2)):
        with pytest.raises(ValueError):
            P.place(*PC.args(c), **kw)
    rows = c["rows"].copy()
    rows[0, 0] ^= 1
    with pytest.raises(ValueError):
        P.place(rows, *PC.args(c)[1:])
    po = c["pair_off"].copy()
    po[2] = po[3] = 0
    with pytest.raises(ValueError):
        P.place(c["rows"], c["lens"], po, *PC.args(c)[3:])
    with pytest.raises(OverflowError):
        P.place(c["rows"], c["lens"], None, c["twords"], np.zeros(3, np.int64), np.full(3, 2 ** 31 - 1, np.int32))


def test_library_exports_the_calls_and_the_engine_has_the_methods():
    lib = alga_amd.load_library()
    for sym in ("alga_place_default_params", "alga_place_reads_device", "alga_place_reads_on_final_device", "alga_write_final_fasta_depth_device"):
        assert hasattr(lib, sym) and sym in alga_amd.engine.EXPORTS
    assert callable(alga_amd.Engine.place_reads) and callable(alga_amd.Engine.place_params)
    assert lib.alga_abi_version() == 7                                       # the calls only add to the ABI
    p = alga_amd.engine.PlaceParams()
    lib.alga_place_default_params(C.byref(p))
    assert (p.k, p.max_mismatches, p.max_occ, p.max_insert, p.flags) == (21, 4, 256, 1000, 0)
    assert C.sizeof(alga_amd.engine.PlaceParams) == 32 and C.sizeof(alga_amd.engine.PlaceInfo) == 8 * (17 + 4)
    assert C.sizeof(alga_amd.engine.PlacementsC) == 8 * (4 + 12)
    binary = open(alga_amd.library_path(), "rb").read()
    for k in KERNELS:
        assert k.encode() in binary


def test_new_kernels_resources():
    """The compiler's resource report of place_kernels.hip: no VGPR spill and no scratch in any kernel"""
    src = os.path.join(ROOT, "alga_amd", "csrc", "place_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_place_resources_%d.o" % os.getpid())
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
        m = re.search(r"Function Name: \S*?(k_pl_[a-z_]+?)E[A-Z]", s)
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
