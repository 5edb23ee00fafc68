"""The pair calls over both passes and the SAM text without a GPU: every case of tests/sam_cases.py passes the independent reading of
tests/sam_invariants.py and has the outcome it was made for; where no read is gapped-placed the checker's pair counters equal
place_checker's; ALGA_SAM_SKIP_UNPLACED only removes lines; the exports and struct sizes of the built library; the compiler's resource report
of sam_kernels.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import alga_amd.engine as AE
import place_checker as P
import sam_cases as SQ
import sam_checker as SC
import sam_invariants as SI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_sam_pair_check", "k_sam_judge", "k_sam_sizes", "k_sam_write")


@pytest.mark.parametrize("name", sorted(SQ.CASES))
def test_case_outcome_and_invariants(name):
    w = SQ.checked(name)
    c = w["case"]
    w["case"]["outcome"](w)
    for flags in (0, SC.NAMES_DEPTH):
        text = SC.sam(c["rows"], c["lens"], c["pair_off"], w["pl"], w["gp"], w["calls"], flags)
        seen = SI.check(text, c["reads"], c["seqs"])
        i = w["calls"]["info"]
        assert (seen["records"], seen["placed"], seen["pairs"], seen["proper"]) == (i["live"], i["placed_h"] + i["placed_g"], i["pairs"], i["pairs_proper"]), (seen, i)
    # the Hamming pass alone
    text = SC.sam(c["rows"], c["lens"], c["pair_off"], w["pl"], None, w["no_gp"])
    assert SI.check(text, c["reads"], c["seqs"])["placed"] == w["no_gp"]["info"]["placed_h"] and w["no_gp"]["info"]["placed_g"] == 0


@pytest.mark.parametrize("name", sorted(SQ.CASES))
def test_without_gapped_reads_the_counters_are_the_placements(name):
    """Rule 2 for two H reads is rule 6 of the placement word for word.  The placement counts every pair_off pair, this stage only live ones, so
    the equality is stated where every paired read is live (all cases but the one with a removed read and its mate, where the difference is
    exactly that pair)"""
    w = SQ.checked(name)
    c, pl, got = w["case"], w["pl"], w["no_gp"]
    dead = 0 if c["pair_off"] is None else sum(1 for r in range(len(c["lens"]) // 2) if c["pair_off"][2 * r + 1] == 1 and min(c["lens"][2 * r + 1], c["lens"][2 * r + 3]) < 1)
    assert dead == (1 if name == "unplaced_and_dead" else 0)
    for k in SC.PAIR_COUNTERS:
        extra = dead if k in ("pairs", "pairs_not_unique") else 0
        assert got["info"][k] + extra == pl["info"][k], (k, got["info"], pl["info"])
    assert (got["insert_hist"] == pl["insert_hist"]).all()


@pytest.mark.parametrize("name", sorted(SQ.CASES))
def test_skip_unplaced_only_removes_lines(name):
    w = SQ.checked(name)
    c = w["case"]
    full = w["text"].split(b"\n")
    some = SC.sam(c["rows"], c["lens"], c["pair_off"], w["pl"], w["gp"], w["calls"], SC.SKIP_UNPLACED)
    assert some.split(b"\n") == [s for s in full if s.startswith(b"@") or not s or not int(s.split(b"\t")[1]) & 0x4]
    SI.check(some, c["reads"], c["seqs"], complete=False)


def test_many_pairs_per_distinct_pair():
    """the set of tests/test_gpu_sam.py's grid-stride test: every record of a drawn pair is the pool pair's record but for the read index"""
    c, n_pool = SQ.many_pairs(80)
    pl = P.place(c["rows"], c["lens"], c["pair_off"], *SQ.targets(c), **c["place"])
    import gapped_checker as GC
    gp = GC.gapped_banded(c["rows"], c["lens"], pl, *SQ.targets(c), **c["gapped"])
    calls = SC.pair_calls(c["lens"], c["pair_off"], pl, gp, c["max_insert"])
    text = SC.sam(c["rows"], c["lens"], c["pair_off"], pl, gp, calls)
    seen = SI.check(text, c["reads"], c["seqs"])
    recs = [s for s in text.split(b"\n") if s and not s.startswith(b"@")]
    assert len(recs) == 160 and seen["proper"] >= 20 and seen["clipped"] == 0 and calls["info"]["proper_with_gapped"] >= 5 and calls["info"]["unplaced"] >= 10
    for i in range(n_pool, 80):
        j = next(x for x in range(n_pool) if (7 * x) % n_pool == (7 * i) % n_pool)
        for h in (0, 1):
            assert recs[2 * i + h].split(b"\t")[1:] == recs[2 * j + h].split(b"\t")[1:] and recs[2 * i + h].split(b"\t")[0] == b"r%d" % (2 * i)


def test_exports_and_struct_sizes():
    """the new calls are in the built library, the structs have the documented sizes, the ABI stays 7"""
    lib = alga_amd.load_library()
    assert lib.alga_abi_version() == 7
    for f in ("alga_pair_default_params", "alga_judge_pairs_device", "alga_write_sam_device"):
        assert f in AE.EXPORTS and hasattr(lib, f), f
    assert (C.sizeof(AE.PairParams), C.sizeof(AE.PairCallsC), C.sizeof(AE.PairInfo), C.sizeof(AE.SamParams)) == (32, 40, 12 * 8 + 2 * 8 + 2 * 8, 32)
    p = AE.PairParams()
    p.max_insert, p.flags = 7, 7
    p.reserved[5] = 9
    lib.alga_pair_default_params(C.byref(p))
    assert (p.max_insert, p.flags, list(p.reserved)) == (1000, 0, [0] * 6)
    assert (AE.SAM_NAMES_DEPTH, AE.SAM_SKIP_UNPLACED) == (SC.NAMES_DEPTH, SC.SKIP_UNPLACED) == (1, 2)
    header = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    for s in ("alga_judge_pairs_device", "alga_write_sam_device", "#define ALGA_SAM_NAMES_DEPTH   1", "#define ALGA_SAM_SKIP_UNPLACED 2", "#define ALGA_AMD_ABI_VERSION 7"):
        assert s in header, s


def test_new_kernels_resources():
    """The compiler's resource report of sam_kernels.hip: every k_sam_* is there, no VGPR spill and no scratch in any of them"""
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_sam_resources_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    src = os.path.join(ROOT, "alga_amd", "csrc", "sam_kernels.hip")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    finally:
        if os.path.exists(out):
            os.remove(out)
    lines = r.stderr.splitlines()
    reps = {}
    for i, s in enumerate(lines):
        m = re.search(r"Function Name: \S*?(k_sam_[a-z_]+)E", s)
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
