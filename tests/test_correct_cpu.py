"""The read error correction without a GPU: the definition (tests/correct_checker.py) on the cases of tests/correct_cases.py -- strand symmetry,
lengths and tails, the outcomes stated by hand, and on the random sets no error-free read changed and no read made worse; the library exports
the calls; the compiler's resource report of correct_kernels.hip; the command line's new switches."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import correct_cases as CC
import correct_checker as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_cr_twin", "k_cr_hist", "k_cr_sum", "k_cr_emit", "k_cr_runs", "k_cr_append", "k_cr_dir", "k_cr_fix"]


def hamming(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_checker_is_strand_symmetric_and_leaves_lengths_and_tails(name):
    c = CC.case(name)
    rows, info = CC.checked(name)
    lens = c["lens"]
    assert rows.shape == c["rows"].shape and rows.dtype == np.uint32
    # the mirror image of the input gives the mirror image of the output, and the same counters
    mrows, mlens = K.mirror(c["rows"], lens)
    got, minfo = K.correct(mrows, mlens, **c["params"])
    assert (got == K.mirror(rows, lens)[0]).all()
    assert minfo == info
    for i in range(len(lens)):
        length = int(lens[i])
        if length < c["params"]["k"]:
            assert (rows[i] == c["rows"][i]).all()
            continue
        nw = K.blocks_of(length)
        assert (rows[i][nw:] == c["rows"][i][nw:]).all()
        assert (K.pack(K.codes_of(rows[i], length), rows.shape[1]) == rows[i])[:nw].all()          # tail bits zero
    fw = K.forward_reads(rows, lens)
    for r, x in enumerate(fw):
        if x is not None:
            assert (K.codes_of(rows[2 * r], len(x)) == K.revcomp(x)).all()
    assert info["runs"] == info["runs_fixed"] + info["runs_ambiguous"] + info["runs_no_candidate"] + info["runs_skipped"]
    print(name, info)


@pytest.mark.parametrize("name", [n for n in sorted(CC.CASES) if CC.CASES[n][0] is not None and n not in CC.RANDOM])
def test_checker_gives_the_outcomes_stated_by_hand(name):
    c = CC.case(name)
    rows, info = CC.checked(name)
    got = K.forward_reads(rows, c["lens"])
    assert len(got) == len(c["want"])
    for r, (g, w) in enumerate(zip(got, c["want"])):
        assert (g is None) == (w is None), r
        if g is not None:
            assert len(g) == len(w) and (g == w).all(), (name, r)
    if name == "every_position":
        assert info["runs_fixed"] == 70 and info["runs_ambiguous"] == 0
    if name == "two_errors":
        k = c["params"]["k"]
        assert info["runs_fixed"] == 2 * 2 and info["runs_skipped"] == k              # d = k + 1, k + 2: two runs each; d <= k: one long run
    if name == "ambiguity":
        assert info["runs_ambiguous"] == c["n_ambiguous"] > 0 and info["runs_no_candidate"] == c["n_no_candidate"] and info["reads_changed"] == 0
    if name == "shapes":
        assert info["runs_fixed"] == 5 + 2 and info["runs_skipped"] == 1 and info["reads_changed"] == 3
    if name == "heavy":
        assert info["runs_fixed"] == 1
    if name in ("empty", "all_removed"):
        assert all(v == 0 for v in info.values())


@pytest.mark.parametrize("name", CC.RANDOM)
def test_random_sets_no_clean_read_changed_and_none_made_worse(name):
    c = CC.case(name)
    rows, info = CC.checked(name)
    before, after = K.forward_reads(c["rows"], c["lens"]), K.forward_reads(rows, c["lens"])
    bad0 = bad1 = restored = 0
    for b, a, t in zip(before, after, c["truth"]):
        d0, d1 = hamming(b, t), hamming(a, t)
        assert d1 <= d0                                          # none made worse
        if d0 == 0:
            assert (a == b).all()                                # no error-free read changed
        bad0 += d0 > 0
        bad1 += d1 > 0
        restored += d0 > 0 and d1 == 0
    print(name, "reads", len(before), "erroneous before / after", bad0, bad1, "restored", restored, info)
    assert info["runs_fixed"] > 0 and restored > 0


def test_refusals_of_the_checker():
    c = CC.case("two_errors")
    for kw in (dict(k=20), dict(k=33), dict(k=3), dict(solid_min=0), dict(min_run=0)):
        with pytest.raises(ValueError):
            K.correct(c["rows"], c["lens"], **kw)
    rows = c["rows"].copy()
    rows[0, 0] ^= 1
    with pytest.raises(ValueError):
        K.correct(rows, c["lens"])
    lens = c["lens"].copy()
    lens[0] -= 1
    with pytest.raises(ValueError):
        K.correct(c["rows"], lens)


def test_library_exports_the_calls_and_the_engine_has_the_methods():
    lib = alga_amd.load_library()
    for sym in ("alga_correct_default_params", "alga_correct_reads_device", "alga_correct_parsed_reads", "alga_ingest_corrected_device"):
        assert hasattr(lib, sym) and sym in alga_amd.engine.EXPORTS
    for m in ("correct_reads", "correct_reads_device", "correct_params"):
        assert callable(getattr(alga_amd.Engine, m))
    assert lib.alga_abi_version() == 7                                       # the calls only add to the ABI
    p = alga_amd.engine.CorrectParams(-1, -1, -1, -1)
    lib.alga_correct_default_params(C.byref(p))
    assert (p.k, p.solid_min, p.min_run, p.reserved) == (21, 3, 1, 0)
    assert C.sizeof(alga_amd.engine.CorrectParams) == 16 and C.sizeof(alga_amd.engine.CorrectInfo) == 8 * (11 + 4)
    binary = open(alga_amd.library_path(), "rb").read()
    for k in KERNELS:
        assert k.encode() in binary


def test_new_kernels_resources():
    """The compiler's resource report of correct_kernels.hip: no VGPR spill and no scratch in any kernel"""
    src = os.path.join(ROOT, "alga_amd", "csrc", "correct_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_correct_resources_%d.o" % os.getpid())
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
        m = re.search(r"Function Name: \S*?(k_cr_[a-z_]+?)E[A-Z]", s)
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


def alga_hip():
    return os.path.join(ROOT, "alga_amd", "bin", "alga_hip")


def test_command_line_names_the_switches_and_refuses_an_even_k(tmp_path):
    r = subprocess.run([alga_hip(), "--help"], capture_output=True, text=True)
    text = r.stdout + r.stderr
    for flag in ("--correct_reads", "--correct_k", "--correct_solid", "--corrected_reads"):
        assert flag in text
    fa = tmp_path / "r.fasta"
    fa.write_text(">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    r = subprocess.run([alga_hip(), "--file1=%s" % fa, "--correct_reads=1", "--correct_k=20", "--output=%s" % (tmp_path / "o.fasta")], capture_output=True, text=True)
    assert r.returncode != 0 and "correct_k" in (r.stdout + r.stderr)
