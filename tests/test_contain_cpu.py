"""The containment stage without a GPU: the two Python statements of the definition (tests/contain_checker.py) agree on the cases of
tests/contain_cases.py, the outcomes the cases were made for; the refusals of the checker; the library exports the calls and the header
declares them; the compiler's resource report of contain_kernels.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import contain_cases as QC
import contain_checker as CC
import place_checker as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_ct_check", "k_ct_cols", "k_ct_contain", "k_ct_decide", "k_ct_root_init", "k_ct_root_jump", "k_ct_absorbed", "k_ct_number", "k_ct_build", "k_ct_fasta_sizes",
           "k_ct_fasta_write"]
SYMBOLS = ("alga_contain_default_params", "alga_drop_contained_device", "alga_write_kept_fasta_device")


def assert_same(got, want, what=""):
    for k in CC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k, got[k], want[k])
    assert got["info"] == want["info"], (what, got["info"], want["info"])


def assert_invariants(c, w, v):
    """what holds for every result"""
    seqs, T = c["seqs"], len(c["seqs"])
    pr = dict(CC.DEFAULT, **v)
    kept = w["old"].tolist()
    assert kept == sorted(kept) == [t for t in range(T) if w["state"][t] & CC.KEPT] and w["new"].tolist() == [kept.index(t) if t in kept else -1 for t in range(T)]
    assert int(w["absorbed"].sum()) == w["info"]["contained"] == sum(1 for t in range(T) if w["state"][t] & CC.CONTAINED) == T - len(kept) - sum(1 for s in seqs if len(s) == 0)
    for t in range(T):
        n, st = len(seqs[t]), int(w["state"][t])
        assert bool(st & CC.KEPT) + bool(st & CC.CONTAINED) == (1 if n else 0)
        if st & CC.CONTAINED:
            h, p, s = int(w["host"][t]), int(w["host_pos"][t]), int(w["host_orient"][t])
            Q = P.revcomp(seqs[t]) if s else seqs[t]
            assert CC.can_host(seqs, h, t) and int(np.count_nonzero(Q != seqs[h][p:p + n])) == int(w["mm"][t]) <= CC.bound(n, pr["max_permille"])
            assert bool(st & CC.MINUS) == bool(s) and bool(st & CC.AMBIGUOUS) == (w["hits"][t] > 1) and bool(st & CC.DUPLICATE) == (len(seqs[h]) == n)
            r, rp = int(w["root"][t]), int(w["root_pos"][t])
            assert w["state"][r] & CC.KEPT and 0 <= rp and rp + n <= len(seqs[r]) and w["absorbed"][r] >= 1
        else:
            assert (int(w["host"][t]), int(w["hits"][t]), int(w["mm"][t]), int(w["absorbed"][t]) if not n else 0) == (-1, 0, 0, 0)
            assert int(w["root"][t]) == (t if n else -1) and int(w["root_pos"][t]) == 0 == int(w["root_orient"][t])
    got = CC.sequences(w)
    assert len(got) == len(kept) and all((a == seqs[t]).all() for a, t in zip(got, kept))
    assert w["info"]["columns_after"] + w["info"]["bases_removed"] == w["info"]["columns_before"] == sum(len(s) for s in seqs)


@pytest.mark.parametrize("name,i", QC.every())
def test_the_two_statements_agree(name, i):
    c, want = QC.case(name), QC.checked(name, i)
    v = c["variants"][i]
    assert_same(CC.contain_bruteforce(c["seqs"], **v), want, (name, i))
    assert_invariants(c, want, v)
    print(name, i, want["info"])


@pytest.mark.parametrize("name,i", QC.every())
def test_the_outcome_the_case_was_made_for(name, i):
    """from the case's inputs: the targets it is about have the container it was built with, or none"""
    c, w = QC.case(name), QC.checked(name, i)
    assert len(c["tbegin"]) < 2 or sorted(set((c["tbegin"] & 15).tolist())) == sorted(set(3 * j % 16 for j in range(len(c["tbegin"]))))
    for t, e in c["expect"][i].items():
        if e is None:
            assert w["state"][t] == CC.KEPT and w["host"][t] == -1 and w["hits"][t] == 0, (name, i, t)
        else:
            assert (int(w["host"][t]), int(w["host_pos"][t]), int(w["host_orient"][t]), int(w["mm"][t]), int(w["hits"][t])) == e, (name, i, t)
            assert w["state"][t] & CC.CONTAINED


def test_outcomes_in_detail():
    # n mod 16 = 0, 1, 15 at p = 0, flush right, p mod 16 = 1 and 15
    c, w = QC.case("word_edges"), QC.checked("word_edges")
    assert sorted(set(len(s) % 16 for s in c["seqs"][1::2])) == [0, 1, 15] and sorted(set(int(p) % 16 for p in w["host_pos"][1::2])) == [0, 1, 15]
    assert all(int(w["host_pos"][t]) + len(c["seqs"][t]) == len(c["seqs"][t - 1]) for t in (3, 11, 19)) and w["info"]["contained"] == 12
    # one cooperative pass of 64 words is 1024 bases; the mismatch lies in the last word, behind the last seed
    c = QC.case("pass_edges")
    assert [P.blocks_of(n) for n in QC.PASS_N] == [64, 64, 65, 129] and all(n - 1 >= 16 * (P.blocks_of(n) - 1) and n - 1 >= 21 * min(n // 21, 64) for n in QC.PASS_N)
    assert QC.checked("pass_edges")["info"]["contained"] == 4 and QC.checked("pass_edges", 1)["info"]["contained"] == 0
    # M(99) = 0, M(100) = 1
    assert (CC.bound(99, 10), CC.bound(100, 10), CC.bound(2 ** 31 - 1, 100)) == (0, 1, 214748364)
    assert QC.checked("permille")["state"].tolist()[4:] == [CC.KEPT, CC.CONTAINED, CC.KEPT, CC.CONTAINED]
    # the reverse complement; the palindrome alone
    w = QC.checked("minus")
    assert w["state"].tolist() == [CC.KEPT, CC.CONTAINED | CC.MINUS, CC.KEPT] and w["info"]["contained_minus"] == 1 and w["root_orient"].tolist() == [0, 1, 0]
    # duplicates: the smallest id is kept
    w = QC.checked("duplicates")
    D = CC.CONTAINED | CC.DUPLICATE
    assert w["state"].tolist() == [CC.KEPT, CC.KEPT, D | CC.MINUS, D | CC.AMBIGUOUS, D | CC.AMBIGUOUS] and w["absorbed"].tolist() == [0, 3, 0, 0, 0]
    assert w["info"]["duplicates"] == 3 and w["new"].tolist() == [0, 1, -1, -1, -1]
    # nests: every member's host is its parent, its root the outermost member; the innermost of the nest of 33 is not within M of its root
    c, w = QC.case("chain"), QC.checked("chain")
    where, seqs = c["where"], c["seqs"]
    for d in QC.CHAIN_DEPTHS:
        for i in range(1, d + 1):
            t = where[(d, i)]
            assert w["host"][t] == where[(d, i - 1)] and w["mm"][t] == 1 and w["root"][t] == where[(d, 0)]
            r, rp, ro = int(w["root"][t]), int(w["root_pos"][t]), int(w["root_orient"][t])
            Q = P.revcomp(seqs[t]) if ro else seqs[t]
            assert int(np.count_nonzero(Q != seqs[r][rp:rp + len(Q)])) == i              # one substitution a level
        assert w["absorbed"][where[(d, 0)]] == d
    t = where[(33, 33)]
    assert 33 > CC.bound(len(seqs[t]), 10) and set(w["root_orient"].tolist()) == {0, 1} and len(set(w["host_orient"].tolist())) == 2
    # seed 63 alone; no seed at all
    w = QC.checked("seed63")
    assert w["info"]["contained"] == 1 and w["info"]["candidates"] == 1 and CC.bound(6400, 10) == 64
    c = QC.case("seed63")
    assert int(np.count_nonzero(c["seqs"][3] != c["seqs"][2][41:6441])) == 64
    # all 64 seeds find one placement: it counts once
    w = QC.checked("one_hit")
    assert w["info"]["candidates"] == 1 and w["info"]["seeds"] == 4 * 64 and w["hits"].tolist() == [1, 0]
    # the repeat
    w0, w1 = QC.checked("repeats"), QC.checked("repeats", 1)
    assert w0["info"]["hits_saturated"] == 1 and w0["info"]["candidates"] == 2 * 281 and w0["hits"][0] == 255 and w0["state"][0] == CC.CONTAINED | CC.AMBIGUOUS
    assert w1["info"]["contained"] == 0 and w1["info"]["seeds_over_max_occ"] == w1["info"]["seeds"] == 2 * (5 + 64) and w1["info"]["candidates"] == 0
    # two hosts: by mm, then h, then p, then s
    w = QC.checked("two_hosts")
    assert w["info"]["ambiguous"] == 4 and (w["state"][6:] == CC.CONTAINED | CC.AMBIGUOUS).all()
    # short targets
    w = QC.checked("short")
    assert w["state"].tolist() == [CC.KEPT, CC.KEPT, CC.CONTAINED, 0, CC.KEPT] and w["new"].tolist() == [0, 1, -1, -1, 2] and w["root"].tolist() == [0, 1, 0, -1, 4]
    assert w["info"]["queries"] == 2
    for name in ("t0", "all_empty"):
        w = QC.checked(name)
        assert w["info"]["kept"] == 0 and len(w["old"]) == 0 and len(w["words"]) == 2 and w["col_off"].tolist() == [0]
    assert QC.checked("one")["info"]["kept"] == 1
    # a family sized by the caller
    c = QC.many_queries(200)
    w = CC.contain_index(c["seqs"])
    assert w["info"]["contained"] == 200 // 16 and w["info"]["contained_minus"] == 6


def test_the_checkers_refusals():
    s = QC.case("minus")["seqs"]
    for bad in (dict(k=7), dict(k=32), dict(max_permille=-1), dict(max_permille=101), dict(max_occ=0), dict(max_occ=65536)):
        for fn in (CC.contain_index, CC.contain_bruteforce):
            with pytest.raises(ValueError):
                fn(s, **bad)
    with pytest.raises(ValueError):
        CC.check_lengths([3, -1])
    CC.check_lengths([3, 0])

    class Long:
        def __len__(self):
            return 2 ** 31 - 1
    with pytest.raises(OverflowError):
        CC.check([Long()] * 3, **CC.DEFAULT)


def test_the_library_exports_the_calls_and_the_header_declares_them():
    lib = alga_amd.load_library()
    header = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in alga_amd.engine.EXPORTS
        assert re.search(r"^(void|int)\s+%s\(" % sym, header, re.M), sym
    assert lib.alga_abi_version() == 7                                       # the calls only add to the ABI
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} alga_contain_params;", header)
    assert m and re.findall(r"\b([a-z_0-9]+)(?:\[2\])?[,;]", strip(m.group(1))) == [k for k, _ in alga_amd.ContainParams._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} alga_contain_info;", header)
    assert m and re.findall(r"\b([a-z_0-9]+)[,;]", strip(m.group(1))) == [k for k, _ in alga_amd.ContainInfo._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} alga_kept;", header)
    assert m and [x.lstrip("*") for x in re.findall(r"(\*?\b[a-z_0-9]+)[,;]", strip(m.group(1)))] == [k for k, _ in alga_amd.KeptC._fields_]
    p = alga_amd.ContainParams()
    lib.alga_contain_default_params(C.byref(p))
    assert {k: getattr(p, k) for k in CC.DEFAULT} == CC.DEFAULT == dict(k=21, max_permille=10, max_occ=256) and p.flags == 0 and list(p.reserved) == [0] * 2
    assert C.sizeof(alga_amd.ContainParams) == 24 and C.sizeof(alga_amd.ContainInfo) == 8 * (17 + 4) and C.sizeof(alga_amd.KeptC) == 8 * (3 + 16)
    assert [k for k, _ in alga_amd.ContainInfo._fields_][:17] == list(CC.COUNTERS) and [k for k, _, _, _ in alga_amd.Kept.KEYS] == list(CC.ARRAYS)
    E = alga_amd.engine
    assert (E.CONTAIN_CONTAINED, E.CONTAIN_MINUS, E.CONTAIN_AMBIGUOUS, E.CONTAIN_DUPLICATE, E.CONTAIN_KEPT) == (CC.CONTAINED, CC.MINUS, CC.AMBIGUOUS, CC.DUPLICATE, CC.KEPT)
    for name, value in (("CONTAINED", 1), ("MINUS", 2), ("AMBIGUOUS", 4), ("DUPLICATE", 8), ("KEPT", 16)):
        assert re.search(r"#define ALGA_CONTAIN_%s\s+%d\b" % (name, value), header)
    assert '"contain_max_blocks"' in header
    for fn in (alga_amd.Engine.drop_contained, alga_amd.Engine.write_kept_fasta, alga_amd.Kept.to_host, alga_amd.Kept.targets, alga_amd.Kept.contain_tsv):
        assert callable(fn)
    for name in ("duplicates", "chain", "short", "t0"):
        assert alga_amd.engine.contain_tsv(QC.checked(name), QC.case(name)["tlen"]).encode() == CC.contain_tsv(QC.checked(name), QC.case(name)["tlen"])
    binary = open(alga_amd.library_path(), "rb").read()
    for k in KERNELS:
        assert k.encode() in binary


def test_new_kernels_resources():
    """The compiler's resource report of contain_kernels.hip: every k_ct_* of the stage is there, no VGPR spill and no scratch in any of them"""
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_contain_resources_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    src = os.path.join(ROOT, "alga_amd", "csrc", "contain_kernels.hip")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    finally:
        if os.path.exists(out):
            os.remove(out)
    lines = r.stderr.splitlines()
    reps = {}
    for i, s in enumerate(lines):
        m = re.search(r"Function Name: \S*?(k_ct_[a-z_]+)E", s)
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
    print({name: {k: v for k, v in rep.items() if "GPR" in k or "Occupancy" in k} for name, rep in reps.items()})
