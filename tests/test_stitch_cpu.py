"""The stitch stage without a GPU: the two Python statements of the definition (tests/stitch_checker.py) agree on the cases of
tests/stitch_cases.py and on seeded random families (planted chains cut with overlaps of 8 .. 600, 0 .. 3 mismatches, random orientations,
decoy entries); the outcomes the cases were made for; the refusals of the checker; the header declares the calls and the binding knows them."""
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import merge_checker as MC
import place_checker as P
import stitch_cases as SQ
import stitch_checker as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_st_targets", "k_st_check", "k_st_overlap", "k_st_joins", "k_st_dropped"]
SYMBOLS = ("alga_stitch_default_params", "alga_stitch_targets_device", "alga_stitch_scaffolds_device", "alga_write_stitched_fasta_device")
# (selected, with_overlap, ambiguous, stitched, dropped_cycle, contigs) of every variant of every case
OUTCOMES = {"pairings": [(4, 4, 0, 4, 0, 5), (4, 0, 0, 0, 0, 9)], "half_length": [(2, 1, 0, 1, 0, 3)], "max_overlap": [(2, 1, 0, 1, 0, 3), (2, 2, 0, 2, 0, 2)],
            "full_window": [(3, 3, 0, 3, 0, 3), (3, 1, 0, 1, 0, 5)], "partial_word": [(6, 6, 0, 6, 0, 6)], "funnel": [(16, 16, 0, 16, 0, 16)], "passes": [(3, 3, 1, 2, 0, 4), (3, 3, 0, 3, 0, 3), (3, 3, 1, 2, 0, 4)],
            "mismatches": [(7, 5, 0, 5, 0, 9), (7, 1, 0, 1, 0, 13), (7, 3, 0, 3, 0, 11), (7, 7, 0, 7, 0, 7)], "short": [(1, 1, 0, 1, 0, 1)],
            "two_partners": [(1, 1, 0, 1, 0, 2)], "periodic": [(1, 1, 1, 0, 0, 2), (1, 1, 0, 1, 0, 1), (1, 1, 0, 1, 0, 1), (1, 1, 1, 0, 0, 2)],
            "gap_extremes": [(3, 0, 0, 0, 0, 6), (3, 0, 0, 0, 0, 6)], "homopolymer": [(1, 1, 1, 0, 0, 2), (1, 1, 1, 0, 0, 2), (1, 1, 1, 0, 0, 2), (1, 1, 0, 1, 0, 1)],
            "unselected": [(3, 3, 0, 3, 0, 5)], "path5": [(4, 4, 0, 4, 0, 1)], "ring3": [(3, 3, 0, 2, 1, 1)], "ring2": [(2, 2, 0, 1, 1, 1)], "tiny": [(4, 1, 0, 1, 0, 4)],
            "t0": [(0, 0, 0, 0, 0, 0)], "j0": [(0, 0, 0, 0, 0, 2)], "none_selected": [(0, 0, 0, 0, 0, 2)]}


def assert_same(got, want, what=""):
    for k in ST.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k, got[k], want[k])
    assert got["info"] == want["info"], (what, got["info"], want["info"])


@pytest.mark.parametrize("name,i", SQ.every())
def test_the_two_statements_agree(name, i):
    c, want = SQ.case(name), SQ.checked(name, i)
    assert_same(ST.stitch_literal(c["seqs"], c["entries"], **c["variants"][i]), want, (name, i))
    info = want["info"]
    assert tuple(info[k] for k in ("selected", "with_overlap", "ambiguous", "stitched", "dropped_cycle", "contigs")) == OUTCOMES[name][i], (name, i, info)
    assert len(c["tbegin"]) < 2 or sorted(set((c["tbegin"] & 15).tolist())) == sorted(set(3 * t % 16 for t in range(len(c["tbegin"]))))
    # what holds for every result: every base of every target with a length is in the result once or, where overlapped, twice
    assert info["columns_after"] == info["columns_before"] - info["bases_removed"] and info["contigs"] == len(want["len"])
    assert (want["j_state"][want["j_hits"] == 1] & ST.STITCHED | want["j_state"][want["j_hits"] == 1] & ST.DROPPED_CYCLE).all()
    print(name, i, info)


def test_every_case_is_listed():
    assert sorted(OUTCOMES) == sorted(SQ.CASES) and all(len(OUTCOMES[n]) == len(SQ.case(n)["variants"]) for n in SQ.CASES)


def test_outcomes_the_cases_were_made_for():
    # o = min_overlap in the four pairings of ends
    w = SQ.checked("pairings")
    assert w["j_olen"].tolist() == [16] * 4 and w["j_hits"].tolist() == [1] * 4 and w["orient"].tolist()[:8] == [0, 0, 0, 1, 1, 0, 1, 1]
    assert w["end_entry"].tolist() == [-1, 0, 0, -1, -1, 1, -1, 1, 2, -1, 2, -1, 3, -1, -1, 3, -1, -1, -1, -1]
    assert (SQ.checked("pairings", 1)["j_state"] == ST.SELECTED).all()
    # n = 2 o is stitched, n = 2 o - 1 is not: its window has 49 bases
    assert SQ.checked("half_length")["j_olen"].tolist() == [50, 0] and SQ.case("half_length")["tlen"].tolist() == [300, 100, 300, 99]
    assert SQ.checked("max_overlap")["j_olen"].tolist() == [64, 0] and SQ.checked("max_overlap", 1)["j_olen"].tolist() == [64, 65]
    assert SQ.checked("partial_word")["j_olen"].tolist() == [47, 48, 49, 17, 31, 33]
    # windows of 4096 bases, the largest
    w = SQ.checked("full_window")
    assert w["j_olen"].tolist() == [4096, 4095, 16] and w["j_mm"].tolist() == [2, 0, 0] and SQ.checked("full_window", 1)["j_olen"].tolist() == [0, 0, 16]
    # every shift of the word pair
    w, c = SQ.checked("funnel"), SQ.case("funnel")
    assert w["j_olen"].tolist() == [40] * 16 and sorted((min(int(c["tlen"][2 * r]), int(c["tlen"][2 * r + 1])) // 2 - 40) % 16 for r in range(16)) == list(range(16))
    assert w["j_mm"].tolist() == [1 if r % 3 == 0 else 0 for r in range(16)]
    # second passes; the better candidate a pass later than the worse one
    w = SQ.checked("passes")
    assert w["j_olen"].tolist() == [80, 81, 81] and w["j_mm"].tolist() == [0, 0, 0] and w["j_hits"].tolist() == [1, 1, 2]
    assert w["j_state"].tolist() == [ST.SELECTED | ST.HAS_OVERLAP | ST.STITCHED] * 2 + [ST.SELECTED | ST.HAS_OVERLAP | ST.AMBIGUOUS]
    w = SQ.checked("passes", 1)                                                  # slack 0: of the third entry (gap -20) o = 20 alone is left
    assert w["j_olen"].tolist() == [80, 81, 20] and w["j_mm"].tolist() == [0, 0, 1] and w["j_hits"].tolist() == [1, 1, 1] and w["info"]["candidates_outside_slack"] == 1
    w = SQ.checked("passes", 2)                                                  # slack 61 = |gap + 81|: o = 81 of the third entry is admissible again
    assert w["j_olen"].tolist() == [80, 81, 81] and w["j_hits"].tolist() == [1, 1, 2]
    # mismatches in the first, the last, both, three columns, none, the two of the last word, three around the word bounds
    assert [SQ.checked("mismatches", i)["j_mm"].tolist() for i in range(4)] == [[1, 1, 2, 0, 0, 2, 0], [0] * 7, [1, 1, 0, 0, 0, 0, 0], [1, 1, 2, 3, 0, 2, 3]]
    assert [SQ.checked("mismatches", i)["j_olen"].tolist() for i in (0, 1)] == [[50, 50, 50, 0, 50, 50, 0], [0, 0, 0, 0, 50, 0, 0]]
    # an overlap of 20: merge refuses it (and so it would however many rounds follow), stitch joins
    c = SQ.case("short")
    assert MC.merge_index(c["seqs"])["info"]["joins"] == 0 and SQ.checked("short")["info"]["stitched"] == 1 and SQ.checked("short")["len"].tolist() == [760]
    # two partners: merge leaves the end ambiguous, the entry decides
    c, w = SQ.case("two_partners"), SQ.checked("two_partners")
    m = MC.merge_index(c["seqs"])
    assert m["end_state"][1] == MC.HAS_OVERLAP | MC.AMBIGUOUS and m["info"]["joins"] == 0
    assert w["j_olen"].tolist() == [60] and w["s_members"].tolist() == [0, 1, 2] and w["len"].tolist() == [500, 240]
    # a periodic end: seven o at the one partner; the slack decides
    assert [(int(SQ.checked("periodic", i)["j_hits"][0]), int(SQ.checked("periodic", i)["j_olen"][0])) for i in range(4)] == [(7, 80), (1, 70), (1, 70), (3, 80)]
    assert [SQ.checked("periodic", i)["info"]["candidates_outside_slack"] for i in range(4)] == [0, 6, 6, 4]
    # gap + o in 64 bits
    w = SQ.checked("gap_extremes")
    assert (w["j_state"] == ST.SELECTED).all() and w["info"]["candidates_outside_slack"] == 3
    # hits saturate
    assert [(int(SQ.checked("homopolymer", i)["j_hits"][0]), SQ.checked("homopolymer", i)["info"]["hits_saturated"]) for i in range(4)] == [(255, 1), (255, 1), (255, 1), (1, 0)]
    assert SQ.checked("homopolymer", 3)["len"].tolist() == [1300] and SQ.checked("homopolymer")["j_olen"].tolist() == [350]
    # unselected entries count nowhere
    w = SQ.checked("unselected")
    assert w["j_state"].tolist() == [11, 0, 0, 0, 11, 11, 0, 0] and w["info"]["entries"] == 8
    # five in a row, as the merge stage lays them out
    w, c = SQ.checked("path5"), SQ.case("path5")
    assert w["s_members"].tolist() == [1, 4, 2, 0, 3] and w["orient"].tolist() == [1, 0, 0, 0, 1] and w["start"].tolist() == [500, 0, 450, 740, 250]
    assert w["overlap_after"].tolist() == [60, 50, 50, 0, 50] and (ST.sequences(w)[0] == c["g"]).all()
    # rings through a raw list: opened at contig 0, the entry at its left end is dropped
    w = SQ.checked("ring3")
    assert w["j_state"].tolist() == [11, 11, 3 | ST.DROPPED_CYCLE] and w["s_members"].tolist() == [0, 1, 2] and w["len"].tolist() == [650]
    w = SQ.checked("ring2")
    assert w["j_state"].tolist() == [3 | ST.DROPPED_CYCLE, 11] and w["len"].tolist() == [450]
    # W below min_overlap
    assert SQ.checked("tiny")["j_state"].tolist() == [11, 1, 1, 1] and SQ.checked("tiny")["stitched"].tolist() == [0, 0, -1, 1, 2, 3]
    # no entry: the targets unchanged, as a target set
    w, c = SQ.checked("j0"), SQ.case("j0")
    assert w["len"].tolist() == [77, 130] and all((a == b).all() for a, b in zip(ST.sequences(w), (c["seqs"][0], c["seqs"][2])))


def family(seed):
    """a genome cut into a chain of contigs with overlaps of 8 .. 600 (or a gap), 0 .. 3 mismatches in an overlap, random orientations and
    ids; an entry per cut with a gap near the truth; decoy entries between unrelated ends, unselected entries with anything in them"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 7))
    g = rng.integers(0, 4, size=n * 1500, dtype=np.uint8)
    cuts, at = [], 0
    pieces = []
    for i in range(n):
        length = int(rng.integers(40, 1400))
        pieces.append([at, at + length])
        o = int(rng.choice([8, 15, 16, 17, 31, 32, 33, 64, 100, 600, int(rng.integers(8, 601)), -5]))
        cuts.append(o)
        at = max(at + length - o, at + 1)
    order = rng.permutation(n)
    flip = rng.integers(0, 2, size=n)
    seqs = [None] * n
    for i, (lo, hi) in enumerate(pieces):
        s = g[lo:hi].copy()
        if i and cuts[i - 1] > 0:
            for q in rng.integers(0, min(cuts[i - 1], len(s)), size=int(rng.integers(0, 4))):
                s[q] = (s[q] + 1) & 3
        seqs[order[i]] = P.revcomp(s) if flip[i] else s
    a, b, gap, state = [], [], [], []
    for i in range(n - 1):
        x, y = 2 * order[i] + (1 - flip[i]), 2 * order[i + 1] + flip[i + 1]     # the right end of piece i, the left end of piece i + 1
        if rng.random() < 0.5:
            x, y = y, x
        a.append(x), b.append(y), gap.append(-cuts[i] + int(rng.integers(-3, 4))), state.append(3 if rng.random() < 0.85 else int(rng.choice([0, 1, 7])))
    free = [2 * order[0] + flip[0], 2 * order[n - 1] + (1 - flip[n - 1])]
    if rng.random() < 0.5:
        a.append(free[0]), b.append(free[1]), gap.append(-20), state.append(3)      # a decoy between the two ends of the chain
    for _ in range(int(rng.integers(0, 3))):
        a.append(int(rng.integers(0, 4 * n))), b.append(int(rng.integers(0, 4 * n))), gap.append(int(rng.integers(-100, 100))), state.append(int(rng.choice([0, 1, 6])))
    perm = rng.permutation(len(a))
    entries = ST.entries_of(*[[v[j] for j in perm] for v in (a, b, gap, state)])
    params = dict(max_mismatches=int(rng.integers(0, 4)), min_overlap=int(rng.choice([8, 16, 17, 32])), max_overlap=int(rng.choice([64, 512, 600, 4096])),
                  slack=int(rng.choice([0, 3, 50, 2 ** 20])))
    params["max_overlap"] = max(params["max_overlap"], params["min_overlap"])
    return seqs, entries, params


@pytest.mark.parametrize("seed", range(40))
def test_seeded_families(seed):
    seqs, entries, params = family(1000 + seed)
    want = ST.stitch_windows(seqs, entries, **params)
    assert_same(ST.stitch_literal(seqs, entries, **params), want, seed)
    every = entries[:3] + (None,)                                                # the same list without a state: all selected, where that is no refusal
    if _acceptable(seqs, every, params):
        assert_same(ST.stitch_literal(seqs, every, **params), ST.stitch_windows(seqs, every, **params), (seed, "state None"))
    print(seed, params, want["info"])


def _acceptable(seqs, entries, params):
    try:
        ST.check(seqs, entries, **dict(ST.DEFAULT, **params))
        return True
    except ValueError:
        return False


def test_the_families_reach_what_they_are_for():
    tot = dict.fromkeys(ST.COUNTERS, 0)
    for seed in range(40):
        seqs, entries, params = family(1000 + seed)
        for k, v in ST.stitch_windows(seqs, entries, **params)["info"].items():
            tot[k] += v
    print(tot)
    assert tot["stitched"] >= 20 and tot["join_mismatches"] >= 5 and tot["candidates_outside_slack"] >= 3 and tot["longest_overlap"] and tot["contigs_multi"] >= 10
    assert tot["selected"] < tot["entries"] and tot["with_overlap"] > tot["stitched"] - 1


def test_refusals():
    c = SQ.case("pairings")
    seqs, (a, b, gap, _) = c["seqs"], c["entries"]
    T = len(seqs)
    for bad in (dict(max_mismatches=-1), dict(max_mismatches=255), dict(min_overlap=7), dict(min_overlap=513), dict(max_overlap=15), dict(max_overlap=4097), dict(slack=-1),
                dict(slack=2 ** 20 + 1)):
        for f in (ST.stitch_windows, ST.stitch_literal):
            with pytest.raises(ValueError):
                f(seqs, c["entries"], **bad)
    for ea, eb in (([2 * T], [0]), ([0], [2 * T]), ([4], [5]), ([3], [3]), (list(a) + [int(a[0])], list(b) + [2 * T - 1])):
        e = ST.entries_of(ea, eb, [0] * len(ea))
        for f in (ST.stitch_windows, ST.stitch_literal):
            with pytest.raises(ValueError):
                f(seqs, e, **{})
        ok = ST.entries_of(ea, eb, [0] * len(ea), [1] * len(ea))                # unselected: nothing of them is checked
        assert ST.stitch_windows(seqs, ok)["info"]["selected"] == 0
    with pytest.raises(ValueError):
        ST.check_lengths([5, -1])
    with pytest.raises(OverflowError):
        ST.check([range(0)] * 0 + [_Long()] * 3, ST.entries_of(), **ST.DEFAULT)


class _Long:
    def __len__(self):
        return 2 ** 31 - 1


def test_the_header_and_the_binding_know_the_calls():
    header = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    lib = alga_amd.load_library()
    for s in SYMBOLS:
        assert s + "(" in header and hasattr(lib, s), s
    for k, v in (("ALGA_STITCH_SELECTED", 1), ("ALGA_STITCH_HAS_OVERLAP", 2), ("ALGA_STITCH_AMBIGUOUS", 4), ("ALGA_STITCH_STITCHED", 8), ("ALGA_STITCH_DROPPED_CYCLE", 16)):
        assert "#define %s" % k in header and getattr(alga_amd.engine, k[5:]) == v == getattr(ST, k[12:])
    assert [f for f, _ in alga_amd.StitchParams._fields_] == ["max_mismatches", "min_overlap", "max_overlap", "slack", "flags", "reserved"]
    assert "#define ALGA_AMD_ABI_VERSION 7" in header and lib.alga_abi_version() == 7                    # the calls add
    assert alga_amd.Stitched.stitch_tsv and alga_amd.engine.stitch_tsv
    w, c = SQ.checked("path5"), SQ.case("path5")
    assert alga_amd.engine.stitch_tsv(w, c["tlen"]).encode() == ST.stitch_tsv(w, c["tlen"]) and ST.stitch_tsv(w, c["tlen"]).count(b"\n") == 5
    assert ST.fasta(w).startswith(b">contig_id=0_length=1000_contigs=5\n")


def test_new_kernels_resources():
    """The compiler's resource report of stitch_kernels.hip: every k_st_* is there, no VGPR spill and no scratch in any of them; k_st_overlap holds
    its four waves' windows in LDS (256 + 257 words each) and no other kernel has any"""
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_stitch_resources_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    src = os.path.join(ROOT, "alga_amd", "csrc", "stitch_kernels.hip")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    finally:
        if os.path.exists(out):
            os.remove(out)
    lines = r.stderr.splitlines()
    reps = {}
    for i, s in enumerate(lines):
        m = re.search(r"Function Name: \S*?(k_st_[a-z_]+)E", s)
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
        assert int(rep["LDS Size [bytes/block]"]) == (4 * (256 + 257) * 4 if name == "k_st_overlap" else 0), (name, rep)
    print({k: (v["VGPRs"], v["Occupancy [waves/SIMD]"]) for k, v in reps.items()})
