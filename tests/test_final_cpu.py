"""The final contig set without a GPU: the library exports the three calls, the structs have the header's sizes, the compiler's resource report
of final_kernels.hip; the Python definition (tests/final_checker.py) gives the answers written out in tests/final_cases.py; its sequential form
equals its round form on every hand-made case and on the reference's graph dumps; the trim of the sequences as they are equals the trim of
their cap form (the first and last 501 nt) through the oracle's creator."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alga_amd
import consensus_checker as S
import contig_checker as CT
import final_cases as FC
import final_checker as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_fc_len_check", "k_fc_gather", "k_fc_rank_keys", "k_fc_init", "k_fc_round_min", "k_fc_round_decide", "k_fc_accept_flags", "k_fc_number",
           "k_fc_apply_trim", "k_fc_fasta_sizes", "k_fc_fasta_write"]
_hand = {}


def hand_made(name):
    """contigs and whole-contig windows of a hand-made case, one checker run per case (read only)"""
    if name not in _hand:
        words, lens, edges, mo = FC.inputs(name)
        u = CT.contigs(words, lens, edges, mo)
        _hand[name] = (u, S.consensus_pileup(words, lens, u, 0))
    return _hand[name]


def test_library_exports_the_calls_and_the_engine_has_the_methods():
    lib = alga_amd.load_library()
    for sym in ("alga_contig_trim_device", "alga_final_contigs_device", "alga_write_final_fasta_device"):
        assert hasattr(lib, sym) and sym in alga_amd.engine.EXPORTS
    for m in ("contig_trim_device", "final_contigs", "write_final_fasta"):
        assert callable(getattr(alga_amd.Engine, m))
    assert lib.alga_abi_version() == 7                                       # the calls only add to the ABI
    hdr = open(os.path.join(ROOT, "include", "alga_amd.h")).read()
    for k, v in (("SHORT", F.SHORT), ("REJECTED", F.REJECTED), ("ACCEPTED", F.ACCEPTED), ("TRIMMED_AWAY", F.TRIMMED_AWAY)):
        assert int(re.search(r"#define\s+ALGA_FINAL_%s\s+(\d+)" % k, hdr).group(1)) == v == getattr(alga_amd.engine, "FINAL_" + k)
    # alga_final_contigs: four ints, eight pointers; alga_final_info: seven counts, three times
    assert C.sizeof(alga_amd.engine.FinalContigsC) == 4 * 4 + 8 * 8
    assert C.sizeof(alga_amd.engine.FinalInfo) == 8 * (7 + 3)
    binary = open(alga_amd.library_path(), "rb").read()
    for k in KERNELS:
        assert k.encode() in binary


def test_new_kernels_resources():
    """The compiler's resource report of final_kernels.hip: no VGPR spill and no scratch in any kernel"""
    src = os.path.join(ROOT, "alga_amd", "csrc", "final_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_final_resources_%d.o" % os.getpid())
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
        m = re.search(r"Function Name: \S*?(k_fc_[a-z_]+?)E[A-Z]", s)
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


def test_the_double_test_is_the_integer_test():
    """100.0 * ((double) new / all) < percent agrees with 100 * new < percent * all wherever the filter can ask: new >= all - 2 (sampled over all
    <= 4 * 10^6, every value below 3000), every per cent value"""
    alls = np.unique(np.concatenate([np.arange(1, 3000), np.random.default_rng(1).integers(3000, 4000001, size=3000)])).astype(np.int64)
    for d in (0, 1, 2):
        new = alls - d
        ok = new >= 0
        ratio = new[ok].astype(np.float64) / alls[ok].astype(np.float64)
        for percent in range(101):
            assert ((100.0 * ratio < float(percent)) == (100 * new[ok] < percent * alls[ok])).all(), (d, percent)
    assert not F.rejects(19, 20, 95) and not F.rejects(38, 40, 95) and F.rejects(18, 19, 95) and F.rejects(37, 39, 95)


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_checker_gives_the_answers_written_out(name):
    u, c = hand_made(name)
    case = FC.CASES[name]
    seq = F.verdicts_sequential(u, c["len"], case["min_length"], case["percent"])
    FC.assert_equals_expected(u, seq, name)
    assert sorted(int(x) for x in seq["id"] if x >= 0) == list(range(len(seq["order"])))
    assert [int(seq["id"][k]) for k in seq["order"]] == list(range(len(seq["order"])))


def assert_same_verdicts(a, b, what):
    for k in ("verdict", "rank", "id", "new_reads", "order"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and (a[k] == b[k]).all(), (what, k)


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_round_form_equals_sequential_form_on_the_hand_made_cases(name):
    u, c = hand_made(name)
    for min_length, percent in [(FC.CASES[name]["min_length"], FC.CASES[name]["percent"])] + FC.SETTINGS:
        rnd, rounds = F.verdicts_rounds(u, c["len"], min_length, percent)
        assert_same_verdicts(F.verdicts_sequential(u, c["len"], min_length, percent), rnd, (name, min_length, percent))
        if name == "ladder" and (min_length, percent) == (1, 95):
            assert FC.LADDER_JUNCTIONS - 1 <= rounds <= FC.LADDER_JUNCTIONS + 1   # rung i waits for rung i - 1


@pytest.mark.parametrize("graph,bound", FC.DUMPS)
@pytest.mark.parametrize("min_votes", FC.MIN_VOTES)
def test_round_form_equals_sequential_form_on_the_dumps(golden_dir, graph, bound, min_votes):
    words, lens, edges, u, c = FC.golden_contigs(golden_dir, graph, bound, min_votes)
    seen = set()
    for min_length, percent in FC.SETTINGS:
        seq = F.verdicts_sequential(u, c["len"], min_length, percent)
        rnd, rounds = F.verdicts_rounds(u, c["len"], min_length, percent)
        assert_same_verdicts(seq, rnd, (graph, min_votes, min_length, percent))
        seen |= set(seq["verdict"].tolist())
        print(graph, "min_votes", min_votes, (min_length, percent), "pairs", u["n_pairs"], "short/rejected/accepted",
              [int((seq["verdict"] == v).sum()) for v in (F.SHORT, F.REJECTED, F.ACCEPTED)], "rounds", rounds)
    if graph.startswith("f5") and min_votes == 0:                          # (at 3 votes the thin coverage of f5 leaves 8 windows)
        assert seen == {F.SHORT, F.REJECTED, F.ACCEPTED}


def test_only_end_entries_are_shared(golden_dir):
    """what the round form rests on: in a contig result a read index that lies in two pairs is the first or the last entry in both"""
    for graph, bound in FC.DUMPS:
        u = FC.golden_contigs(golden_dir, graph, bound, 0)[3]
        po = u["path_off"].astype(np.int64)
        reads = u["path_node"].astype(np.int64) >> 1
        pair = np.repeat(np.arange(u["n_pairs"]), np.diff(po))
        inner = np.ones(len(reads), dtype=bool)
        inner[po[:-1]] = False
        inner[po[1:] - 1] = False
        owner = {}
        for r, k in zip(reads[inner].tolist(), pair[inner].tolist()):
            assert owner.setdefault(r, k) == k
        ends = set(reads[~inner].tolist())
        assert not ends & set(owner)


def test_trim_of_the_cap_form_is_the_trim(golden_dir):
    """O.prefsuf on the sequences as they are against their first and last 501 nt: the same trim_left, with lengths at the cap and round it,
    overlaps of 25 .. 501, branches and both strands"""
    seqs = FC.trim_set()
    lens = np.array([len(s) for s in seqs])
    assert {1001, 1002, 1003} <= set(lens.tolist()) and (lens >= 2000).sum() > 50 and lens.max() <= 3500
    full, _ = F.trim_left(seqs, 25)
    capped, _ = F.trim_left(seqs, 25, capped=True)
    assert (full == capped).all(), np.nonzero(full != capped)[0]
    print("contigs", len(seqs), "non-zero trims", int((full > 0).sum()), "largest", int(full.max()))
    assert (full > 0).sum() >= 100
    assert full.max() >= 490 and full[full > 0].min() <= 30                    # both ends of the overlap range occur
    # and the reference's own values: the n4 golden contigs in the cap form
    import oracle_lib as O
    import gzip
    words, glens = O.load_nodes_bin(os.path.join(golden_dir, "n4_contigs.nodes.bin.gz"))
    want = np.array([int(line.split()[0]) for line in gzip.open(os.path.join(golden_dir, "n4_contigs.trim.txt.gz"), "rt")], dtype=np.int32)
    g = [F.codes_of(words[i], 0, glens[i]) for i in range(len(glens))]
    assert (F.trim_left(g, 25, capped=True)[0] == want).all()


def test_final_contigs_of_the_checker_on_f5(golden_dir):
    """the whole definition on the messy fixture: every verdict occurs, some trims are non-zero, the cap form gives the same result, the FASTA
    holds one record per accepted pair in id order"""
    words, lens, edges, u, c = FC.golden_contigs(golden_dir, "f5_messy.aftercut.graph", 250, 0)
    fin = F.final_contigs(u, c, 150, 95, 25)
    cap = F.final_contigs(u, c, 150, 95, 25, capped=True)
    for k in ("verdict", "trim_left", "begin", "len", "id", "order"):
        assert (fin[k] == cap[k]).all(), k
    print({k: v for k, v in fin["info"].items()}, "non-zero trims", int((fin["trim_left"] > 0).sum()))
    assert fin["info"]["n_short"] > 0 and fin["info"]["rejected"] > 0 and fin["info"]["accepted"] > 0
    assert (fin["trim_left"] > 0).sum() > 0
    text, n = F.fasta_bytes(u, c, fin)
    heads = [x for x in text.decode().split("\n") if x.startswith(">")]
    assert n == fin["n_written"] == len(heads)
    ids = [int(h.split("=")[1].split("_")[0]) for h in heads]
    assert ids == sorted(ids) and set(ids) == {int(fin["id"][k]) for k in range(u["n_pairs"]) if fin["verdict"][k] == F.ACCEPTED}


def test_refusals():
    u, c = hand_made("fork")
    for args in ((-1, 95, 25), (1, -1, 25), (1, 101, 25), (1, 95, -1), (1, 95, 502)):
        with pytest.raises(ValueError):
            F.final_contigs(u, c, *args)
