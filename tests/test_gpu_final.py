"""The final contig set on the GPU (alga_final_contigs_device, alga_contig_trim_device, alga_write_final_fasta_device): every array and every
count equal to the Python definition (tests/final_checker.py) on the hand-made cases of tests/final_cases.py (a ladder of 40 junctions among
them) and on the reference's graph dumps; the trim call against the reference's own values, the oracle on sequences round the cap, every
begin & 15, and a 5 000 000-nt contig; the whole chain on a genome with a repeat; the FASTA against the reference's own files; refusals and
empties; the command line."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import consensus_checker as S
import contig_cases as CC
import final_cases as FC
import final_checker as F
import graph_cases as GC
import oracle_lib as O
import unitig_cases as K

pytestmark = pytest.mark.gpu
KEYS = ("verdict", "rank", "id", "new_reads", "trim_left", "begin", "len", "order")
COUNTS = ("pairs", "n_short", "rejected", "accepted", "trimmed_away", "trim_edges")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what=""):
    for k in ("n_pairs", "n_accepted", "n_written"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
    for k in COUNTS:
        assert got["info"][k] == want["info"][k], (what, k, got["info"][k], want["info"][k])


def device_chain(eng, words, lens, edges, max_offset, min_votes):
    u = eng.contigs(words, lens, edges, max_offset)
    return u, eng.unitig_consensus(words, lens, u, min_votes=min_votes)


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_hand_made_cases(eng, name, tmp_path):
    words, lens, edges, mo = FC.inputs(name)
    case = FC.CASES[name]
    u, c = device_chain(eng, words, lens, edges, mo, 0)
    uh, ch = u.to_host(), c.to_host()
    for trim in (0, 25):
        fin = eng.final_contigs(u, c, case["min_length"], case["percent"], trim)
        got = fin.to_host()
        assert_same(got, F.final_contigs(uh, ch, case["min_length"], case["percent"], trim), (name, trim))
        FC.assert_equals_expected(uh, got, name)                               # (the trim moves window starts; verdicts, new reads and ids stay)
    print(name, fin.info)
    if name == "ladder":
        assert FC.LADDER_JUNCTIONS - 1 <= fin.info["filter_rounds"] <= FC.LADDER_JUNCTIONS + 1
        rungs = [k for k in range(uh["n_pairs"]) if len(FC.name_of(uh, k)) == 3]
        by_rank = sorted(rungs, key=lambda k: got["rank"][k])
        assert [int(got["verdict"][k]) for k in by_rank] == [F.ACCEPTED, F.REJECTED] * 19 + [F.ACCEPTED]
    path = str(tmp_path / "f.fasta")
    info = eng.write_final_fasta(path, fin)
    text, n = F.fasta_bytes(uh, ch, got)
    assert open(path, "rb").read() == text and info["segments"] == n == fin.n_written and info["bytes"] == len(text)


@pytest.mark.parametrize("graph,bound", FC.DUMPS)
@pytest.mark.parametrize("min_votes", FC.MIN_VOTES)
def test_reference_dumps(eng, golden_dir, tmp_path, graph, bound, min_votes):
    words, lens, edges, uw, cw = FC.golden_contigs(golden_dir, graph, bound, min_votes)
    u, c = device_chain(eng, words, lens, edges, bound, min_votes)
    seen, trims = set(), 0
    for min_length, percent in FC.SETTINGS:
        fin = eng.final_contigs(u, c, min_length, percent, 25)
        got = fin.to_host()
        want = F.final_contigs(uw, cw, min_length, percent, 25)
        assert_same(got, want, (graph, min_votes, min_length, percent))
        assert fin.info["filter_rounds"] <= F.verdicts_rounds(uw, cw["len"], min_length, percent)[1]     # (the slowest schedule)
        print(graph, "min_votes", min_votes, (min_length, percent), fin.info, "non-zero trims", int((got["trim_left"] > 0).sum()))
        seen |= set(got["verdict"].tolist())
        trims += int((got["trim_left"] > 0).sum())
        path = str(tmp_path / "f.fasta")
        info = eng.write_final_fasta(path, fin)
        text, n = F.fasta_bytes(uw, cw, want)
        assert open(path, "rb").read() == text and info["segments"] == n
    if graph.startswith("f5") and min_votes == 0:
        assert seen == {F.SHORT, F.REJECTED, F.ACCEPTED, F.TRIMMED_AWAY} and trims > 0


def _n4(golden_dir):
    words, lens = O.load_nodes_bin(os.path.join(golden_dir, "n4_contigs.nodes.bin.gz"))
    want = np.array([int(line.split()[0]) for line in gzip.open(os.path.join(golden_dir, "n4_contigs.trim.txt.gz"), "rt")], dtype=np.int32)
    return words, lens, want


def test_trim_call_gives_the_reference_values(eng, golden_dir):
    words, lens, want = _n4(golden_dir)
    stride = words.shape[1]
    begin = 16 * stride * np.arange(len(lens), dtype=np.int64)
    got = eng.contig_trim_device(words.reshape(-1), begin, lens).cpu().numpy()
    assert (got == want).all() and (want > 0).sum() > 20
    assert (eng.contig_trim(words, lens) == got).all()
    assert eng.contig_trim_device(np.zeros(4, np.uint32), np.zeros(0, np.int64), np.zeros(0, np.int32)).shape == (0,)


def test_trim_call_on_the_cap_set_at_every_shift(eng):
    """the sequences of the CPU test (lengths 1001 .. 1003 and 2000 .. 3500, overlaps 25 .. 501, branches, both strands) laid out ragged, sequence i
    starting at begin & 15 == i mod 16 and, in a second layout, == 15 - i mod 16: the oracle's trim of the sequences as they are"""
    seqs = FC.trim_set()
    want, edges = F.trim_left(seqs, 25)
    assert (want > 0).sum() >= 100
    for shifts in (np.arange(len(seqs)) % 16, 15 - np.arange(len(seqs)) % 16):
        words, begin, lens = FC.ragged(seqs, shifts)
        assert set((begin & 15).tolist()) == set(range(16))
        got = eng.contig_trim_device(words, begin, lens).cpu().numpy()
        assert (got == want).all(), np.nonzero(got != want)[0]
    assert eng.last_trim_edges == F.trim_left(seqs, 25, capped=True)[1]
    small = seqs[:60]
    words, begin, lens = FC.ragged(small, np.arange(len(small)) * 7 % 16)
    for threshold in (60, 501):
        assert (eng.contig_trim_device(words, begin, lens, threshold).cpu().numpy() == F.trim_left(small, threshold)[0]).all(), threshold


def test_trim_call_takes_a_contig_of_five_million_bases(eng):
    rng = np.random.default_rng(9)
    big = rng.integers(0, 4, size=5_000_000, dtype=np.uint8)
    small = np.concatenate([big[-120:], rng.integers(0, 4, size=180, dtype=np.uint8)])
    words, begin, lens = FC.ragged([big, small], [3, 11])
    assert lens.tolist() == [5_000_000, 300]
    got = eng.contig_trim_device(words, begin, lens).cpu().numpy()
    assert got.tolist() == [0, 120]
    rows = alga_amd.pack_reads(np.stack([big, np.concatenate([small, np.zeros(len(big) - 300, np.uint8)])]), lens)
    with pytest.raises(alga_amd.AlgaError):                                    # the host form stops at 4 194 303 nt
        eng.contig_trim(rows, lens)


def test_whole_chain_on_a_genome_with_a_repeat(eng, tmp_path):
    """6 kb with a 400-nt repeat (longer than a read): build -> cut -> contigs -> consensus -> final -> FASTA"""
    r = GC.replicon_reads(circular=[], linear=[6000], n=2400, length=GC.READ_LEN, seed=31, copy=(1000, 4000, 400))
    e = eng.prefsuf_host(r.words, r.lens, GC.MIN_OVERLAP, GC.RSOEMO)
    cut = eng.cut_triangles_host(len(r.lens), e, GC.MOPP)
    u, c = device_chain(eng, r.words, r.lens, cut, GC.MOPP, 0)
    uh, ch = u.to_host(), c.to_host()
    fin = eng.final_contigs(u, c, 150, 95, 25)
    got = fin.to_host()
    want = F.final_contigs(uh, ch, 150, 95, 25)
    assert_same(got, want, "repeat")
    print(fin.info, "lengths", sorted(got["len"][got["verdict"] == F.ACCEPTED].tolist()))
    assert fin.n_written >= 3 and (got["trim_left"] > 0).any() and (got["len"] > 1002).any()
    path = str(tmp_path / "f.fasta")
    eng.write_final_fasta(path, fin)
    text = open(path, "rb").read()
    assert text == F.fasta_bytes(uh, ch, want)[0]
    recs = [x for x in text.decode().split("\n") if x and not x.startswith(">")]
    genome = "".join("ACGT"[b] for b in r.genomes[0])
    for s in recs:
        assert s in genome or S.revcomp(s) in genome
    # the junction reads: first / last entries that more than one pair holds.  Before the trim each is at the end of one contig and at the start
    # of another; in the file none is
    po = uh["path_off"].astype(np.int64)
    ends = np.concatenate([uh["path_node"][po[:-1]], uh["path_node"][po[1:] - 1]]) >> 1
    junction = [int(x) for x in np.unique(ends) if (ends == x).sum() > 1]
    assert junction
    codes = GC.read_codes(r)
    untrimmed = [S.window(uh, ch, k) for k in range(uh["n_pairs"]) if got["verdict"][k] in (F.ACCEPTED, F.TRIMMED_AWAY)]
    doubled = 0
    for j in junction:
        s = "".join("ACGT"[b] for b in codes[j])
        for t in (s, S.revcomp(s)):
            doubled += any(x.endswith(t) for x in untrimmed) and any(x.startswith(t) for x in untrimmed)
            assert not (any(x.endswith(t) for x in recs) and any(x.startswith(t) for x in recs)), j
    assert doubled > 0


def _reference_records(golden_dir, fixture):
    with gzip.open(os.path.join(golden_dir, fixture + ".contigs.fasta.gz"), "rt") as f:
        recs = [x for x in f.read().split(">") if x]
    return [(">" + x.split("\n")[0], "".join(x.split("\n")[1:])) for x in recs]


@pytest.mark.parametrize("fixture", ["f1_cfg1", "f3_paired"])
def test_fasta_is_the_reference_file(eng, golden_dir, tmp_path, fixture):
    words, lens, edges = K.golden(golden_dir, fixture + ".aftersimplifier.graph")
    u, c = device_chain(eng, words, lens, edges, 250, 3)
    fin = eng.final_contigs(u, c, 200, 95, 25)
    path = str(tmp_path / "f.fasta")
    info = eng.write_final_fasta(path, fin)
    (ref_head, ref_seq), = _reference_records(golden_dir, fixture)
    head, seq, rest = open(path).read().split("\n")
    assert info["segments"] == 1 and rest == "" and fin.n_accepted == 1 and fin.info["filter_rounds"] == 0
    assert head == ref_head and (seq == ref_seq or seq == S.revcomp(ref_seq))


def test_refusals_empties_and_what_the_call_leaves_alone(eng, golden_dir, tmp_path):
    words, lens, edges = K.golden(golden_dir, "f2_err2.aftersimplifier.graph")
    u, c = device_chain(eng, words, lens, edges, 262, 0)
    usnap, csnap = u.to_host(), c.to_host()
    fin = eng.final_contigs(u, c, 150, 95, 25)
    snap = fin.to_host()
    assert (snap["trim_left"] > 0).any()
    for k in ("words", "word_off", "len", "path_node", "path_pos", "path_off", "edges"):
        assert (u.to_host()[k] == usnap[k]).all(), k                           # the trim's build leaves the contigs and their consensus alone
    for k in ("words", "trim_left", "len", "changed"):
        assert (c.to_host()[k] == csnap[k]).all(), k
    path = str(tmp_path / "f.fasta")
    for args in ((-1, 95, 25), (150, -1, 25), (150, 101, 25), (150, 95, -1), (150, 95, 502)):
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.final_contigs(u, c, *args)
        assert ei.value.code == -1
        assert_same(fin.to_host(), snap, args)                                 # nothing written: still the engine's current result
        assert eng.write_final_fasta(path, fin)["segments"] == fin.n_written
    with pytest.raises(alga_amd.AlgaError):
        eng.contig_trim_device(np.zeros(4, np.uint32), np.zeros(1, np.int64), np.ones(1, np.int32), 0)
    with pytest.raises(alga_amd.AlgaError):
        eng.contig_trim_device(np.zeros(4, np.uint32), np.zeros(1, np.int64), np.full(1, -1, np.int32), 25)
    # no trim: the windows of the consensus as they are
    plain = eng.final_contigs(u, c, 150, 95, 0)
    got = plain.to_host()
    assert_same(got, F.final_contigs(usnap, csnap, 150, 95, 0), "no trim")
    acc = got["verdict"] == F.ACCEPTED
    assert plain.info["trimmed_away"] == 0 and plain.info["trim_edges"] == 0 and (got["trim_left"] == 0).all()
    assert (got["begin"][acc] == csnap["trim_left"][acc]).all() and (got["len"][acc] == csnap["len"][acc]).all()
    # an empty selection: an empty file
    none = eng.final_contigs(u, c, 10 ** 6, 95, 25)
    assert none.n_accepted == 0 and none.n_written == 0 and none.info["n_short"] == u.n_pairs and none.order.shape == (0,)
    assert eng.write_final_fasta(path, none)["segments"] == 0 and open(path, "rb").read() == b""
    # stale inputs: a new consensus, a new contig call
    c2 = eng.unitig_consensus(words, lens, u, min_votes=0)
    with pytest.raises(alga_amd.AlgaError):
        eng.write_final_fasta(path, none)
    eng.final_contigs(u, c2, 150, 95, 25)
    u2 = eng.contigs(words, lens, edges, 262)
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.final_contigs(u2, c2, 150, 95, 25)
    assert ei.value.code == -1
    # a unitig result shares no read: one round at the most, nothing rejected
    uu = eng.unitigs(words, lens, edges, skip_isolated=True)
    cu = eng.unitig_consensus(words, lens, uu, min_votes=0)
    fu = eng.final_contigs(uu, cu, 1, 95, 0)
    assert fu.info["rejected"] == 0 and fu.info["filter_rounds"] <= 1 and fu.n_accepted == uu.n_pairs
    assert_same(fu.to_host(), F.final_contigs(uu.to_host(), cu.to_host(), 1, 95, 0), "unitigs")
    # an edge list without edges: no pair at all
    w0, l0, e0, mo = CC.inputs("empty_edge_list")
    ue, ce = device_chain(eng, w0, l0, e0, mo, 0)
    fe = eng.final_contigs(ue, ce, 1, 95, 25)
    assert fe.n_pairs == 0 and fe.n_accepted == 0 and eng.write_final_fasta(path, fe)["bytes"] == 0 and open(path, "rb").read() == b""


def test_cli_writes_the_final_contigs(golden_dir, tmp_path):
    """f1 through the command line: build, cut, contigs, consensus, final -- the FASTA is the reference's file up to strand, with or without --contigs="""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    fx = O.Fixture(golden_dir, "f1_cfg1")
    try:
        f1, _ = fx.inputs()
        out = {}
        for name, args in (("both", ["--contigs=c.fasta", "--contigs_final=f.fasta"]), ("final", ["--contigs_final=f.fasta", "--contigs_new_reads_percent=90", "--contigs_trim_threshold=30"]),
                           ("too_long", ["--contigs_final=f.fasta", "--contigs_min_length=30000"])):
            wd = tmp_path / name
            wd.mkdir()
            r = subprocess.run([exe, "--file1=" + f1, "--output=o.fasta"] + args, cwd=str(wd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            assert "Final contigs written" in r.stderr
            out[name] = {f: open(str(wd / f), "rb").read() for f in ("c.fasta", "f.fasta") if (wd / f).exists()}
    finally:
        fx.cleanup()
    (ref_head, ref_seq), = _reference_records(golden_dir, "f1_cfg1")
    for name in ("both", "final"):
        head, seq, rest = out[name]["f.fasta"].decode().split("\n")
        assert head == ref_head and rest == "" and (seq == ref_seq or seq == S.revcomp(ref_seq))
    assert out["both"]["c.fasta"] == out["both"]["f.fasta"] and "c.fasta" not in out["final"]
    assert out["too_long"] == {"f.fasta": b""}
