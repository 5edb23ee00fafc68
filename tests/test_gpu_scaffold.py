"""The scaffolds on the GPU (alga_scaffold_placed_device, alga_write_scaffold_fasta_device): every output array and every counter equal to the
Python definition (tests/scaffold_checker.py) on the cases of tests/scaffold_cases.py, from host arrays and from tensors; the FASTA bytes
and the layout; the planted genome with a polish between; the caller's stream; refusals leave an earlier result valid; a result stays valid
across a later placement and polish; the command line."""
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import place_cases as PC
import place_checker as P
import polish_checker as Q
import scaffold_cases as QC
import scaffold_checker as SC

pytestmark = pytest.mark.gpu
TIMES = ("ms_links", "ms_chain", "ms_total")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what=""):
    for k in SC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert (got[k] == want[k]).all(), (what, k, np.nonzero(got[k] != want[k])[0][:10])
    info = {k: v for k, v in got["info"].items() if k not in TIMES}
    assert info == want["info"], (what, info, want["info"])


def targets(c):
    return c["twords"], c["tbegin"], c["tlen"]


def device_args(c):
    import torch
    t = lambda a, view=None: None if a is None else torch.from_numpy(a.view(view) if view else a).cuda()
    return t(c["rows"], np.int32), t(c["lens"]), (t(c["twords"], np.int32), t(c["tbegin"]), t(c["tlen"])), t(c["pair_off"])


def layout(res):
    return [[(int(c), int(res["orient"][c])) for c in res["s_members"][int(res["s_off"][j]):int(res["s_off"][j + 1])]] for j in range(len(res["s_len"]))]


@pytest.mark.parametrize("name", sorted(QC.CASES))
def test_every_case_equals_the_checker(eng, name, tmp_path):
    c = QC.case(name)
    path = str(tmp_path / "s.fasta")
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"], **c["params"])
    rows, lens, tg, po = device_args(c)
    for i, v in enumerate(c["variants"]):
        want = QC.checked(name, i)
        sc = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl, **v)
        got = sc.to_host()
        assert_same(got, want, (name, i, "host arrays"))
        assert sc.info["pairs_split"] == pl.info["pairs_split"]
        assert (sc.n_targets, sc.n_bundles, sc.n_scaffolds, sc.n_members) == (len(c["tlen"]), len(want["b_a"]), len(want["s_len"]), len(want["s_members"]))
        info = eng.write_scaffold_fasta(path, pl, sc)
        text = open(path, "rb").read()
        assert text == SC.fasta(want, c["seqs"]), (name, i)
        assert info["segments"] == sc.n_scaffolds and info["bytes"] == len(text)
        assert sc.layout_tsv().encode() == SC.layout_tsv(want, c["tlen"]), (name, i)
        print(name, i, sc.info)
    # from tensors: they are used where they are and left untouched
    keep = [x.clone() for x in (rows, lens, *tg)]
    pl = eng.place_reads(rows, lens, targets=tg, pair_off=po, **c["params"])
    before = pl.to_host()
    for i, v in enumerate(c["variants"]):
        sc = eng.scaffold(rows, lens, po, pl, **v)
        assert_same(sc.to_host(), QC.checked(name, i), (name, i, "tensors"))
    for a, b in zip([rows, lens, *tg], keep):
        assert (a == b).all()
    after = pl.to_host()
    assert all((before[k] == after[k]).all() for k in P.ARRAYS)                 # the placement is left as it was


def test_insert_defaults_to_the_placements_median(eng):
    c = QC.case("one_target")
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    assert pl.info["insert_median"] == 300
    assert_same(eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl).to_host(), QC.checked("one_target"), "the median as insert")
    c = QC.case("two")                                                           # no proper pair: no median
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    assert pl.info["insert_median"] == -1
    with pytest.raises(alga_amd.AlgaError):
        eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl)


def test_planted_genome_with_a_polish_between(eng, tmp_path):
    """reads with 1 % substitutions: place -> polish -> scaffold; the sequences of the FASTA are the polished ones"""
    c, g = QC.planted_genome(noisy=True)
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    want_pl = P.place(*PC.args(c))
    pol = eng.polish(c["rows"], c["lens"], pl)
    want_pol = Q.polish_scatter(c["rows"], c["lens"], want_pl, *targets(c))
    sc = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl)
    want = SC.scaffold_dicts(*QC.scaffold_args(c, want_pl), insert=want_pl["info"]["insert_median"])
    got = sc.to_host()
    assert_same(got, want, "planted genome")
    print(pl.info["insert_median"], sc.info)
    assert layout(got) == [QC.PLANTED_TRUTH] and sc.info["joins"] == 2 and (got["b_links"] >= 5).all()
    assert abs(int(got["gap_after"][1]) - 80) <= 100 and abs(int(got["gap_after"][0]) - 60) <= 100
    plain, polished = str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta")
    eng.write_scaffold_fasta(plain, pl, sc)
    eng.write_scaffold_fasta(polished, pl, sc, polished=pol)
    assert open(plain, "rb").read() == SC.fasta(want, c["seqs"])
    assert open(polished, "rb").read() == SC.fasta(want, Q.sequences(want_pol))
    assert (pol.to_host()["words"] == want_pol["words"]).all()
    seq = open(polished).read().split("\n")[1]
    rc = "".join("ACGT"[x] for x in P.revcomp(g))
    truth = rc[:1420] + "N" * int(got["gap_after"][1]) + rc[1500:2740] + "N" * int(got["gap_after"][0]) + rc[2800:]
    assert len(seq) == len(truth)
    # a polish of another placement is refused; so is a scaffold result of another placement
    pl2 = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    for kw in (dict(polished=pol), {}):
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.write_scaffold_fasta(plain, pl2, sc, **kw)
        assert ei.value.code == -1
    sc2 = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl2)
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.write_scaffold_fasta(plain, pl2, sc2, polished=pol)                  # the polish at hand is of the earlier placement
    assert ei.value.code == -1
    eng.write_scaffold_fasta(plain, pl2, sc2)
    assert open(plain, "rb").read() == SC.fasta(want, c["seqs"])


def test_fasta_in_several_chunks(eng, tmp_path):
    """1 MB chunks and more than 2 MB of records: every chunk but the first starts at a record index above 0, and the scaffolds of several
    contigs -- `-` contigs, runs of N -- lie in the later ones"""
    c, want_pl = QC.chunks()
    v = c["variants"][0]
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    got_pl = pl.to_host()
    for k in ("target", "pos", "state", "col_off"):
        assert (got_pl[k] == want_pl[k]).all(), k
    want = SC.scaffold_dicts(*QC.scaffold_args(c, want_pl), **v)
    sc = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl, **v)
    got = sc.to_host()
    assert_same(got, want, "chunks")
    chains = [p for p in layout(got) if len(p) > 1]
    assert chains == [list(x) for x in QC.CHUNK_CHAINS] and int(got["orient"].sum()) == 4 and (got["gap_after"][[20, 33, 22, 35, 30]] >= 10).all()
    text = SC.fasta(want, c["seqs"])
    first = text.index(b">scaffold_id=%d_" % got["scaffold"][20])
    assert len(text) > 2 << 20 and first > 1 << 20                             # the joined scaffolds begin past the first chunk
    a, b = str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta")
    try:
        info = eng.write_scaffold_fasta(a, pl, sc)
        eng.set_option("gfa_chunk_mb", 1)
        info1 = eng.write_scaffold_fasta(b, pl, sc)
    finally:
        eng.set_option("gfa_chunk_mb", 256)
    assert open(b, "rb").read() == text and open(a, "rb").read() == text
    assert info["bytes"] == info1["bytes"] == len(text) and info["segments"] == info1["segments"] == sc.n_scaffolds == CHUNKED_SCAFFOLDS


CHUNKED_SCAFFOLDS = 36 - 5


def test_the_callers_stream(eng):
    import torch
    c, want = QC.case("long_chain"), QC.checked("long_chain")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rows, lens, tg, po = device_args(c)
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    pl = eng.place_reads(rows, lens, targets=tg, pair_off=po, stream=s.cuda_stream, **c["params"])
    sc = eng.scaffold(rows, lens, po, pl, stream=s.cuda_stream, **c["variants"][0])
    assert s.query()                                                             # the call returns with its work on the stream done
    assert_same(sc.to_host(), want, "on the caller's stream")
    sc = eng.scaffold(rows, lens, po, pl, **c["variants"][0])
    assert_same(sc.to_host(), want, "on the engine's stream afterwards")


def test_refusals_leave_an_earlier_result_valid(eng):
    c, want = QC.case("seams"), QC.checked("seams")
    other = QC.case("two")
    stale = eng.place_reads(other["rows"], other["lens"], targets=targets(other), pair_off=other["pair_off"])
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    v0 = c["variants"][0]
    sc = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl, **v0)
    assert_same(sc.to_host(), want, "before")
    host = QC.placed("seams")
    v = int(np.nonzero(host["target"] == 9)[0][0])                               # a read of 25 bases over all of a target of 25

    def lens_with(length):
        a = c["lens"].copy()
        a[2 * v] = a[2 * v + 1] = length
        return a
    bad_pair = c["pair_off"].copy()
    bad_pair[2] = bad_pair[3] = 0                                                # the mate of read 0 does not point back
    big = c["pair_off"].copy()
    big[0] = big[1] = 3
    calls = [dict(rows=other["rows"], lens=other["lens"], pair_off=other["pair_off"], placements=stale),   # a stale placement
             dict(rows=c["rows"][:-2], lens=c["lens"][:-2], pair_off=c["pair_off"][:-2]),                  # n / 2 != n_reads
             dict(rows=c["rows"][:-1], lens=c["lens"][:-1], pair_off=c["pair_off"][:-1]),                  # n odd
             dict(pair_off=bad_pair), dict(pair_off=big),
             dict(lens=lens_with(26)),                                                                     # past the end of its target
             dict(lens=lens_with(33)), dict(lens=lens_with(0)), dict(lens=lens_with(-1)),
             dict(insert=-1), dict(insert=2 ** 20 + 1), dict(max_insert=0), dict(min_links=0), dict(max_second_percent=0), dict(max_second_percent=101),
             dict(min_gap=0), dict(min_gap=2 ** 20 + 1)]
    for change in calls:
        a = dict(dict(rows=c["rows"], lens=c["lens"], pair_off=c["pair_off"], placements=pl, **v0), **change)
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.scaffold(a["rows"], a["lens"], a["pair_off"], a["placements"], **{k: a[k] for k in v0})
        assert ei.value.code == -1, (list(change), ei.value)
        assert_same(sc.to_host(), want, ("after a refusal", list(change)))       # nothing written: the earlier result as it was
    # the target and position branches of the device check, reached by writing through the zero-copy views of the placement
    for view, value in ((pl.target, len(c["tlen"])), (pl.target, -1), (pl.pos, -1), (pl.pos, 1)):
        keep = int(view[v])
        view[v] = value
        try:
            with pytest.raises(alga_amd.AlgaError) as ei:
                eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl, **v0)
            assert ei.value.code == -1, (value, ei.value)
        finally:
            view[v] = keep
        assert_same(sc.to_host(), want, ("after a refusal on the device", value))
    again = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl, **v0)
    assert_same(again.to_host(), want, "the engine afterwards")


def test_a_result_stays_valid_across_a_later_placement_and_polish(eng, tmp_path):
    c, want = QC.case("orient"), QC.checked("orient")
    other = QC.case("ring3")
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    sc = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl, **c["variants"][0])
    pl2 = eng.place_reads(other["rows"], other["lens"], targets=targets(other), pair_off=other["pair_off"])
    eng.polish(other["rows"], other["lens"], pl2)
    assert_same(sc.to_host(), want, "after a later placement and polish")
    assert sc.layout_tsv().encode() == SC.layout_tsv(want, c["tlen"])
    with pytest.raises(alga_amd.AlgaError) as ei:                                # but its FASTA needs the placement it was made from
        eng.write_scaffold_fasta(str(tmp_path / "s.fasta"), pl2, sc)
    assert ei.value.code == -1


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, c in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in c)))


def codes(s):
    return np.array(["ACGT".index(x) for x in s], dtype=np.uint8)


def test_command_line(tmp_path):
    """paired reads of a 6 kb genome with two stretches no read covers, through alga_hip: --scaffolds= and --scaffold_layout= against the
    checker on the contigs the run writes"""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    rng = np.random.default_rng(91)
    g = rng.integers(0, 4, size=6000, dtype=np.uint8)
    holes = ((1900, 1960), (4000, 4080))
    m1, m2 = [], []
    for a in rng.permutation(np.arange(0, 6000 - 400, 2)):
        ins = int(rng.integers(300, 401))
        pair = []
        for lo in (a, a + ins - 100):
            if any(lo < h1 and lo + 100 > h0 for h0, h1 in holes):
                break
            pair.append(lo)
        if len(pair) == 2:
            m1.append(g[pair[0]:pair[0] + 100])
            m2.append(P.revcomp(g[pair[1]:pair[1] + 100]))
    _write_fasta(str(tmp_path / "a.fasta"), m1)
    _write_fasta(str(tmp_path / "b.fasta"), m2)
    base = [exe, "--file1=a.fasta", "--file2=b.fasta", "--output=o.fasta", "--contigs_final=f.fasta", "--contigs_min_length=150", "--consensus_min_votes=0", "--retl=0", "--retr=0"]
    r = subprocess.run(base + ["--scaffolds=s.fasta", "--scaffold_layout=l.tsv", "--scaffold_min_links=4"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Reads placed on the final contigs" in r.stderr and "Scaffolds:" in r.stderr, r.stderr[-2000:]
    for bad in (["--file1=a.fasta", "--file2=b.fasta", "--output=o.fasta", "--scaffolds=s2.fasta"],
                ["--file1=a.fasta", "--output=o.fasta", "--contigs_final=f2.fasta", "--scaffolds=s2.fasta"],
                ["--file1=a.fasta", "--file2=b.fasta", "--output=o.fasta", "--contigs_final=f2.fasta", "--scaffold_layout=l2.tsv"]):
        rb = subprocess.run([exe] + bad, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert rb.returncode == 2 and "needs" in rb.stderr
    contigs = open(str(tmp_path / "f.fasta")).read().split("\n")
    ids = [int(h.split("=")[1].split("_")[0]) for h in contigs[0::2] if h]
    tg = [np.zeros(0, np.uint8)] * (max(ids) + 1)
    for j, s in zip(ids, [codes(s) for s in contigs[1::2] if s]):
        tg[j] = s
    rows, lens = P.nodes_of([x for pair in zip(m1, m2) for x in pair])
    pair_off = np.array([1, 1, 2, 2] * len(m1), dtype=np.uint8)
    tw, tb, tl = P.ragged(tg, [0] * len(tg))
    pl = P.place(rows, lens, pair_off, tw, tb, tl)
    want = SC.scaffold_dicts(rows, lens, pair_off, pl, insert=pl["info"]["insert_median"], min_links=4)
    print(want["info"], r.stderr[-600:])
    assert want["info"]["joins"] >= 2 and want["info"]["scaffolds_multi"] >= 1
    assert open(str(tmp_path / "s.fasta"), "rb").read() == SC.fasta(want, tg)
    assert open(str(tmp_path / "l.tsv"), "rb").read() == SC.layout_tsv(want, tl)
    i = want["info"]
    said = "%d links, %d bundles supported, %d joins, %d scaffolds (%d of several contigs), N50 %d -> %d" % (
        i["links"], i["bundles_supported"], i["joins"], i["scaffolds"], i["scaffolds_multi"], i["n50_targets"], i["n50_scaffolds"])
    assert said in r.stderr, r.stderr[-2000:]
