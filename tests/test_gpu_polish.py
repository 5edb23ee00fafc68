"""The polish on the GPU (alga_polish_placed_device, alga_write_polished_fasta_device): every output array and every counter equal to the
Python definition (tests/polish_checker.py) on the cases of tests/polish_cases.py, from host arrays and from tensors, with and without the
counts; the caller's stream; refusals leave an earlier result valid; a second round on the polished targets; the whole chain on a genome
with a repeat and 1 % substitutions in the reads; the command line."""
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import graph_cases as GC
import place_checker as P
import polish_cases as QC
import polish_checker as Q

pytestmark = pytest.mark.gpu
TIMES = ("ms_sort", "ms_vote", "ms_total")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what="", counts=False):
    for k in Q.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert (got[k] == want[k]).all(), (what, k, np.nonzero(got[k] != want[k])[0][:10])
    if counts:
        assert got["counts"].dtype == np.uint32 and got["counts"].shape == want["counts"].shape and (got["counts"] == want["counts"]).all(), (what, "counts")
    else:
        assert got["counts"] is None, what
    info = {k: v for k, v in got["info"].items() if k not in TIMES}
    assert info == want["info"], (what, info, want["info"])


def targets(c):
    return c["twords"], c["tbegin"], c["tlen"]


def device_args(c):
    import torch
    t = lambda a, view=None: None if a is None else torch.from_numpy(a.view(view) if view else a).cuda()
    return t(c["rows"], np.int32), t(c["lens"]), (t(c["twords"], np.int32), t(c["tbegin"]), t(c["tlen"])), t(c["pair_off"])


def polish_kw(v, counts):
    return dict(min_cover=v["min_cover"], min_percent=v["min_percent"], multi=v["multi"], counts=counts)


@pytest.mark.parametrize("name,i", QC.every())
def test_every_case_equals_the_checker(eng, name, i):
    c = QC.case(name)
    v, want = c["variants"][i], QC.checked(name, i)
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"], flags=QC.place_flags(v), **c["params"])
    assert (pl.to_host()["cover"] == want["cover"]).all()                       # the placement's depth mode agrees with the voters
    for counts in (False, True):
        pol = eng.polish(c["rows"], c["lens"], pl, **polish_kw(v, counts))
        assert_same(pol.to_host(), want, (name, i, "host arrays", counts), counts)
    rows, lens, tg, po = device_args(c)
    keep = [x.clone() for x in (rows, lens, *tg)]
    pl = eng.place_reads(rows, lens, targets=tg, pair_off=po, flags=QC.place_flags(v), **c["params"])
    before = pl.to_host()
    for counts in (True, False):
        pol = eng.polish(rows, lens, pl, **polish_kw(v, counts))
        assert_same(pol.to_host(), want, (name, i, "tensors", counts), counts)
        if counts:
            assert (pol.counts.sum(dim=1) == pl.cover).all()
    for a, b in zip([rows, lens, *tg], keep):
        assert (a == b).all()
    after = pl.to_host()
    assert all((before[k] == after[k]).all() for k in P.ARRAYS)                 # the placement is left as it was
    print(name, i, pol.info)


def test_the_callers_stream(eng):
    """tensors made on a stream of the caller's, both calls on that stream; then a polish on the engine's own stream"""
    import torch
    c, want = QC.case("planted"), QC.checked("planted")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rows, lens, tg, po = device_args(c)
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    pl = eng.place_reads(rows, lens, targets=tg, stream=s.cuda_stream, **c["params"])
    pol = eng.polish(rows, lens, pl, counts=True, stream=s.cuda_stream)
    assert s.query()                                                             # the call returns with its work on the stream done
    assert_same(pol.to_host(), want, "on the caller's stream", True)
    pol = eng.polish(rows, lens, pl)
    assert_same(pol.to_host(), want, "on the engine's stream afterwards")


def test_refusals_leave_an_earlier_result_valid(eng):
    c, want = QC.case("planted"), QC.checked("planted")
    other = QC.case("ties")
    stale = eng.place_reads(other["rows"], other["lens"], targets=targets(other), **other["params"])
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), **c["params"])
    pol = eng.polish(c["rows"], c["lens"], pl, counts=True)
    assert_same(pol.to_host(), want, "before", True)
    host = QC.placed("planted")
    v = int(np.nonzero((host["state"] & P.UNIQUE).astype(bool) & (host["target"] == 4))[0][-1])
    stride = c["rows"].shape[1]

    def lens_with(length):
        a = c["lens"].copy()
        a[2 * v] = a[2 * v + 1] = length
        return a
    calls = [dict(rows=other["rows"], lens=other["lens"], placements=stale),     # a stale placement: the engine holds another one
             dict(rows=c["rows"][:-2], lens=c["lens"][:-2]),                     # n / 2 != n_reads
             dict(rows=c["rows"][:-1], lens=c["lens"][:-1]),                     # n odd
             dict(lens=lens_with(16 * stride)),                                  # a voter that would leave its target (130 bases, pos 30, 112 bases)
             dict(lens=lens_with(16 * stride + 1)), dict(lens=lens_with(0)), dict(lens=lens_with(-1)),
             dict(min_cover=0), dict(min_percent=0), dict(min_percent=101)]
    for change in calls:
        a = dict(dict(rows=c["rows"], lens=c["lens"], placements=pl), **change)
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.polish(a["rows"], a["lens"], a["placements"], counts=True, **{k: a[k] for k in ("min_cover", "min_percent") if k in a})
        assert ei.value.code == -1, (list(change), ei.value)
        assert_same(pol.to_host(), want, ("after a refusal", list(change)), True)    # nothing written: the earlier result as it was
    again = eng.polish(c["rows"], c["lens"], pl)
    assert_same(again.to_host(), want, "the engine afterwards")
    # a later placement call does not invalidate the polish
    eng.place_reads(other["rows"], other["lens"], targets=targets(other), **other["params"])
    assert_same(again.to_host(), want, "after a later placement")


def test_second_round_on_planted(eng):
    """place -> polish on the first round's output, with no new call: nothing changes any more, and every planted column that changed has reads
    without a mismatch over it.  The second polish overwrites the buffer its own targets came from."""
    c, want = QC.case("planted"), QC.checked("planted")
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), **c["params"])
    pol = eng.polish(c["rows"], c["lens"], pl)
    first = pol.to_host()
    assert_same(first, want, "first round")
    pl2 = eng.place_reads(c["rows"], c["lens"], targets=pol.targets(), **c["params"])
    got2 = pl2.to_host()
    tw, tb, tl = Q.targets_of(want)
    want2 = P.place(c["rows"], c["lens"], None, tw, tb, tl, **c["params"])
    for k in P.ARRAYS:
        assert (got2[k] == want2[k]).all(), k
    pol2 = eng.polish(c["rows"], c["lens"], pl2, counts=True)
    h2 = pol2.to_host()
    assert_same(h2, Q.polish_scatter(c["rows"], c["lens"], want2, tw, tb, tl), "second round", True)
    assert pol2.n_changed == 0 and pol2.info["changed"] == 0 and (h2["words"] == first["words"]).all()
    off = first["col_off"].astype(np.int64)
    start = off[np.maximum(got2["target"], 0)] + got2["pos"]
    votes = (got2["state"] & P.UNIQUE).astype(bool)
    for g in first["changed_cols"].astype(np.int64):
        over = votes & (start <= g) & (g < start + c["lens"][1::2])
        assert over.sum() >= 3 and (got2["mm"][over] == 0).any() and h2["counts"][g].max() == h2["counts"][g].sum(), g


@pytest.fixture(scope="module")
def chain(eng):
    """6 kb with a 400-nt repeat, reads with 1 % substitutions: build -> cut -> contigs -> consensus -> final"""
    words, lens, genome = QC.chain_reads()
    e = eng.prefsuf_host(words, lens, GC.MIN_OVERLAP, GC.RSOEMO)
    cut = eng.cut_triangles_host(len(lens), e, GC.MOPP)
    u = eng.contigs(words, lens, cut, GC.MOPP)
    c = eng.unitig_consensus(words, lens, u, min_votes=0)
    fin = eng.final_contigs(u, c, 150, 95, 25)
    return words, lens, genome, u, c, fin


def records(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1
    return lines[0:-1:2], lines[1::2]


def codes(s):
    return np.array(["ACGT".index(x) for x in s], dtype=np.uint8)


def test_whole_chain_polished_final_contigs(eng, chain, tmp_path):
    words, lens, genome, u, c, fin = chain
    tw, tb, tl = QC.final_targets(u.to_host(), c.to_host(), fin.to_host())
    pl = eng.place_reads(words, lens, final=fin)
    want_pl = P.place(words, lens, None, tw, tb, tl)
    pol = eng.polish(words, lens, pl, counts=True)
    want = Q.polish_scatter(words, lens, want_pl, tw, tb, tl)
    got = pol.to_host()
    assert_same(got, want, "on the final contigs", True)
    print(pol.info)
    assert fin.n_accepted >= 3 and pol.n_changed > 0
    paths = {k: str(tmp_path / (k + ".fasta")) for k in ("plain", "depth", "polished", "polished_plain")}
    eng.write_final_fasta(paths["plain"], fin)
    eng.write_final_fasta(paths["depth"], fin, placements=pl)
    info = eng.write_final_fasta(paths["polished"], fin, placements=pl, polished=pol)
    eng.write_final_fasta(paths["polished_plain"], fin, placements=pl, polished=pol, depth=False)
    assert info["segments"] == fin.n_written and info["bytes"] == os.path.getsize(paths["polished"])
    (hp, sp), (hd, sd), (hq, sq), (hqp, sqp) = (records(paths[k]) for k in ("plain", "depth", "polished", "polished_plain"))
    # the same headers and lengths as the depth FASTA (the plain one without the depth), the sequences differ exactly at the changed columns
    assert hq == hd and hqp == hp and sqp == sq and sp == sd and [len(s) for s in sq] == [len(s) for s in sd]
    a, b = codes("".join(sd)), codes("".join(sq))
    assert len(a) == pol.n_columns and np.nonzero(a != b)[0].tolist() == got["changed_cols"].tolist()
    assert (b[got["changed_cols"]] == got["changed_bases"] >> 2).all() and (a[got["changed_cols"]] == got["changed_bases"] & 3).all()
    assert [codes(s).tolist() for s in sq] == [s.tolist() for s in Q.sequences(want) if len(s)]
    before, after = sum(QC.distance_to(genome, codes(s)) for s in sd), sum(QC.distance_to(genome, codes(s)) for s in sq)
    print("distance to the genome", before, "->", after)
    assert after <= before
    # a polish of a placement on caller's targets is none of the final result; nor is a stale one
    other = eng.place_reads(words, lens, targets=(tw, tb, tl))
    pol2 = eng.polish(words, lens, other)
    assert_same(pol2.to_host(), want, "the same windows as caller's targets")
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.write_final_fasta(paths["polished"], fin, placements=other, polished=pol2)
    assert ei.value.code == -1
    pl = eng.place_reads(words, lens, final=fin)
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.write_final_fasta(paths["polished"], fin, placements=pl, polished=pol2)      # the polish at hand is of `other`
    assert ei.value.code == -1
    pol = eng.polish(words, lens, pl)
    eng.write_final_fasta(paths["polished"], fin, placements=pl, polished=pol)
    assert records(paths["polished"]) == (hq, sq)


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, c in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in c)))


def test_command_line(tmp_path):
    """paired reads (1 % substitutions) of a 4 kb genome through alga_hip: --polish=1 --polish_changes= against the checker on the contigs the
    unpolished run writes; the headers carry the depth iff --contigs_depth=1.  (--consensus_min_votes=0: the exact overlaps of such reads give
    contigs of 150 .. 200 bases, which the default window would cut below --contigs_min_length)"""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    rng = np.random.default_rng(78)
    g = rng.integers(0, 4, size=4000, dtype=np.uint8)

    def noisy(r):
        r = r.copy()
        e = rng.random(len(r)) < 0.01
        r[e] = (r[e] + rng.integers(1, 4, size=int(e.sum()))) & 3
        return r
    m1, m2 = [], []
    for a in rng.permutation(np.arange(0, 4000 - 300, 2)):
        ins = int(rng.integers(250, 301))
        m1.append(noisy(g[a:a + 100]))
        m2.append(noisy(P.revcomp(g[a + ins - 100:a + ins])))
    _write_fasta(str(tmp_path / "a.fasta"), m1)
    _write_fasta(str(tmp_path / "b.fasta"), m2)
    out = {}
    for name, args in (("depth", ["--contigs_depth=1"]), ("polish", ["--polish=1", "--contigs_depth=1", "--polish_changes=c.tsv"]), ("polish_plain", ["--polish=1"])):
        wd = tmp_path / name
        wd.mkdir()
        r = subprocess.run([exe, "--file1=../a.fasta", "--file2=../b.fasta", "--output=o.fasta", "--contigs_final=f.fasta", "--contigs_min_length=150", "--consensus_min_votes=0", "--retl=0", "--retr=0"] + args,
                           cwd=str(wd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert ("Final contigs polished" in r.stderr) == name.startswith("polish") and "Reads placed on the final contigs" in r.stderr, r.stderr[-2000:]
        out[name] = {f: open(str(wd / f)).read() for f in ("f.fasta", "c.tsv") if (wd / f).exists()}
        out[name]["stderr"] = r.stderr
    for bad in (["--polish=1"], ["--contigs_final=f.fasta", "--polish_changes=c.tsv"]):
        r = subprocess.run([exe, "--file1=a.fasta", "--output=o.fasta"] + bad, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 2 and "needs" in r.stderr
    assert list(out["depth"]) == list(out["polish_plain"]) == ["f.fasta", "stderr"]
    deep, pol, plain = (out[k]["f.fasta"].split("\n") for k in ("depth", "polish", "polish_plain"))
    assert pol[0::2] == deep[0::2] and pol[1::2] == plain[1::2] and [h.split("_reads=")[0] for h in deep[0::2]] == plain[0::2] and len(deep) > 2
    ids = [int(h.split("=")[1].split("_")[0]) for h in deep[0::2] if h]
    tg = [np.zeros(0, np.uint8)] * (max(ids) + 1)
    for j, s in zip(ids, [codes(s) for s in deep[1::2] if s]):
        tg[j] = s
    rows, lens = P.nodes_of([x for pair in zip(m1, m2) for x in pair])
    tw, tb, tl = P.ragged(tg, [0] * len(tg))
    want = Q.polish_scatter(rows, lens, P.place(rows, lens, None, tw, tb, tl), tw, tb, tl)
    print(want["info"])
    assert want["info"]["changed"] > 0 and len(ids) >= 3
    assert [codes(s).tolist() for s in pol[1::2] if s] == [s.tolist() for s in Q.sequences(want) if len(s)]
    off = want["col_off"].astype(np.int64)
    lines = []
    for col, b in zip(want["changed_cols"].astype(np.int64), want["changed_bases"]):
        t = int(np.searchsorted(off, col, side="right")) - 1
        lines.append("%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d" % ((t, col - off[t], "ACGT"[b & 3], "ACGT"[b >> 2]) + tuple(want["counts"][col].tolist())))
    assert out["polish"]["c.tsv"] == "".join(x + "\n" for x in lines)
    said = "%d voters, %d voted columns of %d, %d changed, %d ambiguous" % tuple(want["info"][k] for k in ("voters", "voted_columns", "columns", "changed", "ambiguous"))
    assert said in out["polish"]["stderr"] and said in out["polish_plain"]["stderr"], out["polish"]["stderr"][-2000:]
