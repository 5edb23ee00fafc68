"""The break stage on the GPU (alga_break_placed_device, alga_write_broken_fasta_device): every output array and every counter equal to the
Python definition (tests/break_checker.py) on the cases of tests/break_cases.py, from host arrays and from tensors; the piece FASTA bytes and
the cuts; the planted chimera end to end with a polish in between and the round trip place -> break -> place on the pieces -> scaffold; the
caller's stream; refusals leave an earlier result valid; a result stays valid across a later placement, polish and scaffold; the command line."""
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import break_cases as QC
import break_checker as BC
import place_cases as PC
import place_checker as P
import polish_checker as Q
import scaffold_checker as SC

pytestmark = pytest.mark.gpu
TIMES = ("ms_span", "ms_cut", "ms_total")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what=""):
    for k in BC.ARRAYS:
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


@pytest.mark.parametrize("name", sorted(QC.CASES))
def test_every_case_equals_the_checker(eng, name, tmp_path):
    c = QC.case(name)
    path = str(tmp_path / "b.fasta")
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"], **c["params"])
    rows, lens, tg, po = device_args(c)
    for i, v in enumerate(c["variants"]):
        want = QC.checked(name, i)
        bk = eng.break_contigs(c["rows"], c["lens"], c["pair_off"], pl, **v)
        got = bk.to_host()
        assert_same(got, want, (name, i, "host arrays"))                         # `words` among them: the targets' columns
        assert bk.info["pairs_proper"] == pl.info["pairs_proper"]
        assert (bk.n_targets, bk.n_pieces, bk.n_cuts, bk.n_columns) == (len(c["tlen"]), len(want["len"]), len(want["cut_cols"]), int(c["tlen"].sum()))
        info = eng.write_broken_fasta(path, bk)
        text = open(path, "rb").read()
        assert text == BC.fasta(want), (name, i)
        assert info["segments"] == int((want["len"] > 0).sum()) and info["bytes"] == len(text)
        assert bk.cuts_tsv().encode() == BC.cuts_tsv(want), (name, i)
        print(name, i, bk.info)
    # from tensors: they are used where they are and left untouched
    keep = [x.clone() for x in (rows, lens, *tg)]
    pl = eng.place_reads(rows, lens, targets=tg, pair_off=po, **c["params"])
    before = pl.to_host()
    for i, v in enumerate(c["variants"]):
        bk = eng.break_contigs(rows, lens, po, pl, **v)
        assert_same(bk.to_host(), QC.checked(name, i), (name, i, "tensors"))
    for a, b in zip([rows, lens, *tg], keep):
        assert (a == b).all()
    after = pl.to_host()
    assert all((before[k] == after[k]).all() for k in P.ARRAYS)                 # the placement is left as it was


def test_margin_defaults_to_the_placements_median(eng):
    c = QC.case("one_cut")
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    median = pl.info["insert_median"]
    assert median == QC.placed("one_cut")["info"]["insert_median"] == 100
    want = BC.break_pairs(*QC.break_args(c, QC.placed("one_cut")), margin=median, inset=20)
    assert_same(eng.break_contigs(c["rows"], c["lens"], c["pair_off"], pl, inset=20).to_host(), want, "the median as margin")
    assert want["info"]["cuts"] == 1
    c = QC.case("no_pairs")                                                      # no proper pair: no median
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    assert pl.info["insert_median"] == -1
    with pytest.raises(alga_amd.AlgaError):
        eng.break_contigs(c["rows"], c["lens"], c["pair_off"], pl)


def damaged_chimera():
    """the planted chimera with 1 % substitutions in the reads and one wrong base in column 500 of the chimera, which the polish puts right"""
    c, g = QC.chimera(noisy=True)
    seqs = [s.copy() for s in c["seqs"]]
    seqs[1][500] = (seqs[1][500] + 1) & 3
    tw, tb, tl = P.ragged(seqs, [3 * i % 16 for i in range(len(seqs))])
    return dict(c, twords=tw, tbegin=tb, tlen=tl, seqs=seqs), g


def test_planted_chimera_end_to_end_with_a_polish_between(eng, tmp_path):
    """place -> polish -> break -> place on the pieces -> scaffold: the pieces carry the polished bases, the second placement equals the
    checker's on the pieces, the scaffold is the CPU test's layout, and the break result is still right after all of it"""
    c, g = damaged_chimera()
    v = c["variants"][0]
    path = str(tmp_path / "b.fasta")
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    want_pl = P.place(*PC.args(c))
    median = want_pl["info"]["insert_median"]
    assert pl.info["insert_median"] == median
    plain = eng.break_contigs(c["rows"], c["lens"], c["pair_off"], pl, **v).to_host()
    assert_same(plain, BC.break_pairs(*QC.break_args(c, want_pl), margin=median, **v), "without the polish: the targets' columns")
    pol = eng.polish(c["rows"], c["lens"], pl)
    want_pol = Q.polish_scatter(c["rows"], c["lens"], want_pl, *targets(c))
    polished = Q.sequences(want_pol)
    assert (polished[1][500] + 1) & 3 == c["seqs"][1][500] and want_pol["info"]["changed"] >= 1   # a column inside piece 1 changed
    bk = eng.break_contigs(c["rows"], c["lens"], c["pair_off"], pl, polished=pol, **v)
    want = BC.break_pairs(*QC.break_args(c, want_pl, polished), margin=median, **v)
    got = bk.to_host()
    assert_same(got, want, "with the polish: the polished columns")
    assert (got["words"] != plain["words"]).any() and (got["words"] == pol.to_host()["words"]).all()
    print(pl.info, bk.info, BC.cuts_tsv(want))
    assert bk.info["cuts"] == 1 and got["t_cuts"].tolist() == [0, 1] and abs(int(got["piece_start"][2]) - QC.CHIMERA_JUNCTION) <= v["inset"]
    eng.write_broken_fasta(path, bk)
    assert open(path, "rb").read() == BC.fasta(want)
    # the round trip: the pieces as the targets of the next placement
    c2 = QC.pieces_case(c, want)
    want_pl2 = P.place(*PC.args(c2))
    pl2 = eng.place_reads(c["rows"], c["lens"], targets=bk.targets(), pair_off=c["pair_off"])
    got_pl2 = pl2.to_host()
    for k in P.ARRAYS:
        assert (got_pl2[k] == want_pl2[k]).all(), k
    assert {k: got_pl2["info"][k] for k in P.COUNTERS} == want_pl2["info"]
    eng.polish(c["rows"], c["lens"], pl2)
    sc = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl2)
    want_sc = SC.scaffold_dicts(c2["rows"], c2["lens"], c2["pair_off"], want_pl2, insert=want_pl2["info"]["insert_median"])
    got_sc = sc.to_host()
    for k in SC.ARRAYS:
        assert (got_sc[k] == want_sc[k]).all(), k
    assert [(int(m), int(got_sc["orient"][m])) for m in got_sc["s_members"]] == [(1, 0), (0, 1), (2, 0)] and sc.info["joins"] == 2 and sc.info["scaffolds"] == 1
    eng.write_scaffold_fasta(str(tmp_path / "s.fasta"), pl2, sc)
    assert open(str(tmp_path / "s.fasta"), "rb").read() == SC.fasta(want_sc, c2["seqs"])
    # the break result and its FASTA after that placement, polish and scaffold
    assert_same(bk.to_host(), want, "after a placement, a polish and a scaffold call")
    eng.write_broken_fasta(path, bk)
    assert open(path, "rb").read() == BC.fasta(want)
    # a second round cuts nothing
    again = eng.break_contigs(c["rows"], c["lens"], c["pair_off"], pl2, **v)
    assert again.info["cuts"] == 0 and again.n_pieces == 3
    assert_same(again.to_host(), BC.break_pairs(c2["rows"], c2["lens"], c2["pair_off"], want_pl2, c2["seqs"], margin=want_pl2["info"]["insert_median"], **v), "second round")


def test_the_callers_stream(eng):
    import torch
    c, want = QC.case("many_cuts"), QC.checked("many_cuts")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rows, lens, tg, po = device_args(c)
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    pl = eng.place_reads(rows, lens, targets=tg, pair_off=po, stream=s.cuda_stream, **c["params"])
    bk = eng.break_contigs(rows, lens, po, pl, stream=s.cuda_stream, **c["variants"][0])
    assert s.query()                                                             # the call returns with its work on the stream done
    assert_same(bk.to_host(), want, "on the caller's stream")
    bk = eng.break_contigs(rows, lens, po, pl, **c["variants"][0])
    assert_same(bk.to_host(), want, "on the engine's stream afterwards")


def test_refusals_leave_an_earlier_result_valid(eng, tmp_path):
    c, want = QC.case("open"), QC.checked("open")
    other = QC.case("inset")
    stale = eng.place_reads(other["rows"], other["lens"], targets=targets(other), pair_off=other["pair_off"])
    stale_polish = eng.polish(other["rows"], other["lens"], stale)
    # the same reads placed earlier on as many targets with fewer columns, and on the same targets with another max_insert: these structs name
    # the buffers, n_reads and n_targets of the current placement, but not its n_columns / n_hist
    short = [s.copy() for s in c["seqs"]]
    short[0] = short[0][:-5]                                                     # (no read lies on target 0)
    stale_cols = eng.place_reads(c["rows"], c["lens"], targets=P.ragged(short, [0] * len(short)), pair_off=c["pair_off"])
    stale_hist = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"], max_insert=500)
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    v0 = c["variants"][0]
    bk = eng.break_contigs(c["rows"], c["lens"], c["pair_off"], pl, **v0)
    assert_same(bk.to_host(), want, "before")
    host = QC.placed("open")
    v = int(np.nonzero((host["target"] == 6) & (host["pos"] == 38))[0][0])       # a read of 25 bases that ends where its target of 63 ends

    def lens_with(length):
        a = c["lens"].copy()
        a[2 * v] = a[2 * v + 1] = length
        return a
    bad_pair = c["pair_off"].copy()
    bad_pair[2] = bad_pair[3] = 0                                                # the mate of read 0 does not point back
    big = c["pair_off"].copy()
    big[0] = big[1] = 3
    calls = [dict(rows=other["rows"], lens=other["lens"], pair_off=other["pair_off"], placements=stale),   # a stale placement
             dict(placements=stale_cols), dict(placements=stale_hist),                                     # stale, of the same reads and target count
             dict(polished=stale_polish),                                                                  # the polish of another placement
             dict(rows=c["rows"][:-2], lens=c["lens"][:-2], pair_off=c["pair_off"][:-2]),                  # n / 2 != n_reads
             dict(rows=c["rows"][:-1], lens=c["lens"][:-1], pair_off=c["pair_off"][:-1]),                  # n odd
             dict(pair_off=bad_pair), dict(pair_off=big),
             dict(lens=lens_with(26)),                                                                     # past the end of its target
             dict(lens=lens_with(33)), dict(lens=lens_with(0)), dict(lens=lens_with(-1)),
             dict(min_span=0), dict(min_span=2 ** 31), dict(inset=-1), dict(inset=2 ** 20 + 1), dict(margin=-1), dict(margin=2 ** 20 + 1)]
    for change in calls:
        a = dict(dict(rows=c["rows"], lens=c["lens"], pair_off=c["pair_off"], placements=pl, polished=None, **v0), **change)
        with pytest.raises((alga_amd.AlgaError, OverflowError)) as ei:
            eng.break_contigs(a["rows"], a["lens"], a["pair_off"], a["placements"], polished=a["polished"], **{k: a[k] for k in v0})
        assert isinstance(ei.value, OverflowError) and "min_span" in change or ei.value.code == -1, (list(change), ei.value)
        assert_same(bk.to_host(), want, ("after a refusal", list(change)))       # nothing written: the earlier result as it was
    # the target and position branches of the device check, reached by writing through the zero-copy views of the placement: the refusal is
    # the check that keeps the pair kernel's writes inside the difference array
    assert stale_cols.n_columns == pl.n_columns - 5 and stale_hist.n_hist == 501 and pl.n_hist == 1001
    assert (stale_cols.n_reads, stale_cols.n_targets, stale_cols._c.d_target, stale_cols._c.d_col_off) == (pl.n_reads, pl.n_targets, pl._c.d_target, pl._c.d_col_off)
    T = len(c["tlen"])
    total = int(pl.col_off[T])
    # ... and the column count the device compares with col_off[n_targets]: refused before any column array is sized or written from it
    for view, at, value in ((pl.target, v, T), (pl.target, v, -1), (pl.pos, v, -1), (pl.pos, v, 39), (pl.col_off, T, total + 1), (pl.col_off, T, total - 1)):
        keep = int(view[at])
        view[at] = value
        try:
            with pytest.raises(alga_amd.AlgaError) as ei:
                eng.break_contigs(c["rows"], c["lens"], c["pair_off"], pl, **v0)
            assert ei.value.code == -1, (value, ei.value)
        finally:
            view[at] = keep
        assert_same(bk.to_host(), want, ("after a refusal on the device", value))
    path = str(tmp_path / "b.fasta")
    eng.write_broken_fasta(path, bk)
    assert open(path, "rb").read() == BC.fasta(want)
    again = eng.break_contigs(c["rows"], c["lens"], c["pair_off"], pl, **v0)
    assert_same(again.to_host(), want, "the engine afterwards")


def test_a_result_stays_valid_across_a_later_placement_polish_and_scaffold(eng, tmp_path):
    c, want = QC.case("seams"), QC.checked("seams")
    other = QC.case("inset")
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
    bk = eng.break_contigs(c["rows"], c["lens"], c["pair_off"], pl, **c["variants"][0])
    pl2 = eng.place_reads(other["rows"], other["lens"], targets=targets(other), pair_off=other["pair_off"])
    eng.polish(other["rows"], other["lens"], pl2)
    eng.scaffold(other["rows"], other["lens"], other["pair_off"], pl2)
    assert_same(bk.to_host(), want, "after a later placement, polish and scaffold")
    assert bk.cuts_tsv().encode() == BC.cuts_tsv(want)
    path = str(tmp_path / "b.fasta")
    eng.write_broken_fasta(path, bk)                                             # the pieces' bases are the result's own copy
    assert open(path, "rb").read() == BC.fasta(want)
    # the pieces (targets that begin at every residue mod 16, empty ones among them) as the targets of a placement
    c2 = QC.pieces_case(c, want)
    got = eng.place_reads(c["rows"], c["lens"], targets=bk.targets(), pair_off=c["pair_off"]).to_host()
    want_pl = P.place(*PC.args(c2))
    for k in P.ARRAYS:
        assert (got[k] == want_pl[k]).all(), k


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, c in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in c)))


def codes(s):
    return np.array(["ACGT".index(x) for x in s], dtype=np.uint8)


def test_command_line(eng, tmp_path):
    """paired reads of a 6 kb genome through alga_hip; every pair whose fragment would span the columns around 3000 has its second mate drawn
    1200 bases away instead (no proper pair: the insert is above 1000), so the reads join the contig there and no pair supports the join:
    --break_misjoins=1 --broken= --break_cuts= --scaffolds= against the Python API and the checker on the contigs the run writes"""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    rng = np.random.default_rng(92)
    g = rng.integers(0, 4, size=6000, dtype=np.uint8)
    m1, m2 = [], []
    for a in rng.permutation(np.arange(0, 6000 - 400, 2)):
        a = int(a)
        ins = int(rng.integers(300, 401))
        if a + 21 < 3020 and a + ins - 21 > 2980:
            ins = 1200
            if a + ins > 6000:
                continue
        m1.append(g[a:a + 100])
        m2.append(P.revcomp(g[a + ins - 100:a + ins]))
    _write_fasta(str(tmp_path / "a.fasta"), m1)
    _write_fasta(str(tmp_path / "b.fasta"), m2)
    base = [exe, "--file1=a.fasta", "--file2=b.fasta", "--output=o.fasta", "--contigs_final=f.fasta", "--contigs_min_length=150", "--consensus_min_votes=0", "--retl=0", "--retr=0"]
    run = lambda args: subprocess.run(args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    r0 = run(base + ["--scaffolds=s0.fasta", "--scaffold_layout=l0.tsv"])
    assert r0.returncode == 0, r0.stderr[-2000:]
    kept = {n: open(str(tmp_path / n), "rb").read() for n in ("f.fasta", "s0.fasta", "l0.tsv")}   # (--output= is the name stock ALGA would write: not run here)
    r = run(base + ["--scaffolds=s.fasta", "--scaffold_layout=l.tsv", "--break_misjoins=1", "--broken=p.fasta", "--break_cuts=c.tsv"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Contigs broken:" in r.stderr and "Reads placed on the pieces" in r.stderr and "Contigs broken:" not in r0.stderr, r.stderr[-2000:]
    assert open(str(tmp_path / "f.fasta"), "rb").read() == kept["f.fasta"]       # what the run wrote without the switch, it writes with it
    r1 = run(base + ["--scaffolds=s1.fasta", "--scaffold_layout=l1.tsv", "--break_misjoins=0"])
    assert r1.returncode == 0 and "Contigs broken:" not in r1.stderr, r1.stderr[-2000:]
    assert open(str(tmp_path / "s1.fasta"), "rb").read() == kept["s0.fasta"] and open(str(tmp_path / "l1.tsv"), "rb").read() == kept["l0.tsv"]
    for bad in (["--file1=a.fasta", "--file2=b.fasta", "--output=o2.fasta", "--break_misjoins=1"],
                ["--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--break_misjoins=1"],
                ["--file1=a.fasta", "--file2=b.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--broken=p2.fasta"],
                ["--file1=a.fasta", "--file2=b.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--break_cuts=c2.tsv"]):
        rb = run([exe] + bad)
        assert rb.returncode == 2 and "need" in rb.stderr
    contigs = kept["f.fasta"].decode().split("\n")
    ids = [int(h.split("=")[1].split("_")[0]) for h in contigs[0::2] if h]
    tg = [np.zeros(0, np.uint8)] * (max(ids) + 1)
    for j, s in zip(ids, [codes(s) for s in contigs[1::2] if s]):
        tg[j] = s
    rows, lens = P.nodes_of([x for pair in zip(m1, m2) for x in pair])
    pair_off = np.array([1, 1, 2, 2] * len(m1), dtype=np.uint8)
    tw, tb, tl = P.ragged(tg, [0] * len(tg))
    # the Python API on the same contigs
    pl = eng.place_reads(rows, lens, targets=(tw, tb, tl), pair_off=pair_off)
    bk = eng.break_contigs(rows, lens, pair_off, pl)
    got = bk.to_host()
    print(bk.info, r.stderr[-900:])
    assert bk.info["cuts"] >= 1 and max(tl) > 3100
    eng.write_broken_fasta(str(tmp_path / "api.fasta"), bk)
    assert open(str(tmp_path / "p.fasta"), "rb").read() == open(str(tmp_path / "api.fasta"), "rb").read()
    assert open(str(tmp_path / "c.tsv"), "rb").read() == bk.cuts_tsv(got).encode()
    i = bk.info
    said = "Contigs broken: %d proper pairs (%d spanning), %d weak columns, %d runs (%d open), %d cuts, %d contigs cut, %d pieces, N50 %d -> %d" % (
        i["pairs_proper"], i["pairs_spanning"], i["weak_columns"], i["runs"], i["runs_open"], i["cuts"], i["targets_cut"], i["pieces"], i["n50_targets"], i["n50_pieces"])
    assert said in r.stderr, r.stderr[-2000:]
    pl2 = eng.place_reads(rows, lens, targets=bk.targets(), pair_off=pair_off)
    sc = eng.scaffold(rows, lens, pair_off, pl2)
    eng.write_scaffold_fasta(str(tmp_path / "api_s.fasta"), pl2, sc)
    assert open(str(tmp_path / "s.fasta"), "rb").read() == open(str(tmp_path / "api_s.fasta"), "rb").read()
    assert open(str(tmp_path / "l.tsv"), "rb").read() == sc.layout_tsv().encode()
    # ... and the checker
    want_pl = P.place(rows, lens, pair_off, tw, tb, tl)
    want = BC.break_pairs(rows, lens, pair_off, want_pl, tg, margin=want_pl["info"]["insert_median"], **BC.DEFAULT)
    assert_same(got, want, "the command line's contigs")
    assert open(str(tmp_path / "p.fasta"), "rb").read() == BC.fasta(want) and open(str(tmp_path / "c.tsv"), "rb").read() == BC.cuts_tsv(want)
