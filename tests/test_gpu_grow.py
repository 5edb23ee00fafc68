"""The grow stage on the GPU (alga_grow_placed_device, alga_write_grown_fasta_device): every output array and every counter equal to the
Python definition (tests/grow_checker.py) on the cases of tests/grow_cases.py, from host arrays and from tensors, with and without a polish
between and with directories of 1, 4 and auto bits; the FASTA bytes and the TSV; the word seams of k_gr_ends and k_gr_build; a wave of k_gr_place that takes a second candidate; the
planted genome end to end with a scaffold call on the last placement; the caller's stream; refusals leave an earlier result valid; a result
stays valid across a later placement, polish, break and scaffold; the command line."""
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import grow_cases as QC
import grow_checker as GC
import place_checker as P
import polish_checker as Q

pytestmark = pytest.mark.gpu
TIMES = ("ms_index", "ms_place", "ms_build", "ms_total")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what=""):
    for k in GC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert (got[k] == want[k]).all(), (what, k, np.nonzero(got[k] != want[k])[0][:10])
    info = {k: v for k, v in got["info"].items() if k not in TIMES}
    assert info == want["info"], (what, info, want["info"])


def targets(c):
    return c["twords"], c["tbegin"], c["tlen"]


def device_args(c):
    import torch
    t = lambda a, view=None: None if a is None else torch.from_numpy(a.view(view) if view else a).cuda()
    return t(c["rows"], np.int32), t(c["lens"]), (t(c["twords"], np.int32), t(c["tbegin"]), t(c["tlen"]))


@pytest.mark.parametrize("name", sorted(QC.CASES))
def test_every_case_equals_the_checker(eng, name, tmp_path):
    c = QC.case(name)
    path = str(tmp_path / "g.fasta")
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), **c["params"])
    assert (pl.to_host()["state"] == QC.placed(name)["state"]).all()
    for i, v in enumerate(c["variants"]):
        want = QC.checked(name, i)
        for bits in (1, 4, 0):
            eng.set_option("place_dir_bits", bits)
            gw = eng.grow_ends(c["rows"], c["lens"], pl, **v)
            assert_same(gw.to_host(), want, (name, i, "host arrays", bits))
        got = gw.to_host()
        assert (gw.n_reads, gw.n_targets, gw.n_columns, gw.max_grow) == (len(c["lens"]) // 2, len(c["tlen"]), int(want["col_off"][-1]), dict(GC.DEFAULT, **v)["max_grow"])
        info = eng.write_grown_fasta(path, gw)
        text = open(path, "rb").read()
        assert text == GC.fasta(want), (name, i)
        assert info["segments"] == int((want["len"] > 0).sum()) and info["bytes"] == len(text)
        assert gw.grow_tsv(got).encode() == GC.grow_tsv(want), (name, i)
        print(name, i, gw.info)
    # with a polish between: the bases are the polished ones
    pol = eng.polish(c["rows"], c["lens"], pl)
    polished = Q.sequences(Q.polish_scatter(c["rows"], c["lens"], QC.placed(name), *targets(c)))
    for i, v in enumerate(c["variants"]):
        gw = eng.grow_ends(c["rows"], c["lens"], pl, polished=pol, **v)
        assert_same(gw.to_host(), GC.grow_index(c["rows"], c["lens"], QC.placed(name), polished, **v), (name, i, "polished"))
    # from tensors: they are used where they are and left untouched
    rows, lens, tg = device_args(c)
    keep = [x.clone() for x in (rows, lens, *tg)]
    pl = eng.place_reads(rows, lens, targets=tg, **c["params"])
    before = pl.to_host()
    for i, v in enumerate(c["variants"]):
        assert_same(eng.grow_ends(rows, lens, pl, **v).to_host(), QC.checked(name, i), (name, i, "tensors"))
    for a, b in zip([rows, lens, *tg], keep):
        assert (a == b).all()
    after = pl.to_host()
    assert all((before[k] == after[k]).all() for k in P.ARRAYS)                 # the placement is left as it was


def test_word_seams_of_the_end_columns_and_of_the_grown_targets(eng):
    """k_gr_ends and k_gr_build on tests/grow_cases.py: word_seams, at 8192 blocks and at one: ends of 1, 15, 16, 17, 31, 32 and 33 columns (those of
    15 and more anchor a read that grows them: a wrong end column loses it) and two of width 0; new lengths of the same values and a 0; totals
    that are no multiple of 16 (the last word partial, the two of padding zero) and, with grow_max_blocks 1, several words per lane in both"""
    c, want = QC.case("word_seams"), QC.checked("word_seams")
    assert want["len"].tolist() == QC.SEAM_NEW_LENS and want["left"][:4].tolist() == [0, 8, 8, 8] and want["right"][8:12].tolist() == [20, 20, 20, 64]
    assert int(want["col_off"][-1]) % 16 and int(want["col_off"][-1]) > 16 * 256
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), **c["params"])
    try:
        for blocks in (8192, 1):
            eng.set_option("grow_max_blocks", blocks)
            gw = eng.grow_ends(c["rows"], c["lens"], pl, **c["variants"][0])
            assert_same(gw.to_host(), want, ("word_seams", blocks))
    finally:
        eng.set_option("grow_max_blocks", 8192)


def test_polished_bases_are_grown(eng):
    """a wrong base in the anchored part of an end, put right by the polish: the unpolished end sees one mismatch more in every voter"""
    c = QC.case("cover")
    g = c["g"]
    seqs = [c["seqs"][0].copy()]
    seqs[0][250] = (seqs[0][250] + 1) & 3                                        # column 250 of g[100:400]: inside every voter's anchored part
    inner = [g[p:p + 100] for p in range(120, 301, 20)]                          # placed reads that cover the column
    rows, lens = P.nodes_of([P.codes_of(c["rows"][2 * r + 1], 0, 100) for r in range(3)] + inner)
    tw, tb, tl = P.ragged(seqs, [5])
    pl = eng.place_reads(rows, lens, targets=(tw, tb, tl))
    want_pl = P.place(rows, lens, None, tw, tb, tl)
    plain = eng.grow_ends(rows, lens, pl).to_host()
    assert_same(plain, GC.grow_index(rows, lens, want_pl, seqs), "unpolished")
    assert plain["mm"][:3].tolist() == [1, 1, 1]
    pol = eng.polish(rows, lens, pl)
    polished = Q.sequences(Q.polish_scatter(rows, lens, want_pl, tw, tb, tl))
    assert (polished[0] == c["seqs"][0]).all()
    got = eng.grow_ends(rows, lens, pl, polished=pol).to_host()
    assert_same(got, GC.grow_index(rows, lens, want_pl, polished), "polished")
    assert got["mm"][:3].tolist() == [0, 0, 0] and (GC.sequences(got)[0] == g[100:410]).all()


def test_a_wave_takes_a_second_candidate(eng):
    import torch
    waves = 8 * 4 * torch.cuda.get_device_properties(0).multi_processor_count  # k_gr_place: 8 blocks of 4 waves per CU
    c = QC.many_reads(waves + waves // 4 + 1000)                             # seven reads in eight are candidates
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c))
    host = pl.to_host()                                                          # (the placement has its own tests: its state is the checker's input here)
    want = GC.grow_index(c["rows"], c["lens"], host, c["seqs"])
    gw = eng.grow_ends(c["rows"], c["lens"], pl)
    assert_same(gw.to_host(), want, "many reads")
    print(gw.info)
    assert gw.info["candidates"] > waves and gw.info["voting"] > 1000 and gw.info["ends_grown"] >= 6 and (want["over"][:8] == np.arange(10, 18)).all()


def test_planted_genome_end_to_end(eng, tmp_path):
    """place -> grow -> place on Grown.targets() -> grow on the device, equal to the checker's loop in every round; every grown base is the
    genome's, round 1 adds at least 10 bases at each end, the inner ends overlap; a scaffold call on the last placement still works"""
    c, g, meta = QC.planted()
    lo, hi = [s for s, _ in QC.PLANTED_BOUNDS], [e for _, e in QC.PLANTED_BOUNDS]
    tg = targets(c)
    pair_off = np.array([1, 1, 2, 2] * (len(c["lens"]) // 4), dtype=np.uint8)
    for rnd in range(1, 5):
        pl = eng.place_reads(c["rows"], c["lens"], targets=tg, pair_off=pair_off)
        want_pl = P.place(c["rows"], c["lens"], pair_off, c["twords"], c["tbegin"], c["tlen"])
        assert (pl.to_host()["state"] == want_pl["state"]).all()
        gw = eng.grow_ends(c["rows"], c["lens"], pl)
        want = GC.grow_index(c["rows"], c["lens"], want_pl, c["seqs"])
        got = gw.to_host()
        assert_same(got, want, ("planted", rnd))
        if rnd == 1:
            assert min(got["left"].tolist() + got["right"].tolist()) >= 10
        for r, (a, clean) in enumerate(meta):
            if clean and any(lo[t] <= a and a + 100 <= hi[t] for t in range(2)):
                assert got["end"][r] == -1 and want_pl["state"][r] & P.PLACED
        lo = [lo[t] - int(got["left"][t]) for t in range(2)]
        hi = [hi[t] + int(got["right"][t]) for t in range(2)]
        for t, s in enumerate(GC.sequences(got)):
            assert (s == g[lo[t]:hi[t]]).all(), (rnd, t)
        print(rnd, gw.info)
        c = QC.next_round(c, want)
        tg = gw.targets()                                                        # the engine's tensors: the next placement reads them where they are
        if hi[0] > lo[1]:
            break
    assert hi[0] > lo[1] and rnd <= 4
    pl = eng.place_reads(c["rows"], c["lens"], targets=tg, pair_off=pair_off)
    sc = eng.scaffold(c["rows"], c["lens"], pair_off, pl, insert=300)
    assert sc.n_targets == 2 and sc.info["scaffolds"] >= 1
    eng.write_grown_fasta(str(tmp_path / "g.fasta"), gw)
    assert open(str(tmp_path / "g.fasta"), "rb").read() == GC.fasta(want)


def test_the_callers_stream(eng):
    import torch
    c, want = QC.case("tiny_targets"), QC.checked("tiny_targets")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rows, lens, tg = device_args(c)
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    pl = eng.place_reads(rows, lens, targets=tg, stream=s.cuda_stream)
    gw = eng.grow_ends(rows, lens, pl, stream=s.cuda_stream, **c["variants"][0])
    assert s.query()                                                             # the call returns with its work on the stream done
    assert_same(gw.to_host(), want, "on the caller's stream")
    gw = eng.grow_ends(rows, lens, pl, **c["variants"][0])
    assert_same(gw.to_host(), want, "on the engine's stream afterwards")


def test_refusals_leave_an_earlier_result_valid(eng, tmp_path):
    c, want = QC.case("mm_bound"), QC.checked("mm_bound")
    other = QC.case("cover")
    stale = eng.place_reads(other["rows"], other["lens"], targets=targets(other))
    stale_polish = eng.polish(other["rows"], other["lens"], stale)
    # the same reads placed earlier on as many targets with fewer columns: the struct names the buffers, n_reads and n_targets of the current
    # placement, but not its n_columns
    short = [s.copy() for s in c["seqs"]]
    short[0] = short[0][:-5]
    stale_cols = eng.place_reads(c["rows"], c["lens"], targets=P.ragged(short, [0] * len(short)))
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c))
    v0 = c["variants"][0]
    gw = eng.grow_ends(c["rows"], c["lens"], pl, **v0)
    assert_same(gw.to_host(), want, "before")
    odd = c["lens"].copy()
    odd[0] = 99                                                                  # twin lengths differ
    flipped = c["rows"].copy()
    flipped[0, 0] ^= 1                                                           # row 0 is not the reverse complement of row 1
    long_ = c["lens"].copy()
    long_[0] = long_[1] = 16 * c["rows"].shape[1] + 1                            # past the stride: refused before any row is read that far
    calls = [dict(rows=other["rows"], lens=other["lens"], placements=stale), dict(placements=stale_cols), dict(polished=stale_polish),
             dict(rows=c["rows"][:-2], lens=c["lens"][:-2]), dict(rows=c["rows"][:-1], lens=c["lens"][:-1]), dict(lens=odd), dict(rows=flipped), dict(lens=long_),
             dict(k=7), dict(k=32), dict(max_mismatches=-1), dict(max_mismatches=255), dict(max_occ=0), dict(max_occ=65536), dict(min_anchor=20),
             dict(min_anchor=2 ** 20 + 1), dict(min_cover=0), dict(min_percent=50), dict(min_percent=101), dict(max_grow=0), dict(max_grow=4097), dict(flags=1)]
    for change in calls:
        a = dict(dict(rows=c["rows"], lens=c["lens"], placements=pl, polished=None, **v0), **change)
        params = {k: a[k] for k in a if k not in ("rows", "lens", "placements", "polished")}
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.grow_ends(a["rows"], a["lens"], a["placements"], polished=a["polished"], **params)
        assert ei.value.code == -1, (list(change), ei.value)
        assert_same(gw.to_host(), want, ("after a refusal", list(change)))       # nothing written: the earlier result as it was
    with pytest.raises(TypeError):
        eng.grow_ends(c["rows"], c["lens"], pl, min_span=1)
    # the column count the device compares with col_off[n_targets], reached by writing through the zero-copy view of the placement: refused
    # before any column array is sized or read from it
    assert (stale_cols.n_reads, stale_cols.n_targets, stale_cols._c.d_col_off) == (pl.n_reads, pl.n_targets, pl._c.d_col_off) and stale_cols.n_columns == pl.n_columns - 5
    T = len(c["tlen"])
    total = int(pl.col_off[T])
    for value in (total + 1, total - 1):
        pl.col_off[T] = value
        try:
            with pytest.raises(alga_amd.AlgaError) as ei:
                eng.grow_ends(c["rows"], c["lens"], pl, **v0)
            assert ei.value.code == -1, (value, ei.value)
        finally:
            pl.col_off[T] = total
        assert_same(gw.to_host(), want, ("after a refusal on the device", value))
    path = str(tmp_path / "g.fasta")
    eng.write_grown_fasta(path, gw)
    assert open(path, "rb").read() == GC.fasta(want)
    again = eng.grow_ends(c["rows"], c["lens"], pl, **v0)
    assert_same(again.to_host(), want, "the engine afterwards")
    with pytest.raises(alga_amd.AlgaError):
        eng.write_grown_fasta(path, gw)                                          # `gw` is the result before the last one
    eng.write_grown_fasta(path, again)
    assert open(path, "rb").read() == GC.fasta(want)


def test_a_result_stays_valid_across_a_later_placement_polish_break_and_scaffold(eng, tmp_path):
    import break_cases as BQ
    c, want = QC.case("tiny_targets"), QC.checked("tiny_targets")
    other = BQ.case("inset")
    pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c))
    gw = eng.grow_ends(c["rows"], c["lens"], pl, **c["variants"][0])
    pl2 = eng.place_reads(other["rows"], other["lens"], targets=targets(other), pair_off=other["pair_off"])
    eng.polish(other["rows"], other["lens"], pl2)
    eng.break_contigs(other["rows"], other["lens"], other["pair_off"], pl2, **other["variants"][0])
    eng.scaffold(other["rows"], other["lens"], other["pair_off"], pl2)
    assert_same(gw.to_host(), want, "after a later placement, polish, break and scaffold")
    path = str(tmp_path / "g.fasta")
    eng.write_grown_fasta(path, gw)                                              # the bases are the result's own copy
    assert open(path, "rb").read() == GC.fasta(want)
    # the grown targets (an empty one among them, every residue mod 16) as the targets of a placement
    c2 = QC.next_round(c, want)
    got = eng.place_reads(c["rows"], c["lens"], targets=gw.targets()).to_host()
    want_pl = P.place(*QC.place_args(c2))
    for k in P.ARRAYS:
        assert (got[k] == want_pl[k]).all(), k
    assert want_pl["info"]["placed"] == 3                                        # the reads that hung over an end lie inside now


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, c in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in c)))


def codes(s):
    return np.array(["ACGT".index(x) for x in s], dtype=np.uint8)


def test_command_line(eng, tmp_path):
    """paired reads of a 6 kb genome with a hole of 400 bases through alga_hip with --grow_ends=2 --grown= --grow_layout=: the files against the Python API doing the same
    rounds on the contigs the run writes, and against the checker; a run at --grow_ends=0 writes what a run without the option writes"""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    rng = np.random.default_rng(93)
    g = rng.integers(0, 4, size=6000, dtype=np.uint8)
    m1, m2 = [], []
    for a in rng.permutation(np.arange(0, 6000 - 400, 2)):
        a, ins = int(a), int(rng.integers(300, 401))
        if a + ins <= 2800 or a >= 3200:                                         # no fragment touches 2800 .. 3200
            m1.append(g[a:a + 100])
            m2.append(P.revcomp(g[a + ins - 100:a + ins]))
    for a in range(45, 55):                                                      # reads that lie on the last / first a bases next to the hole: an overlap below
        m1.append(g[2800 - a:2900 - a])                                          # the graph's minimum of 55, so no contig runs through them, and mates on two contigs
        m2.append(P.revcomp(g[3100 + a:3200 + a]))
    _write_fasta(str(tmp_path / "a.fasta"), m1)
    _write_fasta(str(tmp_path / "b.fasta"), m2)
    base = [exe, "--file1=a.fasta", "--file2=b.fasta", "--output=o.fasta", "--contigs_min_length=150", "--consensus_min_votes=0", "--retl=0", "--retr=0"]
    run = lambda args: subprocess.run(args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    r0 = run(base + ["--contigs_final=f0.fasta", "--scaffolds=s0.fasta", "--scaffold_layout=l0.tsv", "--placements=p0.tsv"])
    assert r0.returncode == 0, r0.stderr[-2000:]
    r1 = run(base + ["--contigs_final=f1.fasta", "--scaffolds=s1.fasta", "--scaffold_layout=l1.tsv", "--placements=p1.tsv", "--grow_ends=0"])
    assert r1.returncode == 0 and "Contig ends grown" not in r0.stderr + r1.stderr, r1.stderr[-2000:]
    for a, b in (("f0.fasta", "f1.fasta"), ("s0.fasta", "s1.fasta"), ("l0.tsv", "l1.tsv"), ("p0.tsv", "p1.tsv")):
        assert open(str(tmp_path / a), "rb").read() == open(str(tmp_path / b), "rb").read(), a
    r = run(base + ["--contigs_final=f.fasta", "--scaffolds=s.fasta", "--scaffold_layout=l.tsv", "--grow_ends=2", "--grown=g.fasta", "--grow_layout=g.tsv", "--grow_min_anchor=25",
                   "--grow_min_cover=2"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Contig ends grown, round 1:" in r.stderr and "Reads placed on the grown contigs" in r.stderr, r.stderr[-2000:]
    assert open(str(tmp_path / "f.fasta"), "rb").read() == open(str(tmp_path / "f0.fasta"), "rb").read()   # the final contigs are what they were
    for bad in (["--file1=a.fasta", "--output=o2.fasta", "--grow_ends=1"], ["--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--grown=g2.fasta"],
                ["--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--grow_layout=g2.tsv"],
                ["--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--grow_ends=17"],
                ["--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--grow_ends=1", "--grow_min_percent=50"]):
        rb = run([exe] + bad)
        assert rb.returncode == 2 and ("need" in rb.stderr or "must be" in rb.stderr), rb.stderr[-500:]
    contigs = open(str(tmp_path / "f.fasta")).read().split("\n")
    ids = [int(h.split("=")[1].split("_")[0]) for h in contigs[0::2] if h]
    tg = [np.zeros(0, np.uint8)] * (max(ids) + 1)
    for j, s in zip(ids, [codes(s) for s in contigs[1::2] if s]):
        tg[j] = s
    rows, lens = P.nodes_of([x for pair in zip(m1, m2) for x in pair])
    pair_off = np.array([1, 1, 2, 2] * len(m1), dtype=np.uint8)
    tw, tb, tl = P.ragged(tg, [0] * len(tg))
    # the Python API and the checker on the same contigs, the same rounds
    pl = eng.place_reads(rows, lens, targets=(tw, tb, tl), pair_off=pair_off)
    want_pl, seqs, said = P.place(rows, lens, pair_off, tw, tb, tl), tg, []
    for rnd in (1, 2):
        gw = eng.grow_ends(rows, lens, pl, min_anchor=25, min_cover=2)
        want = GC.grow_index(rows, lens, want_pl, seqs, min_anchor=25, min_cover=2)
        assert_same(gw.to_host(), want, ("the command line's contigs", rnd))
        i = gw.info
        said.append("Contig ends grown, round %d: %d candidates, %d voting, %d ends grown, %d bases added, N50 %d -> %d;" % (
            rnd, i["candidates"], i["voting"], i["ends_grown"], i["bases_added"], i["n50_before"], i["n50_after"]))
        if not i["bases_added"]:
            break
        pl = eng.place_reads(rows, lens, targets=gw.targets(), pair_off=pair_off)
        seqs = GC.sequences(want)
        want_pl = P.place(rows, lens, pair_off, *P.ragged(seqs, [0] * len(seqs)))
    print(said, r.stderr[-1500:])
    assert all(line in r.stderr for line in said), r.stderr[-3000:]
    assert gw.info["n50_after"] >= gw.info["n50_before"] and "bases added" in said[0] and " 0 bases added" not in said[0]
    eng.write_grown_fasta(str(tmp_path / "api.fasta"), gw)
    assert open(str(tmp_path / "g.fasta"), "rb").read() == open(str(tmp_path / "api.fasta"), "rb").read() == GC.fasta(want)
    assert open(str(tmp_path / "g.tsv"), "rb").read() == gw.grow_tsv().encode() == GC.grow_tsv(want)
    sc = eng.scaffold(rows, lens, pair_off, pl)
    eng.write_scaffold_fasta(str(tmp_path / "api_s.fasta"), pl, sc)
    assert open(str(tmp_path / "s.fasta"), "rb").read() == open(str(tmp_path / "api_s.fasta"), "rb").read()
    assert open(str(tmp_path / "l.tsv"), "rb").read() == sc.layout_tsv().encode()
