"""The gapped placement on the GPU (alga_place_gapped_device, alga_write_gapped_tsv_device): every output array, CIGAR and counter equal to the
Python definition (tests/gapped_checker.py) on the cases of tests/gapped_cases.py, from host arrays and from tensors and with directories of 1
and auto bits; the TSV bytes; a wave of k_gp_score that takes a second read; refusals leave an earlier result valid and the placement stays
valid after a call; the caller's stream; the one index workspace shared with the placement and the merge stage; the planted set; the command
line."""
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import gapped_cases as QC
import gapped_checker as GC
import place_checker as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what=""):
    for k in GC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert (got[k] == want[k]).all(), (what, k, np.nonzero(got[k] != want[k])[0][:10], got[k][got[k] != want[k]][:10], want[k][got[k] != want[k]][:10])
    info = {k: v for k, v in got["info"].items() if not k.startswith("ms_")}
    assert info == want["info"], (what, info, want["info"])


def place(eng, c, tg=None):
    return eng.place_reads(c["rows"], c["lens"], targets=tg if tg is not None else QC.targets(c), **c["place"])


def assert_placed(pl, want, what=""):
    got = pl.to_host()
    for k in P.ARRAYS:
        assert (got[k] == want[k]).all(), (what, k)


@pytest.mark.parametrize("name", sorted(QC.CASES))
def test_every_case_equals_the_checker(eng, name, tmp_path):
    import torch
    c = QC.case(name)
    path = str(tmp_path / "g.tsv")
    pl = place(eng, c)
    assert_placed(pl, QC.placed(name), name)
    try:
        for i, v in enumerate(c["variants"]):
            want = QC.checked(name, i)
            for bits in (1, 0):
                eng.set_option("place_dir_bits", bits)
                gp = eng.place_gapped(c["rows"], c["lens"], pl, targets=QC.targets(c), **v)
                got = gp.to_host()
                assert_same(got, want, (name, i, "host arrays", bits))
            assert (gp.n_reads, gp.n_targets, gp.n_columns, gp.n_cigar) == (len(c["lens"]) // 2, len(c["tlen"]), int(c["tlen"].sum()), len(want["cigar"]))
            assert gp.cigar_strings() == gp.cigar_strings(got) == GC.cigar_strings(want)
            info = eng.write_gapped_tsv(path, gp)
            text = open(path, "rb").read()
            assert text == GC.tsv(want), (name, i)
            assert info["segments"] == want["info"]["placed"] and info["bytes"] == len(text)
            assert_placed(pl, QC.placed(name), (name, i, "the placement after the call"))
            print(name, i, gp.info)
    finally:
        eng.set_option("place_dir_bits", 0)
    # from tensors: they are used where they are and left untouched
    dev = [torch.from_numpy(c["rows"].view(np.int32)).cuda(), torch.from_numpy(c["lens"]).cuda(), torch.from_numpy(c["twords"].view(np.int32)).cuda(),
           torch.from_numpy(c["tbegin"]).cuda(), torch.from_numpy(c["tlen"]).cuda()]
    keep = [x.clone() for x in dev]
    pl = eng.place_reads(dev[0], dev[1], targets=tuple(dev[2:]), **c["place"])
    for i, v in enumerate(c["variants"]):
        assert_same(eng.place_gapped(dev[0], dev[1], pl, targets=tuple(dev[2:]), **v).to_host(), QC.checked(name, i), (name, i, "tensors"))
    for a, b in zip(dev, keep):
        assert (a == b).all()


def test_a_wave_takes_a_second_read(eng):
    import torch
    waves = 8 * 4 * torch.cuda.get_device_properties(0).multi_processor_count  # k_gp_score: 8 blocks of 4 waves per CU
    c = QC.many_reads(waves + 300)
    pl = place(eng, c)
    want = GC.gapped_banded(c["rows"], c["lens"], pl.to_host(), *QC.targets(c))
    gp = eng.place_gapped(c["rows"], c["lens"], pl, targets=QC.targets(c))
    assert_same(gp.to_host(), want, "many reads")
    print(gp.info)
    assert gp.info["tried"] == waves + 300 and gp.info["placed"] == gp.info["unique"] == gp.info["with_indel"] == waves + 300


def test_refusals_leave_an_earlier_result_valid(eng, tmp_path):
    c, want = QC.case("uniqueness"), QC.checked("uniqueness")
    tg = QC.targets(c)
    pl = place(eng, c)
    gp = eng.place_gapped(c["rows"], c["lens"], pl, targets=tg)
    assert_same(gp.to_host(), want, "before")
    shorter, longer = c["tlen"].copy(), c["tlen"].copy()
    shorter[0] -= 1
    longer[1] += 1
    swapped = c["tlen"].copy()
    swapped[0], swapped[1] = swapped[0] - 1, swapped[1] + 1                       # the same n_columns, other targets
    rows = c["rows"].copy()
    rows[0, 0] ^= 1
    calls = [dict(k=7), dict(k=32), dict(max_edits=0), dict(max_edits=16), dict(max_occ=0), dict(max_occ=65536), dict(flags=1), dict(tlen=shorter), dict(tlen=longer),
             dict(tlen=swapped), dict(tlen=c["tlen"][:2]), dict(rows=rows), dict(rows=c["rows"][:4], lens=c["lens"][:4])]
    for change in calls:
        t2 = (c["twords"], c["tbegin"][:len(change["tlen"])] if "tlen" in change else c["tbegin"], change.get("tlen", c["tlen"]))
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.place_gapped(change.get("rows", c["rows"]), change.get("lens", c["lens"]), pl, targets=t2, **{k: v for k, v in change.items() if k not in ("tlen", "rows", "lens")})
        assert ei.value.code == -1, (list(change), ei.value)
        assert_same(gp.to_host(), want, ("after a refusal", list(change)))          # nothing written: the earlier result as it was
    with pytest.raises(TypeError):
        eng.place_gapped(c["rows"], c["lens"], pl, targets=tg, max_mismatches=1)
    # a stale placement: the engine has placed other reads since
    o = QC.case("overhang")
    pl2 = place(eng, o)
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.place_gapped(c["rows"], c["lens"], pl, targets=tg)
    assert ei.value.code == -1
    assert_same(gp.to_host(), want, "after the stale placement")
    path = str(tmp_path / "g.tsv")
    eng.write_gapped_tsv(path, gp)
    assert open(path, "rb").read() == GC.tsv(want)
    again = eng.place_gapped(o["rows"], o["lens"], pl2, targets=QC.targets(o), **o["variants"][0])
    assert_same(again.to_host(), QC.checked("overhang"), "the engine afterwards")
    assert_placed(pl2, QC.placed("overhang"), "the placement stays valid after a call")
    eng.polish(o["rows"], o["lens"], pl2)                                        # ... and is still the engine's current one
    with pytest.raises(alga_amd.AlgaError):
        eng.write_gapped_tsv(path, gp)                                           # `gp` is the result before the last one
    eng.write_gapped_tsv(path, again)
    assert open(path, "rb").read() == GC.tsv(QC.checked("overhang"))


def test_the_callers_stream_and_the_one_index_workspace(eng):
    """place -> gapped -> merge on one engine with different k and directory widths, the gapped call on the caller's stream: each equal to its
    checker -- no index, directory size, k or usable-seed mask is left over from the call before"""
    import torch
    import merge_cases as MQ
    import merge_checker as MC
    c = QC.case("read_lengths")
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            dev = [torch.from_numpy(c["rows"].view(np.int32)).cuda(), torch.from_numpy(c["lens"]).cuda(), torch.from_numpy(c["twords"].view(np.int32)).cuda(),
                   torch.from_numpy(c["tbegin"]).cuda(), torch.from_numpy(c["tlen"]).cuda()]
        assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
        s.synchronize()
        pl = eng.place_reads(dev[0], dev[1], targets=tuple(dev[2:]), **c["place"])                      # k = 21
        eng.set_option("place_dir_bits", 3)
        gp = eng.place_gapped(dev[0], dev[1], pl, targets=tuple(dev[2:]), stream=s.cuda_stream, **c["variants"][1])   # k = 8, 128 seeds
        assert s.query()                                                         # the call returns with its work on the stream done
        assert_same(gp.to_host(), QC.checked("read_lengths", 1), "gapped, k = 8, 3 directory bits, the caller's stream")
        m = MQ.case("seeds64")
        mg = eng.merge_ends(MQ.targets(m), **m["variants"][0])
        want = MQ.checked("seeds64")
        for k in MC.ARRAYS:
            assert (mg.to_host()[k] == want[k]).all(), k
        eng.set_option("place_dir_bits", 0)
        assert_same(gp.to_host(), QC.checked("read_lengths", 1), "the gapped result after the merge")
        assert_same(eng.place_gapped(dev[0], dev[1], pl, targets=tuple(dev[2:])).to_host(), QC.checked("read_lengths", 0), "gapped, k = 21, on the engine's stream")
    finally:
        eng.set_option("place_dir_bits", 0)


def test_planted_set(eng):
    """6 kb, 30x reads of 100 nt with one planted 1-base indel each: equal to the checker, and every read that keeps a seed whose k-mer is unique
    in the genome is UNIQUE at its true locus (tests/test_gapped_cpu.py shows the same of the checker)"""
    c, start, minus = QC.planted()
    pl = place(eng, c)
    gp = eng.place_gapped(c["rows"], c["lens"], pl, targets=QC.targets(c))
    got = gp.to_host()
    assert_same(got, GC.gapped_banded(c["rows"], c["lens"], pl.to_host(), *QC.targets(c)), "planted")
    E, k = GC.DEFAULT["max_edits"], GC.DEFAULT["k"]
    occ = {x: len(v) for x, v in P._index(c["seqs"], k).items()}
    plh = pl.to_host()
    for r in range(len(start)):
        if plh["state"][r] & P.PLACED:
            continue
        seeds = [int(x) for node in (2 * r + 1, 2 * r) for x in P.kmer_values(P.codes_of(c["rows"][node], 0, int(c["lens"][node])), k)[::k]]
        if any(occ.get(x, 0) == 1 for x in seeds):
            assert got["state"][r] & GC.UNIQUE and got["target"][r] == 0 and bool(got["state"][r] & GC.MINUS) == bool(minus[r]) and abs(int(got["pos"][r]) - int(start[r])) <= E, r
    print(gp.info)


def test_on_the_final_contigs(eng):
    """Engine.place_gapped(final=...): the targets of alga_place_reads_on_final_device made again from the final result.  The contig set: 14
    reads without an edge, every one a contig of its own (tests/place_cases.py: header_nodes)"""
    import place_cases as PC
    words, lens = PC.header_nodes()
    u = eng.unitigs(words, lens, np.zeros((0, 3), np.int32), skip_isolated=False)
    cs = eng.unitig_consensus(words, lens, u, min_votes=0)
    fin = eng.final_contigs(u, cs, 1, 95, 0)
    uh, ch, fh = u.to_host(), cs.to_host(), fin.to_host()
    order = fh["order"].astype(np.int64)
    live = fh["verdict"][order] == 2
    tw, tb = ch["words"], 16 * uh["word_off"].astype(np.int64)[order] + np.where(live, fh["begin"][order], 0)
    tl = np.where(live, fh["len"][order], 0).astype(np.int32)
    contigs = [P.codes_of(tw, tb[j], int(tl[j])) for j in range(len(tl))]
    big = [c for c in contigs if len(c) >= 300]
    assert len(big) >= 5
    reads = [QC.edit(c[50:201], [("D", 60, 1)]) for c in big] + [QC.edit(c[80:229], [("I", 90, QC.other(c[170]))]) for c in big] + [big[0][10:160], P.revcomp(big[1][100:250])]
    rows, rlens = P.nodes_of(reads)
    pl = eng.place_reads(rows, rlens, final=fin, max_mismatches=0)
    gp = eng.place_gapped(rows, rlens, pl, final=fin)
    want = GC.gapped_banded(rows, rlens, pl.to_host(), tw, tb, tl)
    assert_same(gp.to_host(), want, "on the final contigs")
    assert pl.info["placed"] == 2 and want["info"]["placed"] == want["info"]["unique"] == want["info"]["with_indel"] == 2 * len(big)
    with pytest.raises(alga_amd.AlgaError) as ei:                                # other targets than the placement's
        eng.place_gapped(rows, rlens, pl, targets=(tw, tb[:-1], tl[:-1]))
    assert ei.value.code == -1
    assert_same(gp.to_host(), want, "after the refusal")


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, c in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in c)))


def codes(s):
    return np.array(["ACGT".index(x) for x in s], dtype=np.uint8)


def test_command_line(eng, tmp_path):
    """reads of a 3 kb genome, every fifth with one planted 1-base indel.  alga_hip with --gapped=1 --gapped_placements=: the TSV is the checker's
    text for the contigs the run writes (placed by the checker with the command line's defaults), the stderr line carries its counters; without
    --gapped=1 and with --gapped=0 every other file is what it was"""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    rng = np.random.default_rng(77)
    g = rng.integers(0, 4, size=3000, dtype=np.uint8)
    reads = []
    for n, a in enumerate(rng.permutation(np.arange(0, 3000 - 101, 3))):
        a = int(a)
        if n % 5 == 0:
            at = int(rng.integers(5, 95))
            reads.append(QC.edit(g[a:a + 101], [("D", at, 1)]) if n % 10 else QC.edit(g[a:a + 99], [("I", at, QC.other(g[a + at]))]))
        else:
            reads.append(g[a:a + 100])
    _write_fasta(str(tmp_path / "a.fasta"), reads)
    base = [exe, "--file1=a.fasta", "--output=o.fasta", "--contigs_min_length=150", "--consensus_min_votes=0", "--retl=0", "--retr=0"]
    run = lambda args: subprocess.run(args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    r0 = run(base + ["--contigs_final=f0.fasta", "--contigs_depth=1", "--placements=p0.tsv"])
    assert r0.returncode == 0, r0.stderr[-2000:]
    r1 = run(base + ["--contigs_final=f1.fasta", "--contigs_depth=1", "--placements=p1.tsv", "--gapped=0"])
    assert r1.returncode == 0 and "laid with indels" not in r0.stderr + r1.stderr, r1.stderr[-2000:]
    r = run(base + ["--contigs_final=f.fasta", "--contigs_depth=1", "--placements=p.tsv", "--gapped=1", "--gapped_placements=g.tsv"])
    assert r.returncode == 0, r.stderr[-2000:]
    for a, b in (("f0.fasta", "f1.fasta"), ("p0.tsv", "p1.tsv"), ("f0.fasta", "f.fasta"), ("p0.tsv", "p.tsv")):   # the depth headers and --placements= stay as they are
        assert open(str(tmp_path / a), "rb").read() == open(str(tmp_path / b), "rb").read(), a
    r3 = run(base + ["--contigs_final=f3.fasta", "--gapped=1", "--gapped_edits=1", "--gapped_placements=g3.tsv"])
    assert r3.returncode == 0, r3.stderr[-2000:]
    for bad in (["--gapped=1"], ["--contigs_final=f2.fasta", "--gapped_placements=g2.tsv"], ["--contigs_final=f2.fasta", "--gapped_edits=3"],
                ["--contigs_final=f2.fasta", "--gapped=2"], ["--contigs_final=f2.fasta", "--gapped=1", "--gapped_edits=0"],
                ["--contigs_final=f2.fasta", "--gapped=1", "--gapped_edits=16"]):
        rb = run([exe, "--file1=a.fasta", "--output=o2.fasta"] + bad)
        assert rb.returncode == 2 and ("need" in rb.stderr or "must be" in rb.stderr), rb.stderr[-500:]
    contigs = open(str(tmp_path / "f.fasta")).read().split("\n")
    ids = [int(h.split("=")[1].split("_")[0]) for h in contigs[0::2] if h]
    tg = [np.zeros(0, np.uint8)] * (max(ids) + 1)
    for j, s in zip(ids, [codes(s) for s in contigs[1::2] if s]):
        tg[j] = s
    rows, lens = P.nodes_of(reads)
    tw, tb, tl = P.ragged(tg, [0] * len(tg))
    plh = P.place(rows, lens, None, tw, tb, tl)
    for edits, name, res in ((6, "g.tsv", r), (1, "g3.tsv", r3)):
        want = GC.gapped_banded(rows, lens, plh, tw, tb, tl, max_edits=edits)
        i = want["info"]
        assert open(str(tmp_path / name), "rb").read() == GC.tsv(want), name
        said = "Unplaced reads laid with indels (up to %d edits): %d tried, %d placed, %d unique, %d with indel, %d edits;" % (
            edits, i["tried"], i["placed"], i["unique"], i["with_indel"], i["edits"])
        print(said)
        assert said in res.stderr, res.stderr[-3000:]
    assert i["placed"] >= 1 and i["with_indel"] >= 1                             # (the text compared above is not empty)
    # the Python API on the same contigs
    pl = eng.place_reads(rows, lens, targets=(tw, tb, tl))
    gp = eng.place_gapped(rows, lens, pl, targets=(tw, tb, tl), max_edits=1)
    assert_same(gp.to_host(), want, "the command line's contigs")
    eng.write_gapped_tsv(str(tmp_path / "api.tsv"), gp)
    assert open(str(tmp_path / "api.tsv"), "rb").read() == open(str(tmp_path / "g3.tsv"), "rb").read()
