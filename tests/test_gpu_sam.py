"""The pair calls over both placement passes and the SAM writer on the GPU (alga_judge_pairs_device, alga_write_sam_device): every array, counter
and histogram bin and every byte of the text equal to the Python definition (tests/sam_checker.py) on the cases of tests/sam_cases.py, from
host arrays and from tensors, with both name forms and both values of the skip flag; every file passes tests/sam_invariants.py; the Hamming-only
calls against the existing k_pl_pairs; grids that make a thread and a wave take a second item, a text in several chunks; refusals leave an
earlier result valid; the engine's placement and gapped result stay current; the caller's stream; the command line."""
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import gapped_cases as QC
import gapped_checker as GC
import place_cases as PC
import place_checker as P
import sam_cases as SQ
import sam_checker as SC
import sam_invariants as SI

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_calls(got, want, what=""):
    for k in SC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert (got[k] == want[k]).all(), (what, k, np.nonzero(got[k] != want[k])[0][:10], got[k][got[k] != want[k]][:10], want[k][got[k] != want[k]][:10])
    info = {k: v for k, v in got["info"].items() if not k.startswith("ms_")}
    assert info == want["info"], (what, info, want["info"])


def both_passes(eng, c, rows=None, lens=None, po=None, tg=None):
    rows, lens, po, tg = (c["rows"] if rows is None else rows), (c["lens"] if lens is None else lens), (c["pair_off"] if po is None else po), tg or SQ.targets(c)
    pl = eng.place_reads(rows, lens, targets=tg, pair_off=po, **c["place"])
    gp = eng.place_gapped(rows, lens, pl, targets=tg, **c["gapped"])
    return pl, gp


@pytest.mark.parametrize("name", sorted(SQ.CASES))
def test_every_case_equals_the_checker(eng, name, tmp_path):
    import torch
    w = SQ.checked(name)
    c = w["case"]
    path = str(tmp_path / "r.sam")
    pl, gp = both_passes(eng, c)
    for k in P.ARRAYS:
        assert (pl.to_host()[k] == w["pl"][k]).all(), (name, k)
    for k in GC.ARRAYS:
        assert (gp.to_host()[k] == w["gp"][k]).all(), (name, k)
    for g, want in ((gp, w["calls"]), (None, w["no_gp"])):
        calls = eng.judge_pairs(c["rows"], c["lens"], pl, gapped=g, pair_off=c["pair_off"], max_insert=c["max_insert"])
        assert_calls(calls.to_host(), want, (name, "host arrays", g is not None))
        assert (calls.n_reads, calls.n_hist) == (len(c["lens"]) // 2, c["max_insert"] + 1)
        for flags in (0, SC.NAMES_DEPTH, SC.SKIP_UNPLACED, SC.NAMES_DEPTH | SC.SKIP_UNPLACED):
            info = eng.write_sam(path, c["rows"], c["lens"], pl, calls, gapped=g, names_depth=bool(flags & SC.NAMES_DEPTH), skip_unplaced=bool(flags & SC.SKIP_UNPLACED))
            text = open(path, "rb").read()
            assert text == SC.sam(c["rows"], c["lens"], c["pair_off"], w["pl"], w["gp"] if g is not None else None, want, flags), (name, flags, g is not None)
            assert info["bytes"] == len(text) and info["segments"] == sum(1 for s in text.split(b"\n") if s and not s.startswith(b"@"))
            SI.check(text, c["reads"], c["seqs"], complete=not flags & SC.SKIP_UNPLACED)
        print(name, g is not None, calls.info)
    # from tensors: they are used where they are and left untouched
    dev = [torch.from_numpy(c["rows"].view(np.int32)).cuda(), torch.from_numpy(c["lens"]).cuda(), torch.from_numpy(c["twords"].view(np.int32)).cuda(),
           torch.from_numpy(c["tbegin"]).cuda(), torch.from_numpy(c["tlen"]).cuda()]
    po = torch.from_numpy(c["pair_off"]).cuda() if c["pair_off"] is not None else None
    keep = [x.clone() for x in dev]
    pl, gp = both_passes(eng, c, dev[0], dev[1], po, tuple(dev[2:]))
    calls = eng.judge_pairs(dev[0], dev[1], pl, gapped=gp, pair_off=po, max_insert=c["max_insert"])
    assert_calls(calls.to_host(), w["calls"], (name, "tensors"))
    eng.write_sam(path, dev[0], dev[1], pl, calls, gapped=gp)
    assert open(path, "rb").read() == w["text"]
    for a, b in zip(dev, keep):
        assert (a == b).all()


@pytest.mark.parametrize("name", ["pairs", "rand"])
def test_hamming_only_equals_the_placements_own_pairs(eng, name):
    """k_sam_judge against the existing k_pl_pairs: with no gapped read and the placement's max_insert, counter for counter and bin for bin (every
    paired read of these two cases is live)"""
    c = PC.case(name)
    assert all(min(c["lens"][2 * r + 1], c["lens"][2 * r + 3]) >= 1 for r in range(len(c["lens"]) // 2) if c["pair_off"][2 * r + 1] == 1)
    pl = eng.place_reads(c["rows"], c["lens"], targets=(c["twords"], c["tbegin"], c["tlen"]), pair_off=c["pair_off"], **c["params"])
    calls = eng.judge_pairs(c["rows"], c["lens"], pl, pair_off=c["pair_off"], max_insert=c["params"].get("max_insert", 1000))
    for k in SC.PAIR_COUNTERS:
        assert calls.info[k] == pl.info[k], (k, calls.info, pl.info)
    assert pl.info["pairs_proper"] >= 1 and (calls.insert_hist == pl.insert_hist).all() and calls.info["pairs_with_gapped"] == 0
    want = SC.pair_calls(c["lens"], c["pair_off"], pl.to_host(), None, c["params"].get("max_insert", 1000))
    assert_calls(calls.to_host(), want, name)


def test_the_loops_go_round_and_the_text_comes_in_chunks(eng, tmp_path):
    """With the grids capped at 2 blocks a thread of k_sam_judge (512 threads) and a wave of k_sam_write (8 waves) take many items; 9000 pairs
    drawn from a pool of 36 give a text above 2 MiB, written in chunks of 1 MiB.  The expectation is computed per distinct pair: the two
    placements of the big set are the pool's, tiled (asserted), and tests/test_sam_cpu.py shows that the checker's records of a drawn pair are
    the pool pair's but for the read index"""
    n_pairs = 9000
    c, n_pool = SQ.many_pairs(n_pairs)
    pool, _ = SQ.many_pairs(n_pool)
    ppl = P.place(pool["rows"], pool["lens"], pool["pair_off"], *SQ.targets(pool), **pool["place"])
    pgp = GC.gapped_banded(pool["rows"], pool["lens"], ppl, *SQ.targets(pool), **pool["gapped"])
    src = np.array([2 * (i % n_pool) + h for i in range(n_pairs) for h in (0, 1)])            # the pool read behind every read (7 and 36 are coprime)
    path = str(tmp_path / "big.sam")
    try:
        eng.set_option("sam_max_blocks", 2)
        eng.set_option("gfa_chunk_mb", 1)
        pl, gp = both_passes(eng, c)
        plh, gph = pl.to_host(), gp.to_host()
        for k in ("target", "pos", "mm", "hits", "state"):
            assert (plh[k] == ppl[k][src]).all(), k
        for k in ("target", "pos", "end", "edits", "state"):
            assert (gph[k] == pgp[k][src]).all(), k
        cg = GC.cigar_strings(pgp)
        assert GC.cigar_strings(gph) == [cg[j] for j in src]
        calls = eng.judge_pairs(c["rows"], c["lens"], pl, gapped=gp, pair_off=c["pair_off"])
        want = SC.pair_calls(c["lens"], c["pair_off"], plh, gph)
        assert_calls(calls.to_host(), want, "many pairs")
        small = SC.pair_calls(pool["lens"], pool["pair_off"], ppl, pgp)
        assert (want["flag"] == small["flag"][src]).all() and (want["tlen"] == small["tlen"][src]).all()
        assert want["info"]["proper_with_gapped"] >= 500 and want["info"]["unplaced"] >= 1000 and want["info"]["pairs"] == n_pairs
        info = eng.write_sam(path, c["rows"], c["lens"], pl, calls, gapped=gp)
        text = open(path, "rb").read()
        assert text == SC.sam(c["rows"], c["lens"], c["pair_off"], plh, gph, want)
        assert len(text) > 2 << 20 and info["bytes"] == len(text) and info["segments"] == 2 * n_pairs
        # records begin at several residues mod 16 of the chunk buffer (the first chunk begins behind the header)
        head = len(SC.header(plh))
        starts, at = set(), head
        for s in text[head:head + (1 << 19)].split(b"\n")[:-1]:
            starts.add((at - head) % 16)
            at += len(s) + 1
        assert len(starts) >= 8, starts
    finally:
        eng.set_option("sam_max_blocks", 0)
        eng.set_option("gfa_chunk_mb", 256)


def test_refusals_leave_an_earlier_result_valid(eng, tmp_path):
    w = SQ.checked("proper")
    c = w["case"]
    path, other_path = str(tmp_path / "r.sam"), str(tmp_path / "untouched.sam")
    pl, gp = both_passes(eng, c)
    args = dict(gapped=gp, pair_off=c["pair_off"], max_insert=c["max_insert"])
    calls = eng.judge_pairs(c["rows"], c["lens"], pl, **args)
    assert_calls(calls.to_host(), w["calls"], "before")
    open(other_path, "wb").write(b"kept")

    def refused(f, *a, **k):
        with pytest.raises(alga_amd.AlgaError) as ei:
            f(*a, **k)
        assert ei.value.code == -1, ei.value
        assert_calls(calls.to_host(), w["calls"], ("after a refusal", a[3:], sorted(k)))       # nothing written: the earlier result as it was
        eng.write_sam(path, c["rows"], c["lens"], pl, calls, gapped=gp)
        assert open(path, "rb").read() == w["text"] and open(other_path, "rb").read() == b"kept"
    bad_po = [c["pair_off"].copy() for _ in range(4)]
    bad_po[0][0] = 3                                                             # a value above 2
    bad_po[1][0] = 0                                                             # differs from its twin
    bad_po[2][-1] = bad_po[2][-2] = 1                                            # the mate is out of range
    bad_po[3][2] = bad_po[3][3] = 0                                              # the mate does not point back
    for po in bad_po:
        refused(eng.judge_pairs, c["rows"], c["lens"], pl, **dict(args, pair_off=po))
    for change in (dict(max_insert=0), dict(max_insert=(1 << 20) + 1), dict(flags=1), dict(reserved=1)):
        refused(eng.judge_pairs, c["rows"], c["lens"], pl, **dict(args, **change))
    refused(eng.judge_pairs, c["rows"][:4], c["lens"][:4], pl, **dict(args, pair_off=c["pair_off"][:4]))     # a wrong read count
    for change in (dict(flags=4), dict(reserved=1)):
        refused(eng.write_sam, other_path, c["rows"], c["lens"], pl, calls, gapped=gp, **change)
    refused(eng.write_sam, other_path, c["rows"], c["lens"], pl, calls, gapped=None)                         # calls made with a gapped result, written without
    refused(eng.write_sam, other_path, c["rows"][:4], c["lens"][:4], pl, calls, gapped=gp)
    # on the device, in the sizes pass: a node set whose reads are not the placed ones (a G read's script has another length); a length above the stride
    lens = c["lens"].copy()
    lens[6] = lens[7] = lens[7] - 1
    refused(eng.write_sam, other_path, c["rows"], lens, pl, calls, gapped=gp)
    lens = c["lens"].copy()
    lens[0] = lens[1] = 16 * c["rows"].shape[1] + 1
    refused(eng.write_sam, other_path, c["rows"], lens, pl, calls, gapped=gp)
    # a gapped result and pair calls of an earlier placement; then a stale placement: the engine has placed other reads since
    pl2 = eng.place_reads(c["rows"], c["lens"], targets=SQ.targets(c), pair_off=c["pair_off"], **c["place"])
    o = SQ.case("singles")
    for step in range(3):
        with pytest.raises(alga_amd.AlgaError) as ei:
            if step == 0:
                eng.judge_pairs(c["rows"], c["lens"], pl2, **args)
            elif step == 1:
                eng.write_sam(other_path, c["rows"], c["lens"], pl2, calls, gapped=None)
            else:
                eng.place_reads(o["rows"], o["lens"], targets=SQ.targets(o), **o["place"])
                eng.judge_pairs(c["rows"], c["lens"], pl2, pair_off=c["pair_off"], max_insert=c["max_insert"])
        assert ei.value.code == -1
        assert_calls(calls.to_host(), w["calls"], ("after a stale input", step))
    assert open(other_path, "rb").read() == b"kept"
    # calls made without a gapped result are refused with one, and the other way round
    pl2 = eng.place_reads(c["rows"], c["lens"], targets=SQ.targets(c), pair_off=c["pair_off"], **c["place"])
    gp2 = eng.place_gapped(c["rows"], c["lens"], pl2, targets=SQ.targets(c), **c["gapped"])
    calls_h = eng.judge_pairs(c["rows"], c["lens"], pl2, pair_off=c["pair_off"], max_insert=c["max_insert"])
    assert_calls(calls_h.to_host(), w["no_gp"], "the Hamming pass alone")
    with pytest.raises(alga_amd.AlgaError):
        eng.write_sam(other_path, c["rows"], c["lens"], pl2, calls_h, gapped=gp2)
    eng.write_sam(path, c["rows"], c["lens"], pl2, calls_h)
    assert open(path, "rb").read() == SC.sam(c["rows"], c["lens"], c["pair_off"], w["pl"], None, w["no_gp"])
    # a second gapped result of the same placement: calls made from the first are refused
    calls2 = eng.judge_pairs(c["rows"], c["lens"], pl2, gapped=gp2, pair_off=c["pair_off"], max_insert=c["max_insert"])
    gp3 = eng.place_gapped(c["rows"], c["lens"], pl2, targets=SQ.targets(c), **dict(c["gapped"], max_edits=1))
    with pytest.raises(alga_amd.AlgaError):
        eng.write_sam(other_path, c["rows"], c["lens"], pl2, calls2, gapped=gp3)
    assert open(other_path, "rb").read() == b"kept"


def test_engine_state_and_the_callers_stream(eng, tmp_path):
    """pl and gp are still the engine's current results after both calls (the indel polish takes them); the judge runs on the caller's stream"""
    import torch
    w = SQ.checked("insert_bound")
    c = w["case"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = [torch.from_numpy(c["rows"].view(np.int32)).cuda(), torch.from_numpy(c["lens"]).cuda(), torch.from_numpy(c["pair_off"]).cuda()]
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    s.synchronize()
    pl, gp = both_passes(eng, c, dev[0], dev[1], dev[2])
    calls = eng.judge_pairs(dev[0], dev[1], pl, gapped=gp, pair_off=dev[2], max_insert=c["max_insert"], stream=s.cuda_stream)
    assert s.query()                                                             # the call returns with its work on the stream done
    assert_calls(calls.to_host(), w["calls"], "the caller's stream")
    path = str(tmp_path / "r.sam")
    eng.write_sam(path, dev[0], dev[1], pl, calls, gapped=gp)
    assert open(path, "rb").read() == w["text"]
    for k in P.ARRAYS:
        assert (pl.to_host()[k] == w["pl"][k]).all(), k
    for k in GC.ARRAYS:
        assert (gp.to_host()[k] == w["gp"][k]).all(), k
    ip = eng.polish_indels(dev[0], dev[1], pl, gp)                               # ... and both are still the engine's current ones
    assert ip.info["voters_gapped"] == w["gp"]["info"]["unique"]
    eng.write_gapped_tsv(path, gp)
    assert open(path, "rb").read() == GC.tsv(w["gp"])
    assert_calls(eng.judge_pairs(dev[0], dev[1], pl, gapped=gp, pair_off=dev[2], max_insert=c["max_insert"]).to_host(), w["calls"], "on the engine's stream")


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, c in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in c)))


def codes(s):
    return np.array(["ACGT".index(x) for x in s], dtype=np.uint8)


def test_command_line(eng, tmp_path):
    """pairs of a 3 kb genome, every fifth second mate with one planted 1-base indel in its middle (the assembly is that of the exact reads).  alga_hip --sam=: the text is the checker's for the contigs
    the run writes (placed by the checkers with the command line's defaults), with and without --gapped=1 and --contigs_depth=1 and with
    --sam_unplaced=0; the @SQ names are the first tokens of the same run's FASTA headers; every other file is what it is without --sam=; the
    stderr line carries the checker's counters; the refusals exit 2"""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    rng = np.random.default_rng(78)
    g = rng.integers(0, 4, size=3000, dtype=np.uint8)
    m1, m2 = [], []
    for n, a in enumerate(rng.permutation(np.arange(0, 3000 - 300, 5))):
        a, ins = int(a), int(rng.integers(250, 299))
        m1.append(g[a:a + 100])
        if n % 5 == 0:
            at = 50                                                              # no exact overlap of 55 (0.55 of the read length) is left: the read joins no contig
            w = QC.edit(g[a + ins - 100:a + ins + 1], [("D", at, 1)]) if n % 10 else QC.edit(g[a + ins - 100:a + ins - 1], [("I", at, QC.other(g[a + ins - 100 + at]))])
        else:
            w = g[a + ins - 100:a + ins]
        m2.append(P.revcomp(w))
    _write_fasta(str(tmp_path / "a.fasta"), m1)
    _write_fasta(str(tmp_path / "b.fasta"), m2)
    base = [exe, "--file1=a.fasta", "--file2=b.fasta", "--output=o.fasta", "--contigs_min_length=150", "--consensus_min_votes=0", "--retl=0", "--retr=0"]
    run = lambda args: subprocess.run(args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    read = lambda name: open(str(tmp_path / name), "rb").read()
    r0 = run(base + ["--contigs_final=f0.fasta", "--contigs_depth=1", "--placements=p0.tsv", "--gapped=1", "--gapped_placements=g0.tsv"])
    assert r0.returncode == 0 and "SAM written" not in r0.stderr, r0.stderr[-2000:]
    r1 = run(base + ["--contigs_final=f1.fasta", "--contigs_depth=1", "--placements=p1.tsv", "--gapped=1", "--gapped_placements=g1.tsv", "--sam=s1.sam"])
    assert r1.returncode == 0, r1.stderr[-2000:]
    for a, b in (("f0.fasta", "f1.fasta"), ("p0.tsv", "p1.tsv"), ("g0.tsv", "g1.tsv")):      # every other file is what it was
        assert read(a) == read(b), a
    r2 = run(base + ["--contigs_final=f2.fasta", "--sam=s2.sam"])
    assert r2.returncode == 0 and "laid with indels" not in r2.stderr, r2.stderr[-2000:]
    r3 = run(base + ["--contigs_final=f3.fasta", "--gapped=1", "--sam=s3.sam", "--sam_unplaced=0"])
    assert r3.returncode == 0, r3.stderr[-2000:]
    for bad in (["--sam=x.sam"], ["--contigs_final=fx.fasta", "--sam_unplaced=0"], ["--contigs_final=fx.fasta", "--sam=x.sam", "--sam_unplaced=2"],
                ["--contigs_final=fx.fasta", "--sam=x.sam", "--polish=1"]):
        rb = run([exe, "--file1=a.fasta", "--file2=b.fasta", "--output=o2.fasta"] + bad)
        assert rb.returncode == 2 and ("need" in rb.stderr or "must be" in rb.stderr), rb.stderr[-500:]
        assert not os.path.exists(str(tmp_path / "x.sam"))
    contigs = read("f2.fasta").decode().split("\n")
    ids = [int(h.split("=")[1].split("_")[0]) for h in contigs[0::2] if h]
    tg = [np.zeros(0, np.uint8)] * (max(ids) + 1)
    for j, s in zip(ids, [codes(s) for s in contigs[1::2] if s]):
        tg[j] = s
    reads = [x for pair in zip(m1, m2) for x in pair]
    rows, lens = P.nodes_of(reads)
    po = np.tile(np.array([1, 1, 2, 2], np.uint8), len(m1))
    tw, tb, tl = P.ragged(tg, [0] * len(tg))
    plh = P.place(rows, lens, po, tw, tb, tl)
    gph = GC.gapped_banded(rows, lens, plh, tw, tb, tl)
    for name, fasta, g_, flags, res in (("s1.sam", "f1.fasta", gph, SC.NAMES_DEPTH, r1), ("s2.sam", "f2.fasta", None, 0, r2), ("s3.sam", "f3.fasta", gph, SC.SKIP_UNPLACED, r3)):
        want = SC.pair_calls(lens, po, plh, g_)
        text = read(name)
        assert text == SC.sam(rows, lens, po, plh, g_, want, flags), name
        SI.check(text, reads, tg, complete=not flags & SC.SKIP_UNPLACED)
        sq = [s.split(b"\t")[1][3:] for s in text.split(b"\n") if s.startswith(b"@SQ")]
        assert sq == [h[1:].split(b" ")[0] for h in read(fasta).split(b"\n")[0::2] if h], name       # the names are the FASTA's of the same run
        i = want["info"]
        said = "%d pairs: %d proper, %d improper, %d split, %d not unique; with a gapped mate %d pairs, %d proper; median insert %d;" % (
            i["pairs"], i["pairs_proper"], i["pairs_improper"], i["pairs_split"], i["pairs_not_unique"], i["pairs_with_gapped"], i["proper_with_gapped"], i["insert_median"])
        print(name, said)
        assert said in res.stderr, res.stderr[-3000:]
    i = SC.pair_calls(lens, po, plh, gph)["info"]
    assert i["proper_with_gapped"] >= 1 and i["pairs_proper"] > SC.pair_calls(lens, po, plh, None)["info"]["pairs_proper"] >= 100
    # the Python API on the same contigs
    pl = eng.place_reads(rows, lens, targets=(tw, tb, tl), pair_off=po)
    gp = eng.place_gapped(rows, lens, pl, targets=(tw, tb, tl))
    calls = eng.judge_pairs(rows, lens, pl, gapped=gp, pair_off=po)
    eng.write_sam(str(tmp_path / "api.sam"), rows, lens, pl, calls, gapped=gp, names_depth=True)
    assert read("api.sam") == read("s1.sam")
