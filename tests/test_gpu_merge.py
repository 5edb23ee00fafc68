"""The merge stage on the GPU (alga_merge_targets_device, alga_write_merged_fasta_device): every output array and every counter equal to the
Python definition (tests/merge_checker.py) on the cases of tests/merge_cases.py, from host arrays and from tensors and with directories of 1, 4
and auto bits; the FASTA bytes and the TSV; the one index workspace shared with the placement and the grow stage, the one chain workspace shared with the
scaffolder and the stitch stage; a wave of k_mg_overlap that
takes a second end; a second round on Merged.targets(); the caller's stream; refusals leave an earlier result valid; a result stays valid across
a later placement, polish, break, grow and scaffold; the planted genome end to end; the command line."""
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import grow_cases as GQ
import grow_checker as GC
import merge_cases as QC
import merge_checker as MC
import place_checker as P

pytestmark = pytest.mark.gpu
TIMES = ("ms_index", "ms_overlap", "ms_build", "ms_total")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what=""):
    for k in MC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert (got[k] == want[k]).all(), (what, k, np.nonzero(got[k] != want[k])[0][:10])
    info = {k: v for k, v in got["info"].items() if k not in TIMES}
    assert info == want["info"], (what, info, want["info"])


def device_targets(c):
    import torch
    return torch.from_numpy(c["twords"].view(np.int32)).cuda(), torch.from_numpy(c["tbegin"]).cuda(), torch.from_numpy(c["tlen"]).cuda()


@pytest.mark.parametrize("name", sorted(QC.CASES))
def test_every_case_equals_the_checker(eng, name, tmp_path):
    c = QC.case(name)
    path = str(tmp_path / "m.fasta")
    assert len(c["tbegin"]) < 2 or sorted(set((c["tbegin"] & 15).tolist())) == sorted(set(3 * i % 16 for i in range(len(c["tbegin"]))))
    for i, v in enumerate(c["variants"]):
        want = QC.checked(name, i)
        for bits in (1, 4, 0):
            eng.set_option("place_dir_bits", bits)
            mg = eng.merge_ends(QC.targets(c), **v)
            assert_same(mg.to_host(), want, (name, i, "host arrays", bits))
        got = mg.to_host()
        assert (mg.n_targets, mg.n_merged, mg.n_members, mg.n_columns) == (len(c["tlen"]), len(want["len"]), len(want["m_members"]), int(want["col_off"][-1]))
        info = eng.write_merged_fasta(path, mg)
        text = open(path, "rb").read()
        assert text == MC.fasta(want), (name, i)
        assert info["segments"] == len(want["len"]) and info["bytes"] == len(text)
        assert mg.merge_tsv().encode() == mg.merge_tsv(c["tlen"], got).encode() == MC.merge_tsv(want, c["tlen"]), (name, i)
        print(name, i, mg.info)
    # from tensors: they are used where they are and left untouched
    tg = device_targets(c)
    keep = [x.clone() for x in tg]
    for i, v in enumerate(c["variants"]):
        assert_same(eng.merge_ends(tg, **v).to_host(), QC.checked(name, i), (name, i, "tensors"))
    for a, b in zip(tg, keep):
        assert (a == b).all()


def test_word_seams_of_the_merged_contigs(eng):
    """k_mg_build on tests/merge_cases.py: word_seams, at 8192 blocks and at one: merged contigs of 1, 15, 16, 17, 31, 32 and 33 bases around two
    joined pairs (one of them minus-oriented), a total that is no multiple of 16 (the last word partial, the two of padding zero) and, with
    merge_max_blocks 1, several words per lane.  The stage has no empty item: the empty target is in no merged contig"""
    c, want = QC.case("word_seams"), QC.checked("word_seams")
    assert want["len"].tolist() == [1, 15, 16, 17, 4450, 31, 32, 4450, 33] and want["orient"].sum() == 2 and len(c["tlen"]) == 12
    assert int(want["col_off"][-1]) % 16 and int(want["col_off"][-1]) > 16 * 256
    try:
        for blocks in (8192, 1):
            eng.set_option("merge_max_blocks", blocks)
            assert_same(eng.merge_ends(QC.targets(c)).to_host(), want, ("word_seams", blocks))
    finally:
        eng.set_option("merge_max_blocks", 8192)


def test_one_index_workspace_serves_the_stages_in_turn(eng):
    """place, merge and grow build their seed index in one workspace of the engine: on one engine, calls of different stages, k, directory
    widths and seed counts in turn, each equal to its checker -- no index, directory size, k or usable-seed mask is left over from the call
    before (many_seeds and second_chunk have reads of more than 64 seeds: they use the per-wave scratch; seeds64 has exactly 64)"""
    import grow_cases as GQC
    import place_cases as PC

    def same(got, want, arrays, what):
        for k in arrays:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
        assert {k: v for k, v in got["info"].items() if not k.startswith("ms_")} == want["info"], (what, got["info"], want["info"])

    def place(c):
        return eng.place_reads(c["rows"], c["lens"], targets=(c["twords"], c["tbegin"], c["tlen"]), pair_off=c.get("pair_off"), **c["params"])

    try:
        same(place(PC.case("many_seeds")).to_host(), PC.checked("many_seeds"), P.ARRAYS, "place many_seeds")
        eng.set_option("place_dir_bits", 3)
        c = QC.case("seeds64")
        assert c["variants"][0]["k"] == 8
        assert_same(eng.merge_ends(QC.targets(c), **c["variants"][0]).to_host(), QC.checked("seeds64"), "merge seeds64, 3 directory bits")
        c = GQC.case("second_chunk")
        pl = place(c)
        assert (pl.to_host()["state"] == GQC.placed("second_chunk")["state"]).all()
        same(eng.grow_ends(c["rows"], c["lens"], pl, **c["variants"][0]).to_host(), GQC.checked("second_chunk"), GC.ARRAYS, "grow second_chunk")
        eng.set_option("place_dir_bits", 0)
        same(place(PC.case("repeat")).to_host(), PC.checked("repeat"), P.ARRAYS, "place repeat")
        c = QC.case("pairings")
        assert_same(eng.merge_ends(QC.targets(c), **c["variants"][0]).to_host(), QC.checked("pairings"), "merge pairings")
    finally:
        eng.set_option("place_dir_bits", 0)


def test_one_chain_workspace_serves_the_stages_in_turn(tmp_path):
    """scaffold, merge and stitch order their contigs in one chain workspace of the engine (the two sets of lists over the 2T states, join, head,
    first / members and their scans, carved for the call's T): on an engine of its own, calls of the three stages in turn with T going
    260 -> 3 -> 3 -> 5 -> 2 569 (the `chains` family, which holds the longest chain: 1 025 windows), a ring behind a ring and chains behind rings, each result equal to its checker array for array and counter
    for counter; the scaffold FASTA of the fourth call is written after the fifth.  No nxt, tail or carve offset is left over from the call
    before.  (Where every stage has buffers of its own the calls cannot meet: there the test passes trivially.)"""
    import merge_fuzz as MF
    import scaffold_cases as SQ
    import scaffold_checker as SC
    import scaffold_fuzz as SF
    import stitch_cases as TQ
    import stitch_checker as ST

    def same(got, want, arrays, what):
        for k in arrays:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)
        assert {k: v for k, v in got["info"].items() if not k.startswith("ms_")} == want["info"], (what, got["info"], want["info"])

    def scaffold(e, c, v):
        pl = e.place_reads(c["rows"], c["lens"], targets=(c["twords"], c["tbegin"], c["tlen"]), pair_off=c["pair_off"], **c["params"])
        return pl, e.scaffold(c["rows"], c["lens"], c["pair_off"], pl, **v)

    key = "rings/%d" % max(SF.RING_M)
    big, ring_sc, ring_mg, ring_st, chains = SF.case(key), SQ.case("ring3"), QC.case("ring3"), TQ.case("ring3"), MF.case("chains")
    assert len(big["tlen"]) == 260 and len(ring_mg["tlen"]) == len(ring_st["tlen"]) == 3 and len(ring_sc["tlen"]) < 260 < len(chains["tlen"])
    assert SF.checked(key)["info"]["joins_dropped_cycle"] == QC.checked("ring3")["info"]["joins_dropped_cycle"] == SQ.checked("ring3")["info"]["joins_dropped_cycle"] == 1
    assert max(MF.CHAIN_LENGTHS) == 1025 and MF.checked("chains")["info"]["merged_multi"] >= len(MF.CHAIN_LENGTHS)
    e = alga_amd.Engine(0)
    try:
        same(scaffold(e, big, big["variants"][0])[1].to_host(), SF.checked(key), SC.ARRAYS, "1: scaffold " + key)
        same(e.merge_ends(QC.targets(ring_mg), **ring_mg["variants"][0]).to_host(), QC.checked("ring3"), MC.ARRAYS, "2: merge ring3")
        same(e.stitch_targets(TQ.targets(ring_st), TQ.entries(ring_st), **ring_st["variants"][0]).to_host(), TQ.checked("ring3"), ST.ARRAYS, "3: stitch ring3")
        pl, sc = scaffold(e, ring_sc, ring_sc["variants"][0])
        same(sc.to_host(), SQ.checked("ring3"), SC.ARRAYS, "4: scaffold ring3")
        same(e.merge_ends(MF.targets(chains), **chains["variants"][0]).to_host(), MF.checked("chains"), MC.ARRAYS, "5: merge chains")
        path = str(tmp_path / "s.fasta")
        e.write_scaffold_fasta(path, pl, sc)
        assert open(path, "rb").read() == SC.fasta(SQ.checked("ring3"), ring_sc["seqs"])
    finally:
        e.close()


def test_a_wave_takes_a_second_end(eng):
    import torch
    waves = 8 * 4 * torch.cuda.get_device_properties(0).multi_processor_count  # k_mg_overlap: 8 blocks of 4 waves per CU
    c = QC.many_ends(waves // 2 + 300)                                           # two ends per target
    want = MC.merge_index(c["seqs"])
    mg = eng.merge_ends(QC.targets(c))
    assert_same(mg.to_host(), want, "many ends")
    print(mg.info)
    assert mg.info["ends"] > waves and mg.info["joins"] >= 4 and (want["partner"][2 * (waves // 2):] >= 0).any()


def test_a_second_round_on_the_merged_targets(eng, tmp_path):
    """path5 at max_overlap 55 joins what overlaps by 50 and leaves the overlap of 60 (its window lies off) to a second round at the default"""
    c = QC.case("path5")
    first = MC.merge_index(c["seqs"], max_overlap=55)
    assert first["info"]["joins"] == 3 and first["info"]["merged"] == 2
    mg = eng.merge_ends(QC.targets(c), max_overlap=55)
    assert_same(mg.to_host(), first, "round 1")
    c2 = QC.next_round(first)
    second = MC.merge_index(c2["seqs"])
    mg2 = eng.merge_ends(mg.targets())                                       # the input is the result before: it is read while the other set is written
    assert_same(mg2.to_host(), second, "round 2")
    assert second["info"]["joins"] == 1 and second["info"]["merged"] == 1
    s = MC.sequences(mg2.to_host())[0]
    assert (s == c["g"]).all() or (s == P.revcomp(c["g"])).all()
    eng.write_merged_fasta(str(tmp_path / "m.fasta"), mg2)
    assert open(str(tmp_path / "m.fasta"), "rb").read() == MC.fasta(second)


def test_the_callers_stream(eng):
    import torch
    c, want = QC.case("partial_word"), QC.checked("partial_word")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tg = device_targets(c)
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    mg = eng.merge_ends(tg, stream=s.cuda_stream)
    assert s.query()                                                             # the call returns with its work on the stream done
    assert_same(mg.to_host(), want, "on the caller's stream")
    assert_same(eng.merge_ends(tg).to_host(), want, "on the engine's stream afterwards")


def test_refusals_leave_an_earlier_result_valid(eng, tmp_path):
    c, want = QC.case("path5"), QC.checked("path5")
    mg = eng.merge_ends(QC.targets(c))
    assert_same(mg.to_host(), want, "before")
    neg = c["tlen"].copy()
    neg[3] = -1
    calls = [dict(tlen=neg), dict(k=7), dict(k=32), dict(max_mismatches=-1), dict(max_mismatches=255), dict(max_occ=0), dict(max_occ=65536), dict(min_overlap=20),
             dict(min_overlap=513), dict(max_overlap=41), dict(max_overlap=4097), dict(k=8, min_overlap=8, max_overlap=513), dict(flags=1)]
    for change in calls:
        tg = (c["twords"], c["tbegin"], change.get("tlen", c["tlen"]))
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.merge_ends(tg, **{k: v for k, v in change.items() if k != "tlen"})
        assert ei.value.code == -1, (list(change), ei.value)
        assert_same(mg.to_host(), want, ("after a refusal", list(change)))       # nothing written: the earlier result as it was
    with pytest.raises(TypeError):
        eng.merge_ends(QC.targets(c), min_anchor=1)
    # three lengths of 2^31 - 1: the column sum is above 2^32 - 2, refused after the check and before a base is read
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.merge_ends((c["twords"], np.zeros(3, np.int64), np.full(3, 2 ** 31 - 1, np.int32)))
    assert ei.value.code == -5, ei.value                                         # ALGA_ERR_CAPACITY
    assert_same(mg.to_host(), want, "after the capacity refusal")
    path = str(tmp_path / "m.fasta")
    eng.write_merged_fasta(path, mg)
    assert open(path, "rb").read() == MC.fasta(want)
    again = eng.merge_ends(QC.targets(c))
    assert_same(again.to_host(), want, "the engine afterwards")
    with pytest.raises(alga_amd.AlgaError):
        eng.write_merged_fasta(path, mg)                                         # `mg` is the result before the last one
    eng.write_merged_fasta(path, again)
    assert open(path, "rb").read() == MC.fasta(want)


def test_a_result_stays_valid_across_the_other_stages(eng, tmp_path):
    import break_cases as BQ
    c, want = QC.case("pairings"), QC.checked("pairings")
    other, g = BQ.case("inset"), GQ.case("tiny_targets")
    mg = eng.merge_ends(QC.targets(c))
    pl2 = eng.place_reads(other["rows"], other["lens"], targets=(other["twords"], other["tbegin"], other["tlen"]), pair_off=other["pair_off"])
    eng.polish(other["rows"], other["lens"], pl2)
    eng.break_contigs(other["rows"], other["lens"], other["pair_off"], pl2, **other["variants"][0])
    eng.scaffold(other["rows"], other["lens"], other["pair_off"], pl2)
    pl3 = eng.place_reads(g["rows"], g["lens"], targets=(g["twords"], g["tbegin"], g["tlen"]))
    eng.grow_ends(g["rows"], g["lens"], pl3, **g["variants"][0])
    assert_same(mg.to_host(), want, "after a later placement, polish, break, scaffold and grow")
    path = str(tmp_path / "m.fasta")
    eng.write_merged_fasta(path, mg)                                             # the bases are the result's own copy
    assert open(path, "rb").read() == MC.fasta(want)
    # the merged contigs as the targets of a placement: reads over the joins are placed
    seqs = MC.sequences(want)
    reads = [s[a:a + 60] for s in seqs if len(s) > 150 for a in (0, len(s) // 2 - 30, len(s) - 60)]
    rows, lens = P.nodes_of(reads)
    got = eng.place_reads(rows, lens, targets=mg.targets()).to_host()
    want_pl = P.place(rows, lens, None, want["words"], want["begin"].astype(np.int64), want["len"])
    for k in P.ARRAYS:
        assert (got[k] == want_pl[k]).all(), k
    assert want_pl["info"]["placed"] == len(reads) == 12


def test_planted_genome_end_to_end(eng):
    """three rounds of place -> grow on the device, then the merge: one contig, the genome's window 11 .. 2992, one join of 58 bases without a
    mismatch; the reads are then placed on it"""
    c, g, meta = GQ.planted()
    tg = (c["twords"], c["tbegin"], c["tlen"])
    for rnd in range(3):
        pl = eng.place_reads(c["rows"], c["lens"], targets=tg)
        gw = eng.grow_ends(c["rows"], c["lens"], pl)
        tg = gw.targets()
    seqs = GC.sequences(gw.to_host())
    assert (seqs[0] == g[11:1292]).all() and (seqs[1] == g[1234:2992]).all()
    mg = eng.merge_ends(tg)
    got = mg.to_host()
    assert_same(got, MC.merge_index(seqs), "planted")
    i = mg.info
    assert (i["joins"], i["bases_removed"], i["join_mismatches"], i["merged"], i["longest"]) == (1, 58, 0, 1, 2981)
    assert (MC.sequences(got)[0] == g[11:2992]).all()
    pl = eng.place_reads(c["rows"], c["lens"], targets=mg.targets())
    assert pl.n_targets == 1 and pl.info["placed"] > gw._placements.info["placed"]
    print(i, pl.info)


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, c in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in c)))


def codes(s):
    return np.array(["ACGT".index(x) for x in s], dtype=np.uint8)


def test_command_line(eng, tmp_path):
    """paired reads of a 6 kb genome in which no read ends more than 27 bases behind position 3000 or begins more than 27 before it: two reads
    overlap there by 54 at the most, below the graph's minimum of 55, so two contigs come out whose ends overlap.  alga_hip with --grow_ends=1
    --merge_ends=1 --merged= --merge_layout=: the files against the Python API doing the same on the contigs the run writes, and against the
    checker; a run with --merge_ends=0 writes what a run without the option writes"""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    rng = np.random.default_rng(94)
    g = rng.integers(0, 4, size=6000, dtype=np.uint8)
    X, D = 3000, 27
    ok = lambda s: s + 100 <= X + D or s >= X - D
    m1, m2 = [], []
    for a in rng.permutation(np.arange(0, 6000 - 400, 2)):
        a, ins = int(a), int(rng.integers(300, 401))
        if ok(a) and ok(a + ins - 100):
            m1.append(g[a:a + 100])
            m2.append(P.revcomp(g[a + ins - 100:a + ins]))
    for ins in range(300, 400, 10):                                              # reads that reach exactly that far, from both sides
        m1.append(g[X + D - ins:X + D - ins + 100])
        m2.append(P.revcomp(g[X + D - 100:X + D]))
        m1.append(g[X - D:X - D + 100])
        m2.append(P.revcomp(g[X - D + ins - 100:X - D + ins]))
    _write_fasta(str(tmp_path / "a.fasta"), m1)
    _write_fasta(str(tmp_path / "b.fasta"), m2)
    base = [exe, "--file1=a.fasta", "--file2=b.fasta", "--output=o.fasta", "--contigs_min_length=150", "--consensus_min_votes=0", "--retl=0", "--retr=0", "--grow_ends=1"]
    run = lambda args: subprocess.run(args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    r0 = run(base + ["--contigs_final=f0.fasta", "--scaffolds=s0.fasta", "--scaffold_layout=l0.tsv", "--grown=g0.fasta"])
    assert r0.returncode == 0, r0.stderr[-2000:]
    r1 = run(base + ["--contigs_final=f1.fasta", "--scaffolds=s1.fasta", "--scaffold_layout=l1.tsv", "--grown=g1.fasta", "--merge_ends=0"])
    assert r1.returncode == 0 and "Contig ends merged" not in r0.stderr + r1.stderr, r1.stderr[-2000:]
    for a, b in (("f0.fasta", "f1.fasta"), ("s0.fasta", "s1.fasta"), ("l0.tsv", "l1.tsv"), ("g0.fasta", "g1.fasta")):
        assert open(str(tmp_path / a), "rb").read() == open(str(tmp_path / b), "rb").read(), a
    r = run(base + ["--contigs_final=f.fasta", "--scaffolds=s.fasta", "--scaffold_layout=l.tsv", "--grown=g.fasta", "--merge_ends=1", "--merged=m.fasta", "--merge_layout=m.tsv",
                   "--merge_min_overlap=30"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Contig ends merged:" in r.stderr and "Reads placed on the merged contigs" in r.stderr, r.stderr[-2000:]
    for a, b in (("f.fasta", "f0.fasta"), ("g.fasta", "g0.fasta")):              # the final and the grown contigs are what they were
        assert open(str(tmp_path / a), "rb").read() == open(str(tmp_path / b), "rb").read(), a
    for bad in (["--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--merge_ends=1"],
                ["--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--grow_ends=1", "--merged=m2.fasta"],
                ["--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--grow_ends=1", "--merge_layout=m2.tsv"],
                ["--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--grow_ends=1", "--merge_ends=2"],
                ["--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--grow_ends=1", "--merge_ends=1", "--merge_min_overlap=20"],
                ["--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--grow_ends=1", "--merge_ends=1", "--merge_max_mismatches=255"]):
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
    # the Python API and the checker on the same contigs, the same steps
    pl = eng.place_reads(rows, lens, targets=(tw, tb, tl), pair_off=pair_off)
    gw = eng.grow_ends(rows, lens, pl)
    grown = GC.sequences(GC.grow_index(rows, lens, P.place(rows, lens, pair_off, tw, tb, tl), tg))
    mg = eng.merge_ends(gw.targets(), min_overlap=30)
    want = MC.merge_index(grown, min_overlap=30)
    got = mg.to_host()
    assert_same(got, want, "the command line's contigs")
    i = mg.info
    said = "Contig ends merged: %d ends with an overlap, %d ambiguous, %d joins, %d bases removed, N50 %d -> %d;" % (
        i["ends_with_overlap"], i["ends_ambiguous"], i["joins"], i["bases_removed"], i["n50_before"], i["n50_after"])
    print(said, r.stderr[-1500:])
    assert said in r.stderr, r.stderr[-3000:]
    assert i["joins"] >= 1 and i["n50_after"] > i["n50_before"]
    s = MC.sequences(got)[int(np.argmax(got["len"]))]
    where = lambda s: "".join("ACGT"[x] for x in g).find("".join("ACGT"[x] for x in s))
    assert where(s) >= 0 or where(P.revcomp(s)) >= 0                            # the merged contig runs through position 3000: a window of the genome
    assert len(s) > 5000
    eng.write_merged_fasta(str(tmp_path / "api.fasta"), mg)
    assert open(str(tmp_path / "m.fasta"), "rb").read() == open(str(tmp_path / "api.fasta"), "rb").read() == MC.fasta(want)
    tlen = [len(x) for x in grown]
    assert open(str(tmp_path / "m.tsv"), "rb").read() == mg.merge_tsv(tlen, got).encode() == MC.merge_tsv(want, tlen)
    pl = eng.place_reads(rows, lens, targets=mg.targets(), pair_off=pair_off)
    sc = eng.scaffold(rows, lens, pair_off, pl)
    eng.write_scaffold_fasta(str(tmp_path / "api_s.fasta"), pl, sc)
    assert open(str(tmp_path / "s.fasta"), "rb").read() == open(str(tmp_path / "api_s.fasta"), "rb").read()
    assert open(str(tmp_path / "l.tsv"), "rb").read() == sc.layout_tsv().encode()
