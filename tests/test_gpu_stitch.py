"""The stitch stage on the GPU (alga_stitch_targets_device, alga_stitch_scaffolds_device, alga_write_stitched_fasta_device): every output array
and every counter equal to the Python definition (tests/stitch_checker.py) on the cases of tests/stitch_cases.py, from host arrays and from
tensors; the FASTA bytes and the TSV; grids that stride and a wave of k_st_overlap that takes further entries; refusals leave an earlier result
valid; the caller's stream; a second round on Stitched.targets(); a result stays valid across the other stages; the merge stage's results in
and out; the planted genome end to end through place -> scaffold -> stitch -> place -> scaffold, with a polish between; the command line.

Measured on an MI355X: the whole file, 31 tests, in 5.7 s; the slowest are the command line (2.0 s: three runs of alga_hip and seven refused
ones) and the first case (1.6 s of set-up: it creates the engine); every other test takes under 0.4 s, most of it the checker's."""
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import merge_cases as MQ
import merge_checker as MC
import place_cases as PC
import place_checker as P
import polish_checker as Q
import scaffold_checker as SC
import stitch_cases as SQ
import stitch_checker as ST

pytestmark = pytest.mark.gpu
TIMES = ("ms_overlap", "ms_build", "ms_total")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what=""):
    for k in ST.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert (got[k] == want[k]).all(), (what, k, np.nonzero(got[k] != want[k])[0][:10])
    info = {k: v for k, v in got["info"].items() if k not in TIMES}
    assert info == want["info"], (what, info, want["info"])


def device_inputs(c):
    import torch
    tg = (torch.from_numpy(c["twords"].view(np.int32)).cuda(), torch.from_numpy(c["tbegin"]).cuda(), torch.from_numpy(c["tlen"]).cuda())
    a, b, gap, state = c["entries"]
    en = (torch.from_numpy(a.view(np.int32)).cuda(), torch.from_numpy(b.view(np.int32)).cuda(), torch.from_numpy(gap).cuda())
    return tg, en if state is None else en + (torch.from_numpy(state).cuda(),)


@pytest.mark.parametrize("name", sorted(SQ.CASES))
def test_every_case_equals_the_checker(eng, name, tmp_path):
    c = SQ.case(name)
    path = str(tmp_path / "s.fasta")
    for i, v in enumerate(c["variants"]):
        want = SQ.checked(name, i)
        st = eng.stitch_targets(SQ.targets(c), SQ.entries(c), **v)
        got = st.to_host()
        assert_same(got, want, (name, i, "host arrays"))
        assert (st.n_targets, st.n_entries, st.n_stitched, st.n_members, st.n_columns) == (len(c["tlen"]), len(c["entries"][0]), len(want["len"]), len(want["s_members"]),
                                                                                            int(want["col_off"][-1]))
        info = eng.write_stitched_fasta(path, st)
        text = open(path, "rb").read()
        assert text == ST.fasta(want), (name, i)
        assert info["segments"] == len(want["len"]) and info["bytes"] == len(text)
        assert st.stitch_tsv().encode() == st.stitch_tsv(c["tlen"], got).encode() == ST.stitch_tsv(want, c["tlen"]), (name, i)
        print(name, i, st.info)
    # from tensors: they are used where they are and left untouched
    tg, en = device_inputs(c)
    keep = [x.clone() for x in tg + en]
    for i, v in enumerate(c["variants"]):
        assert_same(eng.stitch_targets(tg, en, **v).to_host(), SQ.checked(name, i), (name, i, "tensors"))
    for x, y in zip(tg + en, keep):
        assert (x == y).all()


def test_what_the_merge_stage_refuses(eng):
    """an overlap of 20 and an end with two partners: Engine.merge_ends on the same targets joins nothing, the stitch joins the entry's two ends"""
    for name, state in (("short", 0), ("two_partners", MC.HAS_OVERLAP | MC.AMBIGUOUS)):
        c = SQ.case(name)
        mg = eng.merge_ends(SQ.targets(c))
        assert mg.info["joins"] == 0 and mg.n_merged == len(c["tlen"]) and int(mg.end_state[1]) == state, (name, mg.info)
        st = eng.stitch_targets(SQ.targets(c), SQ.entries(c))
        assert st.info["stitched"] == 1 and st.n_stitched == len(c["tlen"]) - 1, (name, st.info)
        assert_same(st.to_host(), SQ.checked(name), name)


def test_grids_stride_and_a_wave_takes_further_entries(eng):
    """about 3000 entries with stitch_max_blocks 1 and 2: one and two blocks of four waves work through all of them, every other grid strides too;
    the cap set back to its default gives the same result"""
    c = SQ.many(3001)
    want = ST.stitch_windows(c["seqs"], c["entries"])
    i = want["info"]
    assert i["entries"] == 3001 and i["selected"] == 2401 and i["stitched"] > 1500 and i["join_mismatches"] > 300 and i["contigs_multi"] == i["stitched"]
    try:
        for cap in (1, 2):
            eng.set_option("stitch_max_blocks", cap)
            assert_same(eng.stitch_targets(SQ.targets(c), SQ.entries(c)).to_host(), want, ("many entries", cap))
    finally:
        eng.set_option("stitch_max_blocks", 8192)
    st = eng.stitch_targets(SQ.targets(c), SQ.entries(c))
    assert_same(st.to_host(), want, "many entries, the default cap")
    print("many entries", st.info)
    for bad in (0, 8193):
        with pytest.raises(alga_amd.AlgaError):
            eng.set_option("stitch_max_blocks", bad)


def test_refusals_leave_an_earlier_result_valid(eng, tmp_path):
    c, want = SQ.case("path5"), SQ.checked("path5")
    st = eng.stitch_targets(SQ.targets(c), SQ.entries(c))
    assert_same(st.to_host(), want, "before")
    T = len(c["tlen"])
    a, b, gap, state = c["entries"]
    neg = c["tlen"].copy()
    neg[3] = -1

    def with_entry(x, y, s=3):
        return (np.append(a, np.uint32(x)), np.append(b, np.uint32(y)), np.append(gap, np.int32(0)), np.append(state, np.uint8(s)))
    calls = [dict(tlen=neg), dict(max_mismatches=-1), dict(max_mismatches=255), dict(min_overlap=7), dict(min_overlap=513), dict(max_overlap=15), dict(max_overlap=4097),
             dict(slack=-1), dict(slack=2 ** 20 + 1), dict(flags=1), dict(entries=with_entry(2 * T, 7)), dict(entries=with_entry(7, 2 * T)), dict(entries=with_entry(7, 0xFFFFFFFF)),
             dict(entries=with_entry(2, 3)), dict(entries=with_entry(7, 7)), dict(entries=with_entry(7, int(a[0]))), dict(entries=with_entry(int(b[1]), 2))]
    for change in calls:
        tg = (c["twords"], c["tbegin"], change.get("tlen", c["tlen"]))
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.stitch_targets(tg, change.get("entries", SQ.entries(c)), **{k: v for k, v in change.items() if k not in ("tlen", "entries")})
        assert ei.value.code == -1, (list(change), ei.value)
        assert_same(st.to_host(), want, ("after a refusal", list(change)))       # nothing written: the earlier result as it was
    # the same malformed entries unselected: ignored
    assert_same_but_entries(eng.stitch_targets(SQ.targets(c), with_entry(2 * T, 7, 1)).to_host(), want)
    st = eng.stitch_targets(SQ.targets(c), SQ.entries(c))
    with pytest.raises(TypeError):
        eng.stitch_targets(SQ.targets(c), SQ.entries(c), k=21)
    # three lengths of 2^31 - 1: the column sum is above 2^32 - 2, refused after the check and before a base is read
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.stitch_targets((c["twords"], np.zeros(3, np.int64), np.full(3, 2 ** 31 - 1, np.int32)), ST.entries_of())
    assert ei.value.code == -5, ei.value                                         # ALGA_ERR_CAPACITY
    assert_same(st.to_host(), want, "after the capacity refusal")
    path = str(tmp_path / "s.fasta")
    eng.write_stitched_fasta(path, st)
    assert open(path, "rb").read() == ST.fasta(want)
    again = eng.stitch_targets(SQ.targets(c), SQ.entries(c))
    assert_same(again.to_host(), want, "the engine afterwards")
    with pytest.raises(alga_amd.AlgaError):
        eng.write_stitched_fasta(path, st)                                       # `st` is the result before the last one
    eng.write_stitched_fasta(path, again)
    assert open(path, "rb").read() == ST.fasta(want)


def assert_same_but_entries(got, want):
    """the result of a call with one further, unselected entry"""
    for k in ST.ARRAYS:
        if k.startswith("j_"):
            assert (got[k][:-1] == want[k]).all() and got[k][-1] == 0, k
        else:
            assert (got[k] == want[k]).all(), k
    assert got["info"]["entries"] == want["info"]["entries"] + 1 and got["info"]["selected"] == want["info"]["selected"]


def test_the_callers_stream(eng):
    import torch
    c, want = SQ.case("partial_word"), SQ.checked("partial_word")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tg, en = device_inputs(c)
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    st = eng.stitch_targets(tg, en, stream=s.cuda_stream)
    assert s.query()                                                             # the call returns with its work on the stream done
    assert_same(st.to_host(), want, "on the caller's stream")
    assert_same(eng.stitch_targets(tg, en).to_host(), want, "on the engine's stream afterwards")


def test_a_second_round_on_the_stitched_targets(eng):
    """path5 at max_overlap 55 stitches what overlaps by 50 and leaves the overlap of 60 (its window lies off) to a second round, whose targets are
    the first round's result: it is read while the other set is written"""
    c = SQ.case("path5")
    first = ST.stitch_windows(c["seqs"], c["entries"], max_overlap=55)
    assert first["info"]["stitched"] == 3 and first["info"]["contigs"] == 2 and first["s_members"].tolist() == [0, 2, 4, 1, 3] and first["len"].tolist() == [800, 260]
    st = eng.stitch_targets(SQ.targets(c), SQ.entries(c), max_overlap=55)
    assert_same(st.to_host(), first, "round 1")
    # stitched 0 is the path 0, 2, 4, 1, entered at contig 0's left end, where the overlap of 60 with the left end of contig 3 (stitched 1) lies
    seqs = ST.sequences(first)
    entry = ST.entries_of([0], [2], [-60])
    second = ST.stitch_windows(seqs, entry)
    st2 = eng.stitch_targets(st.targets(), SQ.entries(dict(entries=entry)))
    assert_same(st2.to_host(), second, "round 2")
    assert second["info"]["stitched"] == 1 and second["info"]["contigs"] == 1
    s = ST.sequences(st2.to_host())[0]
    assert (s == c["g"]).all() or (s == P.revcomp(c["g"])).all()


def test_a_result_stays_valid_across_the_other_stages(eng, tmp_path):
    import break_cases as BQ
    import grow_cases as GQ
    c, want = SQ.case("pairings"), SQ.checked("pairings")
    other, g, m = BQ.case("inset"), GQ.case("tiny_targets"), MQ.case("pairings")
    st = eng.stitch_targets(SQ.targets(c), SQ.entries(c))
    pl2 = eng.place_reads(other["rows"], other["lens"], targets=(other["twords"], other["tbegin"], other["tlen"]), pair_off=other["pair_off"])
    eng.polish(other["rows"], other["lens"], pl2)
    eng.break_contigs(other["rows"], other["lens"], other["pair_off"], pl2, **other["variants"][0])
    eng.scaffold(other["rows"], other["lens"], other["pair_off"], pl2)
    pl3 = eng.place_reads(g["rows"], g["lens"], targets=(g["twords"], g["tbegin"], g["tlen"]))
    eng.grow_ends(g["rows"], g["lens"], pl3, **g["variants"][0])
    eng.merge_ends(MQ.targets(m))
    assert_same(st.to_host(), want, "after a later placement, polish, break, scaffold, grow and merge")
    path = str(tmp_path / "s.fasta")
    eng.write_stitched_fasta(path, st)                                           # the bases are the result's own copy
    assert open(path, "rb").read() == ST.fasta(want)


def test_the_merge_stage_in_front_and_behind(eng):
    """Merged.targets() in and Engine.merge_ends(Stitched.targets()) out: the two stages' buffers do not collide"""
    m = MQ.case("path5")                                                         # merged at max_overlap 55: two contigs that overlap by 60
    first = MC.merge_index(m["seqs"], max_overlap=55)
    mg = eng.merge_ends(MQ.targets(m), max_overlap=55)
    seqs = MC.sequences(first)
    assert [len(s) for s in seqs] == [800, 260]
    entry = ST.entries_of([0], [2], [-60])
    want = ST.stitch_windows(seqs, entry)
    st = eng.stitch_targets(mg.targets(), entry[:3])
    assert_same(st.to_host(), want, "on the merged contigs")
    s = ST.sequences(want)[0]
    assert want["info"]["stitched"] == 1 and ((s == m["g"]).all() or (s == P.revcomp(m["g"])).all())
    assert (mg.to_host()["words"] == first["words"]).all()                       # the merge result as it was
    c = SQ.case("mismatches")                                                    # overlaps of 50: the merge stage joins those with at most one mismatch
    st = eng.stitch_targets(SQ.targets(c), SQ.entries(c), max_mismatches=0)
    want = SQ.checked("mismatches", 1)
    mg2 = eng.merge_ends(st.targets())
    want_mg = MC.merge_index(ST.sequences(want))
    for k in MC.ARRAYS:
        assert (mg2.to_host()[k] == want_mg[k]).all(), k
    assert want_mg["info"]["joins"] == 2 and mg2.info["joins"] == 2
    assert_same(st.to_host(), want, "after the merge of its targets")


def _place(eng, c, tg):
    return eng.place_reads(c["rows"], c["lens"], targets=tg, pair_off=c["pair_off"])


def test_planted_genome_end_to_end(eng, tmp_path):
    """three contigs that overlap by 30 and 25, pairs laid over them: place -> scaffold writes two runs of N; Engine.stitch equals stitch_targets on
    the bundles and the checker fed with the scaffold checker's bundles; place on the stitched contig -> scaffold: no N, the planted sequence"""
    c, g = SQ.planted()
    tg = SQ.targets(c)
    pl = _place(eng, c, tg)
    sc = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl)
    want_pl = P.place(*PC.args(c))
    want_sc = SC.scaffold_dicts(c["rows"], c["lens"], c["pair_off"], want_pl, insert=want_pl["info"]["insert_median"])
    assert sc.info["joins"] == 2 and (sc.to_host()["b_gap"] == want_sc["b_gap"]).all()
    before = str(tmp_path / "before.fasta")
    eng.write_scaffold_fasta(before, pl, sc)
    n_before = open(before).read().count("N")
    assert n_before == 20                                                        # two joins with a negative gap estimate: min_gap Ns each
    entries = ST.entries_of(want_sc["b_a"], want_sc["b_b"], want_sc["b_gap"], want_sc["b_state"])
    want = ST.stitch_windows(c["seqs"], entries)
    st = eng.stitch(pl, sc)
    got = st.to_host()
    assert_same(got, want, "Engine.stitch")
    assert st.stitch_tsv().encode() == ST.stitch_tsv(want, c["tlen"])
    i = st.info
    assert (i["stitched"], i["bases_removed"], i["join_mismatches"], i["contigs"], i["longest"]) == (2, 55, 0, 1, 4000) and sorted(got["j_olen"][got["j_hits"] == 1]) == [25, 30]
    s = ST.sequences(got)[0]
    assert (s == g).all() or (s == P.revcomp(g)).all()
    by_hand = eng.stitch_targets(tg, (sc.b_a, sc.b_b, sc.b_gap, sc.b_state))
    assert_same(by_hand.to_host(), want, "stitch_targets on the bundles")
    # a placement that is not current, a stale scaffold result
    st = eng.stitch(pl, sc)
    pl2 = _place(eng, c, st.targets())
    for args in ((pl, sc), (pl2, sc)):
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.stitch(*args)
        assert ei.value.code == -1
    assert_same(st.to_host(), want, "after the refusals")
    # the reads on the stitched contig: one scaffold, no N
    sc2 = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl2)
    after = str(tmp_path / "after.fasta")
    eng.write_scaffold_fasta(after, pl2, sc2)
    text = open(after).read().split("\n")
    assert sc2.n_scaffolds == 1 and "N" not in text[1] and text[1] in ("".join("ACGT"[x] for x in g), "".join("ACGT"[x] for x in P.revcomp(g)))
    assert pl2.info["placed"] > pl.info["placed"]                                # the reads over the cuts lie now
    assert eng.stitch(pl2, sc2).info["selected"] == 0
    print(i, pl.info["placed"], pl2.info["placed"])


def test_planted_genome_with_a_polish_between(eng):
    """base 500 of every contig is wrong; with polished= the stitched bases are the polished ones"""
    c, g = SQ.planted(dirty=True)
    tg = SQ.targets(c)
    pl = _place(eng, c, tg)
    pol = eng.polish(c["rows"], c["lens"], pl)
    sc = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl)
    want_pl = P.place(*PC.args(c))
    want_pol = Q.polish_scatter(c["rows"], c["lens"], want_pl, *tg)
    want_sc = SC.scaffold_dicts(c["rows"], c["lens"], c["pair_off"], want_pl, insert=want_pl["info"]["insert_median"])
    entries = ST.entries_of(want_sc["b_a"], want_sc["b_b"], want_sc["b_gap"], want_sc["b_state"])
    plain, polished = ST.stitch_windows(c["seqs"], entries), ST.stitch_windows(Q.sequences(want_pol), entries)
    assert_same(eng.stitch(pl, sc).to_host(), plain, "the placement's bases")
    st = eng.stitch(pl, sc, polished=pol)
    assert_same(st.to_host(), polished, "the polished bases")
    s, p = ST.sequences(polished)[0], ST.sequences(plain)[0]
    assert ((s == g).all() or (s == P.revcomp(g)).all()) and int((s != p).sum()) == 3
    pl2 = _place(eng, c, tg)
    sc2 = eng.scaffold(c["rows"], c["lens"], c["pair_off"], pl2)
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.stitch(pl2, sc2, polished=pol)                                       # the polish at hand is of the earlier placement
    assert ei.value.code == -1
    assert_same(st.to_host(), polished, "after the refusal")


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, c in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in c)))


def codes(s):
    return np.array(["ACGT".index(x) for x in s], dtype=np.uint8)


def test_command_line(eng, tmp_path):
    """the reads of test_gpu_merge's command line: two contigs whose ends overlap by less than the graph's minimum of 55.  alga_hip with
    --scaffolds= --stitch=1 --stitched= --stitch_layout=: the files against the Python API doing the same on the contigs the run writes, and
    against the checker; a run with --stitch=0 writes what a run without the option writes; the flag errors"""
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
    base = [exe, "--file1=a.fasta", "--file2=b.fasta", "--output=o.fasta", "--contigs_min_length=150", "--consensus_min_votes=0", "--retl=0", "--retr=0"]
    run = lambda args: subprocess.run(args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    r0 = run(base + ["--contigs_final=f0.fasta", "--scaffolds=s0.fasta", "--scaffold_layout=l0.tsv"])
    assert r0.returncode == 0, r0.stderr[-2000:]
    r1 = run(base + ["--contigs_final=f1.fasta", "--scaffolds=s1.fasta", "--scaffold_layout=l1.tsv", "--stitch=0"])
    assert r1.returncode == 0 and "stitched" not in r0.stderr + r1.stderr, r1.stderr[-2000:]
    for a, b in (("f0.fasta", "f1.fasta"), ("s0.fasta", "s1.fasta"), ("l0.tsv", "l1.tsv")):
        assert open(str(tmp_path / a), "rb").read() == open(str(tmp_path / b), "rb").read(), a
    r = run(base + ["--contigs_final=f.fasta", "--scaffolds=s.fasta", "--scaffold_layout=l.tsv", "--stitch=1", "--stitched=st.fasta", "--stitch_layout=st.tsv"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Scaffold joins stitched:" in r.stderr and "Reads placed on the stitched contigs" in r.stderr, r.stderr[-2000:]
    assert open(str(tmp_path / "f.fasta"), "rb").read() == open(str(tmp_path / "f0.fasta"), "rb").read()      # the final contigs are what they were
    for bad in (["--file1=a.fasta", "--file2=b.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--stitch=1"],
                ["--file1=a.fasta", "--file2=b.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--scaffolds=s2.fasta", "--stitched=st2.fasta"],
                ["--file1=a.fasta", "--file2=b.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--scaffolds=s2.fasta", "--stitch_layout=st2.tsv"],
                ["--file1=a.fasta", "--file2=b.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--scaffolds=s2.fasta", "--stitch=2"],
                ["--file1=a.fasta", "--file2=b.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--scaffolds=s2.fasta", "--stitch=1", "--stitch_min_overlap=7"],
                ["--file1=a.fasta", "--file2=b.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--scaffolds=s2.fasta", "--stitch=1", "--stitch_max_mismatches=255"],
                ["--file1=a.fasta", "--file2=b.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--scaffolds=s2.fasta", "--stitch=1", "--stitch_slack=-1"]):
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
    sc = eng.scaffold(rows, lens, pair_off, pl)
    h = sc.to_host()
    want = ST.stitch_windows(tg, ST.entries_of(h["b_a"], h["b_b"], h["b_gap"], h["b_state"]))
    st = eng.stitch(pl, sc)
    got = st.to_host()
    assert_same(got, want, "the command line's contigs")
    i = st.info
    said = "Scaffold joins stitched: %d selected, %d with an overlap, %d ambiguous, %d stitched, %d bases removed, N50 %d -> %d;" % (
        i["selected"], i["with_overlap"], i["ambiguous"], i["stitched"], i["bases_removed"], i["n50_before"], i["n50_after"])
    print(said, r.stderr[-1500:])
    assert said in r.stderr, r.stderr[-3000:]
    assert i["stitched"] >= 1 and i["n50_after"] > i["n50_before"]
    s = ST.sequences(got)[int(np.argmax(got["len"]))]
    where = lambda s: "".join("ACGT"[x] for x in g).find("".join("ACGT"[x] for x in s))
    assert where(s) >= 0 or where(P.revcomp(s)) >= 0                            # the stitched contig runs through position 3000: a window of the genome
    assert len(s) > 5000
    eng.write_stitched_fasta(str(tmp_path / "api.fasta"), st)
    assert open(str(tmp_path / "st.fasta"), "rb").read() == open(str(tmp_path / "api.fasta"), "rb").read() == ST.fasta(want)
    tlen = [len(x) for x in tg]
    assert open(str(tmp_path / "st.tsv"), "rb").read() == st.stitch_tsv(tlen, got).encode() == ST.stitch_tsv(want, tlen)
    pl2 = eng.place_reads(rows, lens, targets=st.targets(), pair_off=pair_off)
    sc2 = eng.scaffold(rows, lens, pair_off, pl2)
    eng.write_scaffold_fasta(str(tmp_path / "api_s.fasta"), pl2, sc2)
    assert open(str(tmp_path / "s.fasta"), "rb").read() == open(str(tmp_path / "api_s.fasta"), "rb").read()
    assert open(str(tmp_path / "l.tsv"), "rb").read() == sc2.layout_tsv().encode()
    assert open(str(tmp_path / "s.fasta")).read().count("N") < open(str(tmp_path / "s0.fasta")).read().count("N")
