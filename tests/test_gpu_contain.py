"""The containment stage on the GPU (alga_drop_contained_device, alga_write_kept_fasta_device): every output array and every counter equal to
the Python definition (tests/contain_checker.py) on the cases of tests/contain_cases.py, from host arrays with directories of 1 bit and auto and
from tensors; the FASTA bytes and the TSV; every case again with contain_max_blocks 1 and 3; a wave of k_ct_contain that takes a second (c, s); a
second call on Kept.targets(); the caller's stream; the index workspace shared with the placement; refusals leave an earlier result valid; a
result stays valid across a later placement and merge; the planted genome with two planted extras; the command line."""
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import contain_cases as QC
import contain_checker as CC
import grow_cases as GQ
import grow_checker as GC
import place_cases as PC
import place_checker as P

pytestmark = pytest.mark.gpu
TIMES = ("ms_index", "ms_contain", "ms_build", "ms_total")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what=""):
    for k in CC.ARRAYS:
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
    path = str(tmp_path / "k.fasta")
    for i, v in enumerate(c["variants"]):
        want = QC.checked(name, i)
        for bits in (1, 0):
            eng.set_option("place_dir_bits", bits)
            kp = eng.drop_contained(QC.targets(c), **v)
            assert_same(kp.to_host(), want, (name, i, "host arrays", bits))
        got = kp.to_host()
        assert (kp.n_targets, kp.n_kept, kp.n_columns) == (len(c["tlen"]), len(want["len"]), int(want["col_off"][-1]))
        info = eng.write_kept_fasta(path, kp)
        text = open(path, "rb").read()
        assert text == CC.fasta(want), (name, i)
        assert info["segments"] == len(want["len"]) and info["bytes"] == len(text)
        assert kp.contain_tsv().encode() == kp.contain_tsv(c["tlen"], got).encode() == CC.contain_tsv(want, c["tlen"]), (name, i)
        print(name, i, kp.info)
    # from tensors: they are used where they are and left untouched
    tg = device_targets(c)
    keep = [x.clone() for x in tg]
    for i, v in enumerate(c["variants"]):
        assert_same(eng.drop_contained(tg, **v).to_host(), QC.checked(name, i), (name, i, "tensors"))
    for a, b in zip(tg, keep):
        assert (a == b).all()


@pytest.mark.parametrize("blocks", [1, 3])
def test_every_case_with_capped_grids(eng, blocks):
    """contain_max_blocks 1 and 3: every grid-stride loop takes further passes, the results are identical"""
    try:
        eng.set_option("contain_max_blocks", blocks)
        for name, i in QC.every():
            c = QC.case(name)
            assert_same(eng.drop_contained(QC.targets(c), **c["variants"][i]).to_host(), QC.checked(name, i), (name, i, blocks))
    finally:
        eng.set_option("contain_max_blocks", 8192)
    for bad in (0, 8193):
        with pytest.raises(alga_amd.AlgaError):
            eng.set_option("contain_max_blocks", bad)


def test_a_wave_takes_a_second_query(eng):
    import torch
    waves = 8 * 4 * torch.cuda.get_device_properties(0).multi_processor_count  # k_ct_contain: 8 blocks of 4 waves per CU
    c = QC.many_queries(waves // 2 + 300)                                        # two queries per target
    want = CC.contain_index(c["seqs"])
    kp = eng.drop_contained(QC.targets(c))
    assert_same(kp.to_host(), want, "many queries")
    print(kp.info)
    assert 2 * kp.info["queries"] > waves and kp.info["contained"] >= 4 and (want["host"][waves // 2:] >= 0).any()


def test_a_second_call_on_the_kept_targets(eng, tmp_path):
    """the input is the result before: it is read while the other set is written.  Nothing is contained any more, the bases are the same"""
    c, first = QC.case("chain"), QC.checked("chain")
    kp = eng.drop_contained(QC.targets(c))
    assert_same(kp.to_host(), first, "call 1")
    c2 = QC.next_round(first)
    second = CC.contain_index(c2["seqs"])
    kp2 = eng.drop_contained(kp.targets())
    got = kp2.to_host()
    assert_same(got, second, "call 2")
    assert second["info"]["contained"] == 0 and second["info"]["kept"] == first["info"]["kept"] == len(QC.CHAIN_DEPTHS)
    assert (got["words"] == first["words"]).all() and (got["len"] == first["len"]).all()
    eng.write_kept_fasta(str(tmp_path / "k.fasta"), kp2)
    assert open(str(tmp_path / "k.fasta"), "rb").read() == CC.fasta(second)


def test_the_callers_stream(eng):
    import torch
    c, want = QC.case("word_edges"), QC.checked("word_edges")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tg = device_targets(c)
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    kp = eng.drop_contained(tg, stream=s.cuda_stream)
    assert s.query()                                                             # the call returns with its work on the stream done
    assert_same(kp.to_host(), want, "on the caller's stream")
    assert_same(eng.drop_contained(tg).to_host(), want, "on the engine's stream afterwards")


def test_one_index_workspace_serves_the_stages_in_turn(eng):
    """the placement and this stage build their seed index in one workspace of the engine: a placement with another index (another k, another
    directory width) between two calls leaves nothing behind"""
    def place(c):
        return eng.place_reads(c["rows"], c["lens"], targets=(c["twords"], c["tbegin"], c["tlen"]), pair_off=c.get("pair_off"), **c["params"])
    c = QC.case("repeats")
    try:
        assert_same(eng.drop_contained(QC.targets(c), **c["variants"][0]).to_host(), QC.checked("repeats"), "k = 8")
        eng.set_option("place_dir_bits", 3)
        got, want = place(PC.case("many_seeds")).to_host(), PC.checked("many_seeds")
        for k in P.ARRAYS:
            assert (got[k] == want[k]).all(), k
        eng.set_option("place_dir_bits", 0)
        assert_same(eng.drop_contained(QC.targets(QC.case("seed63"))).to_host(), QC.checked("seed63"), "k = 21 after a placement")
    finally:
        eng.set_option("place_dir_bits", 0)


def test_refusals_leave_an_earlier_result_valid(eng, tmp_path):
    c, want = QC.case("duplicates"), QC.checked("duplicates")
    kp = eng.drop_contained(QC.targets(c))
    assert_same(kp.to_host(), want, "before")
    neg = c["tlen"].copy()
    neg[3] = -1
    calls = [dict(tlen=neg), dict(k=7), dict(k=32), dict(max_permille=-1), dict(max_permille=101), dict(max_occ=0), dict(max_occ=65536), dict(flags=1), dict(reserved=1)]
    for change in calls:
        tg = (c["twords"], c["tbegin"], change.get("tlen", c["tlen"]))
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.drop_contained(tg, **{k: v for k, v in change.items() if k != "tlen"})
        assert ei.value.code == -1, (list(change), ei.value)
        assert_same(kp.to_host(), want, ("after a refusal", list(change)))       # nothing written: the earlier result as it was
    with pytest.raises(TypeError):
        eng.drop_contained(QC.targets(c), max_mismatches=1)
    # three lengths of 2^31 - 1: the column sum is above 2^32 - 2, refused after the check and before a base is read
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.drop_contained((c["twords"], np.zeros(3, np.int64), np.full(3, 2 ** 31 - 1, np.int32)))
    assert ei.value.code == -5, ei.value                                         # ALGA_ERR_CAPACITY
    assert_same(kp.to_host(), want, "after the capacity refusal")
    path = str(tmp_path / "k.fasta")
    eng.write_kept_fasta(path, kp)
    assert open(path, "rb").read() == CC.fasta(want)
    again = eng.drop_contained(QC.targets(c))
    assert_same(again.to_host(), want, "the engine afterwards")
    with pytest.raises(alga_amd.AlgaError):
        eng.write_kept_fasta(path, kp)                                           # `kp` is the result before the last one: a stale handle
    eng.write_kept_fasta(path, again)
    assert open(path, "rb").read() == CC.fasta(want)


def test_a_result_stays_valid_across_the_other_stages(eng, tmp_path):
    import merge_cases as MQ
    c, want = QC.case("two_hosts"), QC.checked("two_hosts")
    other, m = PC.case("repeat"), MQ.case("path5")
    kp = eng.drop_contained(QC.targets(c))
    eng.place_reads(other["rows"], other["lens"], targets=(other["twords"], other["tbegin"], other["tlen"]), pair_off=other.get("pair_off"), **other["params"])
    eng.merge_ends(MQ.targets(m))
    assert_same(kp.to_host(), want, "after a later placement and merge")
    path = str(tmp_path / "k.fasta")
    eng.write_kept_fasta(path, kp)                                               # the bases are the result's own copy
    assert open(path, "rb").read() == CC.fasta(want)
    # the kept contigs as the targets of a placement
    seqs = CC.sequences(want)
    reads = [s[a:a + 60] for s in seqs for a in (0, len(s) - 60)]
    rows, lens = P.nodes_of(reads)
    got = eng.place_reads(rows, lens, targets=kp.targets()).to_host()
    want_pl = P.place(rows, lens, None, want["words"], want["begin"].astype(np.int64), want["len"])
    for k in P.ARRAYS:
        assert (got[k] == want_pl[k]).all(), k
    assert want_pl["info"]["placed"] == len(reads) == 2 * len(seqs)


def planted_with_extras(eng):
    """the planted genome of the grow and merge tests after three rounds of place -> grow and the merge (one contig, the genome's window 11 ..
    2992), and two planted extras: a 300-base copy of an inner stretch with one substitution, the reverse complement of another stretch"""
    c, g, meta = GQ.planted()
    tg = (c["twords"], c["tbegin"], c["tlen"])
    for rnd in range(3):
        pl = eng.place_reads(c["rows"], c["lens"], targets=tg)
        gw = eng.grow_ends(c["rows"], c["lens"], pl)
        tg = gw.targets()
    merged = [g[11:2992]]
    mg = eng.merge_ends(tg)
    got = mg.to_host()
    assert mg.n_merged == 1 and (P.codes_of(got["words"], 0, int(got["len"][0])) == merged[0]).all()
    copy = np.array(g[700:1000], copy=True)
    copy[150] = (copy[150] + 1) & 3
    return c, merged + [copy, P.revcomp(g[1800:2150])]


def test_planted_pipeline(eng):
    c, seqs = planted_with_extras(eng)
    tw, tb, tl = P.ragged(seqs, [3 * i % 16 for i in range(len(seqs))])
    want = CC.contain_index(seqs)
    kp = eng.drop_contained((tw, tb, tl))
    assert_same(kp.to_host(), want, "planted")
    i = kp.info
    assert (i["contained"], i["contained_minus"], i["kept"], i["bases_removed"], i["ambiguous"]) == (2, 1, 1, 650, 0)
    assert want["host"].tolist() == [-1, 0, 0] and want["host_pos"].tolist() == [0, 700 - 11, 1800 - 11] and want["mm"].tolist() == [0, 1, 0]
    # the reads on the doubled stretches are placed twice on the input set and once on the kept set: more UNIQUE reads, as the Python placement counts them
    before = eng.place_reads(c["rows"], c["lens"], targets=(tw, tb, tl)).info
    after = eng.place_reads(c["rows"], c["lens"], targets=kp.targets()).info
    want_before = P.place(c["rows"], c["lens"], None, tw, tb, tl)["info"]
    want_after = P.place(c["rows"], c["lens"], None, want["words"], want["begin"].astype(np.int64), want["len"])["info"]
    print(i, before, after)
    assert before["unique"] == want_before["unique"] and after["unique"] == want_after["unique"] and before["placed"] == want_before["placed"]
    assert after["unique"] > before["unique"]


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, c in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in c)))


def codes(s):
    return np.array(["ACGT".index(x) for x in s], dtype=np.uint8)


def test_command_line(eng, tmp_path):
    """the reads of the merge stage's command-line test (two contigs whose ends overlap) and, beside them, the reads of a 500-base copy of an inner
    stretch with four substitutions.  alga_hip with --merge_ends=1 --drop_contained=1 --kept= --contain_layout=: the files against the Python API
    doing the same on the contigs the run writes, and against the checker; a run with --drop_contained=0 writes what a run without the option
    writes"""
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
    copy = np.array(g[1000:1500], copy=True)
    for q in (100, 200, 300, 400):
        copy[q] = (copy[q] + 1) & 3
    for a in range(0, 500 - 300 + 1, 4):                                         # pairs of the copy at insert 300
        m1.append(copy[a:a + 100])
        m2.append(P.revcomp(copy[a + 200:a + 300]))
    _write_fasta(str(tmp_path / "a.fasta"), m1)
    _write_fasta(str(tmp_path / "b.fasta"), m2)
    base = [exe, "--file1=a.fasta", "--file2=b.fasta", "--output=o.fasta", "--contigs_min_length=150", "--consensus_min_votes=0", "--retl=0", "--retr=0", "--grow_ends=1",
            "--merge_ends=1", "--merge_min_overlap=30"]
    files = ("--contigs_final=f%s.fasta", "--scaffolds=s%s.fasta", "--scaffold_layout=l%s.tsv", "--grown=g%s.fasta", "--merged=m%s.fasta", "--merge_layout=m%s.tsv")
    run = lambda args: subprocess.run(args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    r0 = run(base + [f % "0" for f in files])
    assert r0.returncode == 0, r0.stderr[-2000:]
    r1 = run(base + [f % "1" for f in files] + ["--drop_contained=0"])
    assert r1.returncode == 0 and "Contained contigs dropped" not in r0.stderr + r1.stderr, r1.stderr[-2000:]
    names = ("f%s.fasta", "s%s.fasta", "l%s.tsv", "g%s.fasta", "m%s.fasta", "m%s.tsv")
    for n in names:
        assert open(str(tmp_path / (n % "0")), "rb").read() == open(str(tmp_path / (n % "1")), "rb").read(), n
    r = run(base + [f % "" for f in files] + ["--drop_contained=1", "--kept=k.fasta", "--contain_layout=k.tsv"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Contained contigs dropped:" in r.stderr and "Reads placed on the kept contigs" in r.stderr, r.stderr[-2000:]
    for n in ("f%s.fasta", "g%s.fasta", "m%s.fasta", "m%s.tsv"):                 # the final, the grown and the merged contigs are what they were
        assert open(str(tmp_path / (n % "")), "rb").read() == open(str(tmp_path / (n % "0")), "rb").read(), n
    short = [exe, "--file1=a.fasta", "--output=o2.fasta", "--contigs_final=f2.fasta", "--grow_ends=1"]
    for bad in (["--drop_contained=1"], ["--merge_ends=1", "--kept=k2.fasta"], ["--merge_ends=1", "--contain_layout=k2.tsv"], ["--merge_ends=1", "--drop_contained=2"],
                ["--merge_ends=1", "--drop_contained=1", "--contain_max_permille=101"]):
        rb = run(short + bad)
        assert rb.returncode == 2 and ("need" in rb.stderr or "must be" in rb.stderr), rb.stderr[-500:]
    # the Python API and the checker on the merged contigs the run wrote
    merged = [codes(s) for s in open(str(tmp_path / "m.fasta")).read().split("\n")[1::2] if s]
    tw, tb, tl = P.ragged(merged, [0] * len(merged))
    kp = eng.drop_contained((tw, tb, tl))
    want = CC.contain_index(merged)
    got = kp.to_host()
    assert_same(got, want, "the command line's contigs")
    i = kp.info
    said = "Contained contigs dropped: %d queries, %d candidates, %d contained (%d minus, %d duplicates), %d ambiguous, %d bases removed, N50 %d -> %d;" % (
        i["queries"], i["candidates"], i["contained"], i["contained_minus"], i["duplicates"], i["ambiguous"], i["bases_removed"], i["n50_before"], i["n50_after"])
    print(said, [len(s) for s in merged], r.stderr[-1500:])
    assert said in r.stderr, r.stderr[-3000:]
    assert i["contained"] >= 1 and i["kept"] < len(merged)                       # a contig of the copy between two substitutions is a stretch of the genome
    eng.write_kept_fasta(str(tmp_path / "api.fasta"), kp)
    assert open(str(tmp_path / "k.fasta"), "rb").read() == open(str(tmp_path / "api.fasta"), "rb").read() == CC.fasta(want)
    assert open(str(tmp_path / "k.tsv"), "rb").read() == kp.contain_tsv(tl, got).encode() == CC.contain_tsv(want, tl)
    rows, lens = P.nodes_of([x for pair in zip(m1, m2) for x in pair])
    pair_off = np.array([1, 1, 2, 2] * len(m1), dtype=np.uint8)
    pl = eng.place_reads(rows, lens, targets=kp.targets(), pair_off=pair_off)
    sc = eng.scaffold(rows, lens, pair_off, pl)
    eng.write_scaffold_fasta(str(tmp_path / "api_s.fasta"), pl, sc)
    assert open(str(tmp_path / "s.fasta"), "rb").read() == open(str(tmp_path / "api_s.fasta"), "rb").read()
    assert open(str(tmp_path / "l.tsv"), "rb").read() == sc.layout_tsv().encode()
