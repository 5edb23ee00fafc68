"""The read placement on the GPU (alga_place_reads_device, alga_place_reads_on_final_device, alga_write_final_fasta_depth_device): every output
array and every counter equal to the Python definition (tests/place_checker.py) on the cases of tests/place_cases.py, through host arrays and
through tensors, whatever the directory; more reads than k_pl_place has waves; the caller's stream; refusals leave an earlier result valid;
the capacity bound; the whole chain on a genome with a repeat; every width of the depth header; the command line."""
import os
import subprocess

import numpy as np
import pytest

import alga_amd
import consensus_checker as S
import final_checker as F
import graph_cases as GC
import place_cases as PC
import place_checker as P

pytestmark = pytest.mark.gpu
TIMES = ("ms_index", "ms_place", "ms_depth", "ms_total")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what=""):
    for k in P.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert (got[k] == want[k]).all(), (what, k, np.nonzero(got[k] != want[k])[0][:10])
    info = {k: v for k, v in got["info"].items() if k not in TIMES}
    assert info == want["info"], (what, info, want["info"])


def device_args(c):
    import torch
    t = lambda a, view=None: None if a is None else torch.from_numpy(a.view(view) if view else a).cuda()
    return (t(c["rows"], np.int32), t(c["lens"]), (t(c["twords"], np.int32), t(c["tbegin"]), t(c["tlen"])), t(c["pair_off"]))


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_every_case_equals_the_checker(eng, name):
    c = PC.case(name)
    snap = {k: (None if c[k] is None else c[k].copy()) for k in ("rows", "lens", "pair_off", "twords", "tbegin", "tlen")}
    for flags in (0, P.DEPTH_MULTI):
        pl = eng.place_reads(c["rows"], c["lens"], targets=(c["twords"], c["tbegin"], c["tlen"]), pair_off=c["pair_off"], flags=flags, **c["params"])
        assert_same(pl.to_host(), PC.checked(name, flags), (name, flags, "host arrays"))
    rows, lens, targets, po = device_args(c)
    keep = [x.clone() for x in (rows, lens, *targets)] + ([po.clone()] if po is not None else [])
    pl = eng.place_reads(rows, lens, targets=targets, pair_off=po, **c["params"])
    assert_same(pl.to_host(), PC.checked(name), (name, "tensors"))
    for a, b in zip([rows, lens, *targets] + ([po] if po is not None else []), keep):
        assert (a == b).all()
    for k, v in snap.items():
        assert v is None or (c[k] == v).all(), k
    print(name, pl.info)


@pytest.mark.parametrize("name", ["rand", "repeat", "unaligned", "saturate", "many_seeds", "tiny_targets"])
def test_the_directory_changes_nothing(eng, name):
    c = PC.case(name)
    try:
        for bits in (1, 4, 16, 26):
            eng.set_option("place_dir_bits", bits)
            pl = eng.place_reads(c["rows"], c["lens"], targets=(c["twords"], c["tbegin"], c["tlen"]), pair_off=c["pair_off"], **c["params"])
            assert_same(pl.to_host(), PC.checked(name), (name, bits))
        for k in (8, 13, 31):                                                    # the directory is never wider than the k-mer
            pl = eng.place_reads(c["rows"], c["lens"], targets=(c["twords"], c["tbegin"], c["tlen"]), pair_off=c["pair_off"], **dict(c["params"], k=k))
            assert_same(pl.to_host(), P.place(*PC.args(c), **dict(c["params"], k=k)), (name, "k", k))
    finally:
        eng.set_option("place_dir_bits", 0)


def test_a_wave_takes_more_than_one_read(eng):
    """k_pl_place runs at most 8 blocks of 4 waves per CU and a wave walks r += n_waves: with more reads than waves the state of a read (best,
    lane_mm, lane_cnt, the usable masks that the 1400-nt reads 0 .. 7 left in the scratch of waves 0 .. 7) must not reach the wave's next one"""
    import torch
    waves = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    n = (waves + 808 + 1) // 2 * 2
    assert n > waves
    c = PC.many_reads(n)
    want = P.place(*PC.args(c), **c["params"])
    late = want["state"][waves:]
    assert (late & P.PLACED).any() and (late == 0).any() and (late & P.MINUS).any()
    assert (c["lens"][:16] // PC.K > 64).all() and want["info"]["pairs"] == n // 2
    pl = eng.place_reads(c["rows"], c["lens"], targets=(c["twords"], c["tbegin"], c["tlen"]), pair_off=c["pair_off"], **c["params"])
    assert_same(pl.to_host(), want, "many_reads(%d)" % n)
    print(n, pl.info)


def test_the_callers_stream(eng):
    """tensors made on a stream of the caller's, the call on that stream; then a call on the engine's own stream"""
    import torch
    c = PC.case("pairs")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rows, lens, targets, po = device_args(c)
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    pl = eng.place_reads(rows, lens, targets=targets, pair_off=po, stream=s.cuda_stream, **c["params"])
    assert s.query()                                                             # the call returns with its work on the stream done
    assert_same(pl.to_host(), PC.checked("pairs"), "on the caller's stream")
    pl = eng.place_reads(rows, lens, targets=targets, pair_off=po, **c["params"])
    assert_same(pl.to_host(), PC.checked("pairs"), "on the engine's stream afterwards")


def test_refusals_leave_an_earlier_result_valid(eng):
    c = PC.case("pairs")
    want = PC.checked("pairs")
    tg = (c["twords"], c["tbegin"], c["tlen"])
    pl = eng.place_reads(c["rows"], c["lens"], targets=tg, pair_off=c["pair_off"], **c["params"])
    assert_same(pl.to_host(), want, "before")
    bad_twin = c["rows"].copy()
    bad_twin[6, 1] ^= 4
    bad_len = c["lens"].copy()
    bad_len[8] -= 1
    bad_mate = c["pair_off"].copy()
    bad_mate[6] = bad_mate[7] = 0                                                # nodes 4, 5 still name them
    above = c["pair_off"].copy()
    above[0] = above[1] = 3
    neg = c["tlen"].copy()
    neg[1] = -5
    calls = [dict(rows=bad_twin), dict(lens=bad_len), dict(pair_off=bad_mate), dict(pair_off=above), dict(tlen=neg)]
    calls += [dict(params=dict(c["params"], **kw)) for kw in (dict(k=7), dict(k=32), dict(max_mismatches=-1), dict(max_mismatches=255), dict(max_occ=0),
                                                              dict(max_occ=65536), dict(max_insert=0), dict(max_insert=(1 << 20) + 1), dict(flags=2))]
    for change in calls:
        a = dict(c, **change)
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.place_reads(a["rows"], a["lens"], targets=(a["twords"], a["tbegin"], a["tlen"]), pair_off=a["pair_off"], **a["params"])
        assert ei.value.code == -1, (change.keys(), ei.value)
        assert_same(pl.to_host(), want, "after a refusal")                       # nothing written: the earlier result as it was
    with pytest.raises(alga_amd.AlgaError):
        eng.place_reads(c["rows"][:-1], c["lens"][:-1], targets=tg)              # n odd
    again = eng.place_reads(c["rows"], c["lens"], targets=tg, pair_off=c["pair_off"], **c["params"])
    assert_same(again.to_host(), want, "the engine afterwards")


def test_capacity_is_refused_before_anything_of_that_size_is_allocated(eng):
    import torch
    c = PC.case("exact")
    pl = eng.place_reads(c["rows"], c["lens"], targets=(c["twords"], c["tbegin"], c["tlen"]))
    free0 = torch.cuda.mem_get_info()[0]
    for lens in ([2 ** 31 - 1, 2 ** 31 - 1, 1], [2 ** 31 - 1] * 3, [600] + [2 ** 31 - 1] * 4):
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.place_reads(c["rows"], c["lens"], targets=(c["twords"], np.zeros(len(lens), np.int64), np.array(lens, np.int32)))
        assert ei.value.code == -5, ei.value                                     # ALGA_ERR_CAPACITY
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)                    # (2^32 columns would take tens of GB)
    assert_same(pl.to_host(), PC.checked("exact"), "after the refusals")


@pytest.fixture(scope="module")
def chain(eng):
    """6 kb with a 400-nt repeat, error-free reads: build -> cut -> contigs -> consensus -> final (the set of the final-contig tests)"""
    r = GC.replicon_reads(circular=[], linear=[6000], n=2400, length=GC.READ_LEN, seed=31, copy=(1000, 4000, 400))
    e = eng.prefsuf_host(r.words, r.lens, GC.MIN_OVERLAP, GC.RSOEMO)
    cut = eng.cut_triangles_host(len(r.lens), e, GC.MOPP)
    u = eng.contigs(r.words, r.lens, cut, GC.MOPP)
    c = eng.unitig_consensus(r.words, r.lens, u, min_votes=0)
    fin = eng.final_contigs(u, c, 150, 95, 25)
    return r, cut, u, c, fin


def final_targets(uh, ch, fh):
    order = fh["order"].astype(np.int64)
    live = fh["verdict"][order] == F.ACCEPTED
    begin = 16 * uh["word_off"].astype(np.int64)[order] + np.where(live, fh["begin"][order], 0)
    return ch["words"], begin, np.where(live, fh["len"][order], 0).astype(np.int32)


def test_whole_chain_depth_of_the_final_contigs(eng, chain, tmp_path):
    r, cut, u, c, fin = chain
    uh, ch, fh = u.to_host(), c.to_host(), fin.to_host()
    pl = eng.place_reads(r.words, r.lens, final=fin)
    got = pl.to_host()
    want = P.place(r.words, r.lens, None, *final_targets(uh, ch, fh))
    assert_same(got, want, "on the final contigs")
    print(pl.info)
    assert pl.n_targets == fin.n_accepted >= 3 and got["info"]["unique"] > 2000 and got["info"]["multi"] > 0
    # the call leaves the results it reads as they were, and current
    for k in ("words", "word_off", "len", "path_node", "path_pos", "path_off", "edges"):
        assert (u.to_host()[k] == uh[k]).all(), k
    for k in ("words", "trim_left", "len", "changed"):
        assert (c.to_host()[k] == ch[k]).all(), k
    for k in F_KEYS:
        assert (fin.to_host()[k] == fh[k]).all(), k
    plain, deep = str(tmp_path / "plain.fasta"), str(tmp_path / "depth.fasta")
    eng.write_final_fasta(plain, fin)
    info = eng.write_final_fasta(deep, fin, placements=pl)
    a, b = open(plain).read().split("\n"), open(deep).read().split("\n")
    assert a[1::2] == b[1::2] and len(a) == len(b) and info["segments"] == fin.n_written and info["bytes"] == os.path.getsize(deep)
    heads = [P.depth_header(j, int(fh["len"][k]), want["t_reads"][j], want["t_bases"][j]) for j, k in enumerate(fh["order"]) if fh["verdict"][k] == F.ACCEPTED]
    assert b[0::2][:-1] == heads and all(h.startswith(x + "_reads=") for h, x in zip(b[0::2], a[0::2]) if x)
    # a placement on caller's targets is not one on the final result
    other = eng.place_reads(r.words, r.lens, targets=final_targets(uh, ch, fh))
    assert_same(other.to_host(), want, "the same windows as caller's targets")
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.write_final_fasta(deep, fin, placements=other)
    assert ei.value.code == -1
    # a stale final result: refused, for the placement and for the depth FASTA
    pl = eng.place_reads(r.words, r.lens, final=fin)
    fin2 = eng.final_contigs(u, c, 150, 95, 0)
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.write_final_fasta(deep, fin2, placements=pl)
    assert ei.value.code == -1
    c2 = eng.unitig_consensus(r.words, r.lens, u, min_votes=0)
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.place_reads(r.words, r.lens, final=fin2)
    assert ei.value.code == -1
    assert c2.n_pairs == u.n_pairs


def test_depth_header_widths(eng, tmp_path):
    """`>contig_id=<id>_length=<L>_reads=<n>_depth=<q>.<dd>` is formatted on the device with widths computed by hand: ids of one and two digits,
    lengths of two to four, reads of one to four (0 among them), q of one to three, dd below and above 10 (PC.HEADER_ENDS).  The contig set:
    14 reads without an edge, every one a contig of its own (tests/test_place_cpu.py: what the checkers of those stages say)"""
    words, lens = PC.header_nodes()
    u = eng.unitigs(words, lens, np.zeros((0, 3), np.int32), skip_isolated=False)
    c = eng.unitig_consensus(words, lens, u, min_votes=0)
    fin = eng.final_contigs(u, c, 1, 95, 0)
    uh, ch, fh = u.to_host(), c.to_host(), fin.to_host()
    tw, tb, tl = final_targets(uh, ch, fh)
    assert fin.n_accepted == 14 == fin.n_written and tl.tolist() == sorted(PC.HEADER_LENS, reverse=True)
    rows, rlens = P.nodes_of(PC.header_reads([P.codes_of(tw, tb[j], int(tl[j])) for j in range(14)]))
    pl = eng.place_reads(rows, rlens, final=fin)
    want = P.place(rows, rlens, None, tw, tb, tl)
    assert_same(pl.to_host(), want, "the header case")
    plain, deep = str(tmp_path / "plain.fasta"), str(tmp_path / "depth.fasta")
    eng.write_final_fasta(plain, fin)
    info = eng.write_final_fasta(deep, fin, placements=pl)
    a, b = open(plain).read().split("\n"), open(deep).read().split("\n")
    assert len(a) == len(b) == 29 and a[-1] == b[-1] == "" and a[1::2] == b[1::2] and info["segments"] == 14 and info["bytes"] == os.path.getsize(deep)
    assert b[0:28:2] == [P.depth_header(j, int(tl[j]), want["t_reads"][j], want["t_bases"][j]) for j in range(14)]
    for j, h in enumerate(b[0:28:2]):
        L = int(tl[j])
        assert h.startswith(a[2 * j] + "_reads=") and a[2 * j] == ">contig_id=%d_length=%d" % (j, L) and len(b[2 * j + 1]) == L
        assert h.endswith(PC.HEADER_ENDS[L]) if L != 1200 else PC.HEADER_ENDS[L] in h, h
    heads = dict(zip(tl.tolist(), b[0:28:2]))
    assert heads[1000] == ">contig_id=2_length=1000_reads=11_depth=1.05" and heads[40] == ">contig_id=12_length=40_reads=120_depth=120.00"
    assert heads[999] == ">contig_id=3_length=999_reads=0_depth=0.00" and heads[50] == ">contig_id=11_length=50_reads=0_depth=0.00"
    assert heads[1200].startswith(">contig_id=0_length=1200_reads=1000_depth=") and heads[21] == ">contig_id=13_length=21_reads=1_depth=1.00"
    minus = (want["state"] & P.MINUS).astype(bool)
    on480 = want["target"] == tl.tolist().index(480)
    assert on480.sum() == 3 and minus[on480].all() and not minus[~on480].any() and int(want["t_reads"][0]) == 1000


F_KEYS = ("verdict", "rank", "id", "new_reads", "trim_left", "begin", "len", "order")


def _write_fasta(path, codes):
    with open(path, "w") as f:
        for i, c in enumerate(codes):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in c)))


def test_command_line(tmp_path):
    """paired reads of a 4 kb genome through alga_hip: with --contigs_depth=1 --placements= the TSV and the headers are the checker's on the
    contigs the FASTA holds; with neither option the FASTA is byte for byte that of --contigs_depth=0"""
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    rng = np.random.default_rng(77)
    g = rng.integers(0, 4, size=4000, dtype=np.uint8)
    m1, m2 = [], []
    for a in rng.permutation(np.arange(0, 4000 - 300, 2)):
        ins = int(rng.integers(250, 301))
        m1.append(g[a:a + 100])
        m2.append(P.revcomp(g[a + ins - 100:a + ins]))
    _write_fasta(str(tmp_path / "a.fasta"), m1)
    _write_fasta(str(tmp_path / "b.fasta"), m2)
    out = {}
    for name, args in (("none", []), ("zero", ["--contigs_depth=0"]), ("depth", ["--contigs_depth=1", "--placements=p.tsv"]), ("tsv", ["--placements=p.tsv"])):
        wd = tmp_path / name
        wd.mkdir()
        r = subprocess.run([exe, "--file1=../a.fasta", "--file2=../b.fasta", "--output=o.fasta", "--contigs_final=f.fasta", "--contigs_min_length=150", "--retl=0", "--retr=0"] + args, cwd=str(wd),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert ("Reads placed on the final contigs" in r.stderr) == (name in ("depth", "tsv")), r.stderr[-2000:]
        out[name] = {f: open(str(wd / f)).read() for f in ("f.fasta", "p.tsv") if (wd / f).exists()}
    assert out["none"] == out["zero"] and list(out["none"]) == ["f.fasta"] and out["tsv"]["f.fasta"] == out["none"]["f.fasta"]
    assert out["tsv"]["p.tsv"] == out["depth"]["p.tsv"]
    plain, deep = out["none"]["f.fasta"].split("\n"), out["depth"]["f.fasta"].split("\n")
    assert plain[1::2] == deep[1::2] and len(plain) > 2
    # the records hold the contigs (ids may have gaps where a contig was trimmed away: a target of length 0)
    ids = [int(h.split("=")[1].split("_")[0]) for h in plain[0::2] if h]
    seqs = [np.array(["ACGT".index(x) for x in s], dtype=np.uint8) for s in plain[1::2] if s]
    targets = [np.zeros(0, np.uint8)] * (max(ids) + 1)
    for j, s in zip(ids, seqs):
        targets[j] = s
    reads = [x for pair in zip(m1, m2) for x in pair]
    rows, lens = P.nodes_of(reads)
    want = P.place(rows, lens, np.tile(np.array([1, 1, 2, 2], np.uint8), len(m1)), *P.ragged(targets, [0] * len(targets)))
    lines = ["%d\t%d\t%d\t%s\t%d\t%d" % (i, want["target"][i], want["pos"][i], "." if not want["state"][i] & P.PLACED else "-" if want["state"][i] & P.MINUS else "+",
                                         want["mm"][i], want["hits"][i]) for i in range(len(reads))]
    assert out["depth"]["p.tsv"] == "\n".join(lines) + "\n"
    assert [h for h in deep[0::2] if h] == [P.depth_header(j, len(targets[j]), want["t_reads"][j], want["t_bases"][j]) for j in ids]
    assert want["info"]["pairs_proper"] > 1000 and 250 <= want["info"]["insert_median"] <= 300
