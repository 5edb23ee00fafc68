"""The polish with the gapped reads on the GPU (alga_polish_indels_device and its two writers): every array, event, counter and both text outputs
equal to the Python definition (tests/ipolish_checker.py) byte for byte on the cases of tests/ipolish_cases.py, from host arrays and from
tensors, with and without COUNTS (counts.sum(axis=1) == the gapped cover), and with the k_ip_* grids capped at one or two blocks; a planted
set of 300 targets with every grid capped at one block, so that each grid-stride loop of the stage takes further passes (its sizes are asserted); the planted set comes back as the genome and a second round finds nothing; a gapped result with
nothing placed gives Engine.polish's words and changes; refusals leave the earlier result as it was; the caller's stream; the new targets
go into the placement; the command line; `many`: 2.1 M reads from a pool on 2.2 M columns, the loops at the real cap of 8192 blocks and both
texts in several chunks, against what the planting says."""
import numpy as np
import pytest

import alga_amd
import gapped_checker as GC
import ipolish_cases as XC
import ipolish_checker as IC
import place_checker as P
import polish_checker as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what=""):
    for k in IC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape)
        assert (got[k] == want[k]).all(), (what, k, np.nonzero(got[k] != want[k])[0][:10], got[k][got[k] != want[k]][:10], want[k][got[k] != want[k]][:10])
    info = {k: v for k, v in got["info"].items() if not k.startswith("ms_")}
    assert info == want["info"], (what, info, want["info"])


def stage(eng, c, want_pl=None, want_gp=None, tensors=False):
    """place -> gapped on the device, both equal to their checkers -> (rows, lens, pl, gp)"""
    import torch
    rows, lens, tg = c["rows"], c["lens"], XC.targets(c)
    if tensors:
        dev = torch.device("cuda", eng.device)
        rows, lens = torch.from_numpy(c["rows"].view(np.int32)).to(dev), torch.from_numpy(c["lens"]).to(dev)
        tg = (torch.from_numpy(c["twords"].view(np.int32)).to(dev), torch.from_numpy(c["tbegin"]).to(dev), torch.from_numpy(c["tlen"]).to(dev))
    pl = eng.place_reads(rows, lens, targets=tg, **c["place"])
    gp = eng.place_gapped(rows, lens, pl, targets=tg, **c["gapped"])
    if want_pl is not None:
        got = pl.to_host()
        for k in ("target", "pos", "state", "col_off"):
            assert (got[k] == want_pl[k]).all(), k
        got = gp.to_host()
        for k in GC.ARRAYS:
            assert (got[k] == want_gp[k]).all(), k
    return rows, lens, pl, gp


def check_result(eng, ip, want, gp_cover, tmp_path, what):
    got = ip.to_host()
    assert_same(got, want, what)
    assert (ip.n_targets, ip.n_columns_before, ip.n_columns, ip.n_events) == (len(want["len"]), want["info"]["columns"], want["info"]["columns_after"], len(want["ev_col"]))
    if "counts" in want:
        assert got["counts"].shape == want["counts"].shape and (got["counts"] == want["counts"]).all() and (got["span"] == want["span"]).all(), what
        assert (got["counts"].sum(axis=1) == gp_cover).all(), what
    else:
        assert ip.counts is None and ip.span is None
    fa, tsv = str(tmp_path / "i.fasta"), str(tmp_path / "i.tsv")
    i1, i2 = eng.write_ipolished_fasta(fa, ip), eng.write_ipolish_events_tsv(tsv, ip)
    text = open(fa, "rb").read().decode()
    assert text == IC.fasta(want), what
    assert i1["segments"] == int((want["len"] > 0).sum()) and i1["bytes"] == len(text)
    text = open(tsv, "rb").read().decode()
    assert text == IC.events_tsv(want), what
    assert i2["segments"] == len(want["ev_col"]) and i2["bytes"] == len(text)


@pytest.mark.parametrize("name", sorted(XC.CASES))
def test_every_case_equals_the_checker(eng, name, tmp_path):
    c = XC.case(name)
    want_pl, want_gp = XC.placed(name)
    for tensors in (False, True):
        rows, lens, pl, gp = stage(eng, c, want_pl, want_gp, tensors)
        for i, v in enumerate(c["variants"]):
            for counts in (False, True):
                if tensors and (i or counts):
                    continue
                want = XC.checked(name, i, counts)
                ip = eng.polish_indels(rows, lens, pl, gp, counts=counts, **v)
                check_result(eng, ip, want, want_gp["cover"], tmp_path, (name, i, counts, tensors))
                print(name, i, {k: ip.info[k] for k in ("voters_hamming", "voters_gapped", "substituted", "deleted", "inserted_slots", "ambiguous_columns", "ambiguous_slots")})


@pytest.mark.parametrize("name", ["normalise", "insert_vote", "seams", "deep"])
def test_grid_stride_loops_take_further_passes(eng, name, tmp_path):
    """every k_ip_* grid capped at 1 or 2 blocks of 256: the per-read and per-column loops need more than one pass (seams: 522 reads and 2931
    columns > 512; deep: 814 reads; normalise: 899 columns > 256) and the result is the same.  The words, the insertion votes and the targets of
    these cases fit one block: their loops stride in test_every_loop_strides_with_one_block"""
    c = XC.case(name)
    want_pl, want_gp = XC.placed(name)
    rows, lens, pl, gp = stage(eng, c)
    try:
        eng.set_option("ipolish_max_blocks", 2 if name != "normalise" else 1)
        for i, v in enumerate(c["variants"]):
            ip = eng.polish_indels(rows, lens, pl, gp, counts=True, **v)
            check_result(eng, ip, XC.checked(name, i, True), want_gp["cover"], tmp_path, (name, i))
    finally:
        eng.set_option("ipolish_max_blocks", 8192)


def test_word_seams_of_the_new_column_array(eng, tmp_path):
    """k_ip_words on tests/ipolish_cases.py: word_seams, at 8192 blocks and at one: targets whose new length is 1, 15, 16, 17, 31, 32 and 33 at
    offsets that insertions and deletions in the targets before them have moved, deleted columns between kept ones, a new total that is no
    multiple of 16 (the last word partial, the two of padding zero) and, with ipolish_max_blocks 1, two words per lane"""
    c = XC.case("word_seams")
    want_pl, want_gp = XC.placed("word_seams")
    want = XC.checked("word_seams", 0, False)
    assert want["len"].tolist() == [1, 15, 16, 120, 0, 17, 31, 120, 32, 33, 120, 4200] and c["tlen"].tolist() != want["len"].tolist()
    assert (want["t_dels"] > 0).sum() == (want["t_ins_bases"] > 0).sum() == 3 and int(want["col_off"][-1]) % 16 and (int(want["col_off"][-1]) + 15) // 16 + 2 > 256
    rows, lens, pl, gp = stage(eng, c, want_pl, want_gp)
    try:
        for blocks in (8192, 1):
            eng.set_option("ipolish_max_blocks", blocks)
            check_result(eng, eng.polish_indels(rows, lens, pl, gp), want, want_gp["cover"], tmp_path, ("word_seams", blocks))
    finally:
        eng.set_option("ipolish_max_blocks", 8192)


def run_planted_many(eng, m, tmp_path, **params):
    """place -> gapped -> polish_indels on a set of tests/ipolish_cases.py: many; every array, counter and both texts against what the planting
    says -> (the placement, the result, its host copy)"""
    import torch
    dev = torch.device("cuda", eng.device)
    rows, lens = torch.from_numpy(m["rows"].view(np.int32)).to(dev), torch.from_numpy(m["lens"]).to(dev)
    tg = tuple(torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(dev) for x in m["targets"])
    pl = eng.place_reads(rows, lens, targets=tg, **m["place"])
    gp = eng.place_gapped(rows, lens, pl, targets=tg)
    ip = eng.polish_indels(rows, lens, pl, gp, **params)
    got = ip.to_host()
    T, K, n, info, ev = len(m["truths"]), m["K"], m["n_reads"], ip.info, m["events"]
    assert info["voters_hamming"] + info["voters_gapped"] == n and info["voters_gapped"] == 4 * K * T and pl.info["placed"] == n - 4 * K * T
    assert (info["substituted"], info["deleted"], info["inserted_slots"], info["inserted_bases"], info["ambiguous_columns"], info["ambiguous_slots"]) == \
        (T * m["t_subs"], T, T, T, 0, 0)
    assert info["del_votes"] == info["ins_votes"] == 2 * K * T and info["max_cover"] == 2 * K and info["columns_after"] == ip.n_columns == m["truths"].size
    assert (got["len"] == m["truths"].shape[1]).all() and ip.n_events == len(ev)
    for t, s in enumerate(IC.sequences(got)):
        assert (s == m["truths"][t]).all(), t
    off = pl.to_host()["col_off"].astype(np.int64)
    assert (got["ev_col"] == np.array([off[e[0]] + e[1] for e in ev])).all() and (got["ev_kind"] == np.array([e[2] for e in ev])).all()
    assert (got["ev_votes"] == np.array([e[6] for e in ev])).all() and (got["ev_cover"] == np.array([e[7] for e in ev])).all() and (got["ev_len"] == 1).all()
    assert (got["t_subs"] == m["t_subs"]).all() and (got["t_dels"] == 1).all() and (got["t_ins_bases"] == 1).all() and (got["t_ambiguous"] == 0).all()
    assert (got["col_off"] == np.arange(T + 1) * m["truths"].shape[1]).all() and (got["begin"] == got["col_off"][:-1]).all()
    return pl, ip, got


def test_every_loop_strides_with_one_block(eng, tmp_path):
    """tests/ipolish_cases.py: many with 300 targets and every window once, every k_ip_* grid capped at ONE block of 256 threads: 187 500 new
    words (k_ip_words), 600 insertion votes (k_ip_ins_pick) and 301 targets (k_ip_targets) -- the three loops that no affordable input strides
    at 8192 blocks -- and the reads and columns with them all take further passes; min_cover 1, since a column is covered by two reads"""
    m = XC.many(300, 10000, 1)
    want_fa, want_tsv = XC.many_texts(m)
    try:
        eng.set_option("ipolish_max_blocks", 1)
        pl, ip, got = run_planted_many(eng, m, tmp_path, min_cover=1)
    finally:
        eng.set_option("ipolish_max_blocks", 8192)
    assert (ip.n_columns + 15) // 16 + 2 > 256 and ip.info["ins_votes"] == 600 > 256 and ip.n_targets + 1 == 301 > 256
    assert ip.n_columns_before > 256 and m["n_reads"] == 300 * 199 > 256
    fa, tsv = str(tmp_path / "o.fasta"), str(tmp_path / "o.tsv")
    eng.write_ipolished_fasta(fa, ip), eng.write_ipolish_events_tsv(tsv, ip)
    assert open(fa, "rb").read().decode() == want_fa and open(tsv, "rb").read().decode() == want_tsv


def test_planted_set_comes_back_as_the_genome(eng, tmp_path):
    """condition, not a measurement: place -> gapped -> polish_indels gives the genome exactly; a second round on the new target places every
    read with 0 mismatches by the Hamming pass alone and reports 0 events"""
    seed, c, g, want_pl, want_gp, want = XC.planted()
    print("seed", seed)
    rows, lens, pl, gp = stage(eng, c, want_pl, want_gp)
    ip = eng.polish_indels(rows, lens, pl, gp)
    check_result(eng, ip, want, want_gp["cover"], tmp_path, "planted")
    got = ip.to_host()
    seq = IC.sequences(got)[0]
    assert len(seq) == len(g) and (seq == g).all()
    print({k: v for k, v in ip.info.items()})
    tg = tuple(t.clone() for t in ip.targets)                        # the result is the engine's: the second round rewrites it
    pl2 = eng.place_reads(rows, lens, targets=tg, **c["place"])
    assert pl2.info["placed"] == pl2.info["reads"] == len(c["lens"]) // 2 and int(pl2.to_host()["mm"].max()) == 0
    gp2 = eng.place_gapped(rows, lens, pl2, targets=tg)
    assert gp2.info["tried"] == 0
    ip2 = eng.polish_indels(rows, lens, pl2, gp2)
    assert ip2.n_events == 0 and ip2.n_columns == 6000 and ip2.info["voters_gapped"] == 0 and (ip2.to_host()["words"] == got["words"]).all()


def test_no_gapped_voter_is_the_polish(eng):
    """existing code is the yardstick: with no G voter d_words and the S events are Engine.polish's d_words, d_changed_cols and d_changed_bases"""
    c = XC.case("no_gapped")
    rows, lens, pl, gp = stage(eng, c)
    assert gp.info["unique"] == 0
    for v in c["variants"]:
        po = eng.polish(rows, lens, pl, **v).to_host()
        ip = eng.polish_indels(rows, lens, pl, gp, **v)
        got = ip.to_host()
        assert ip.info["voters_gapped"] == 0 and (got["words"] == po["words"]).all() and (got["col_off"] == po["col_off"]).all()
        assert (got["ev_kind"] == IC.EV_S).all() and (got["ev_col"] == po["changed_cols"]).all() and (got["ev_bases"] == po["changed_bases"]).all()
        assert (got["t_subs"] == po["t_changed"]).all() and (got["t_ambiguous"] == po["t_ambiguous"]).all()
    # and a target with planted substitutions that the H voters repair
    g = XC.plain(120, 500)
    t = XC.edit(g, [("S", 100), ("S", 250)])
    c = XC.make(XC.windows(g, list(range(0, 400, 5))), [t])
    c["place"] = dict(k=21, max_mismatches=2)
    rows, lens, pl, gp = stage(eng, c)
    po, ip = eng.polish(rows, lens, pl).to_host(), eng.polish_indels(rows, lens, pl, gp)
    got = ip.to_host()
    assert len(po["changed_cols"]) == 2 and (got["words"] == po["words"]).all() and (got["ev_col"] == po["changed_cols"]).all() and (got["ev_bases"] == po["changed_bases"]).all()
    assert (IC.sequences(got)[0] == g).all()


def test_refusals_leave_the_earlier_result_as_it_was(eng, tmp_path):
    c = XC.case("normalise")
    rows, lens, pl, gp = stage(eng, c)
    want = XC.checked("normalise")
    refused = 0
    for kw in (dict(min_cover=0), dict(min_cover=2 ** 31), dict(min_percent=0), dict(min_percent=101), dict(max_ins=0), dict(max_ins=14)):
        with pytest.raises(alga_amd.AlgaError):
            eng.polish_indels(rows, lens, pl, gp, **kw)
        refused += 1
    lib, h = eng._lib, eng._h
    import ctypes as C
    import torch
    dev = torch.device("cuda", eng.device)
    rt, lt = torch.from_numpy(c["rows"].view(np.int32)).to(dev), torch.from_numpy(c["lens"]).to(dev)

    def call(nd_n=None, flags=0, reserved=0, pl_c=None, gp_c=None):
        nd = alga_amd.engine._Nodes(rt.data_ptr(), int(rt.shape[1]), lt.data_ptr(), len(c["lens"]) if nd_n is None else nd_n, None, None)
        pp, out = alga_amd.IpolishParams(), alga_amd.IpolishedC()
        lib.alga_ipolish_default_params(C.byref(pp))
        pp.flags, pp.reserved[2] = flags, reserved
        return lib.alga_polish_indels_device(h, C.byref(nd), C.byref(pl_c or pl._c), C.byref(gp_c or gp._c), C.byref(pp), None, C.byref(out), None)
    assert call() == 0                                                # (the raw call itself is right: what follows is refused for its argument)
    ip = eng.polish_indels(rows, lens, pl, gp)
    before = ip.to_host()
    for kw in (dict(flags=2), dict(reserved=1), dict(nd_n=len(c["lens"]) - 2)):
        assert call(**kw) != 0
        refused += 1
    twisted = rt.clone()
    twisted[0, 0] ^= 1                                                # the twin property: a device refusal
    with pytest.raises(alga_amd.AlgaError):
        eng.polish_indels(twisted, lt, pl, gp)
    refused += 1
    # a gapped result of an earlier placement; then a stale placement
    pl2 = eng.place_reads(rows, lens, targets=XC.targets(c), **c["place"])
    with pytest.raises(alga_amd.AlgaError):
        eng.polish_indels(rows, lens, pl2, gp)
    refused += 1
    gp2 = eng.place_gapped(rows, lens, pl2, targets=XC.targets(c))
    other = XC.case("ties")
    pl3 = eng.place_reads(other["rows"], other["lens"], targets=XC.targets(other), **other["place"])
    with pytest.raises(alga_amd.AlgaError):
        eng.polish_indels(rows, lens, pl2, gp2)
    refused += 1
    assert refused == 12
    # the result of the first call is as it was, and still the engine's current one: the writers take it
    after = ip.to_host()
    for k in IC.ARRAYS:
        assert (after[k] == before[k]).all(), k
    check_result(eng, ip, want, XC.placed("normalise")[1]["cover"], tmp_path, "after the refusals")
    assert pl3.n_reads == len(other["lens"]) // 2


def test_the_callers_stream_and_the_chain(eng, tmp_path):
    """the call on a stream of the caller's; IndelPolished.targets goes into place_reads and every repaired target is the truth"""
    import torch
    c = XC.case("seams")
    want_pl, want_gp = XC.placed("seams")
    rows, lens, pl, gp = stage(eng, c, tensors=True)
    st = torch.cuda.Stream(device=eng.device)
    ip = eng.polish_indels(rows, lens, pl, gp, stream=st.cuda_stream)
    check_result(eng, ip, XC.checked("seams"), want_gp["cover"], tmp_path, "stream")
    for s, t in zip(IC.sequences(ip.to_host()), c["truths"]):
        assert len(s) == len(t) and (s == t).all()
    words, begin, tlen = (t.clone() for t in ip.targets)
    pl2 = eng.place_reads(rows, lens, targets=(words, begin, tlen), **c["place"])
    assert pl2.info["placed"] == pl2.info["reads"] and pl2.n_columns == ip.n_columns


def _write_fasta(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[b] for b in r)))


def test_command_line(eng, tmp_path):
    """reads of a 3 kb genome, every fifth with one planted 1-base indel.  alga_hip --gapped=1 --polish_indels=1: --ipolished= and
    --ipolish_events= are the checker's texts for the contigs the run writes, and what the Python API gives for them; the stderr line carries
    the counters; every other file is what it is without the option; the option errors"""
    import os
    import subprocess
    import gapped_cases as QC
    exe = os.path.join(os.path.dirname(alga_amd.library_path()), "..", "bin", "alga_hip")
    rng = np.random.default_rng(78)
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
    r0 = run(base + ["--contigs_final=f0.fasta", "--contigs_depth=1", "--placements=p0.tsv", "--gapped=1", "--gapped_placements=g0.tsv"])
    assert r0.returncode == 0 and "polished with the gapped reads" not in r0.stderr, r0.stderr[-2000:]
    r = run(base + ["--contigs_final=f.fasta", "--contigs_depth=1", "--placements=p.tsv", "--gapped=1", "--gapped_placements=g.tsv", "--polish_indels=1",
                    "--ipolished=i.fasta", "--ipolish_events=e.tsv"])
    assert r.returncode == 0, r.stderr[-2000:]
    r1 = run(base + ["--contigs_final=f1.fasta", "--gapped=1", "--polish_indels=1", "--polish_max_ins=1", "--ipolished=i1.fasta"])
    assert r1.returncode == 0, r1.stderr[-2000:]
    for a, b in (("f0.fasta", "f.fasta"), ("p0.tsv", "p.tsv"), ("g0.tsv", "g.tsv")):
        assert open(str(tmp_path / a), "rb").read() == open(str(tmp_path / b), "rb").read(), a
    for bad in (["--contigs_final=f2.fasta", "--polish_indels=1"], ["--contigs_final=f2.fasta", "--gapped=1", "--ipolished=x.fasta"],
                ["--contigs_final=f2.fasta", "--gapped=1", "--ipolish_events=x.tsv"], ["--contigs_final=f2.fasta", "--gapped=1", "--polish_max_ins=3"],
                ["--contigs_final=f2.fasta", "--gapped=1", "--polish_indels=2"], ["--contigs_final=f2.fasta", "--gapped=1", "--polish_indels=1", "--polish_max_ins=0"],
                ["--contigs_final=f2.fasta", "--gapped=1", "--polish_indels=1", "--polish_max_ins=14"]):
        rb = run([exe, "--file1=a.fasta", "--output=o2.fasta"] + bad)
        assert rb.returncode == 2 and ("need" in rb.stderr or "must be" in rb.stderr), rb.stderr[-500:]
    contigs = open(str(tmp_path / "f.fasta")).read().split("\n")
    ids = [int(h.split("=")[1].split("_")[0]) for h in contigs[0::2] if h]
    tg = [np.zeros(0, np.uint8)] * (max(ids) + 1)
    for j, s in zip(ids, [np.array(["ACGT".index(x) for x in s], dtype=np.uint8) for s in contigs[1::2] if s]):
        tg[j] = s
    rows, lens = P.nodes_of(reads)
    tw, tb, tl = P.ragged(tg, [0] * len(tg))
    plh = P.place(rows, lens, None, tw, tb, tl)
    gph = GC.gapped_banded(rows, lens, plh, tw, tb, tl)
    pl = eng.place_reads(rows, lens, targets=(tw, tb, tl))
    gp = eng.place_gapped(rows, lens, pl, targets=(tw, tb, tl))
    for max_ins, fa, ev, res in ((6, "i.fasta", "e.tsv", r), (1, "i1.fasta", None, r1)):
        want = IC.ipolish_scatter(rows, lens, plh, gph, tw, tb, tl, max_ins=max_ins)
        ip = eng.polish_indels(rows, lens, pl, gp, max_ins=max_ins)
        eng.write_ipolished_fasta(str(tmp_path / "api.fasta"), ip)
        eng.write_ipolish_events_tsv(str(tmp_path / "api.tsv"), ip)
        text = open(str(tmp_path / fa), "rb").read()
        assert text.decode() == IC.fasta(want) and text == open(str(tmp_path / "api.fasta"), "rb").read() and len(text) > 1000, fa
        if ev:
            text = open(str(tmp_path / ev), "rb").read()
            assert text.decode() == IC.events_tsv(want) and text == open(str(tmp_path / "api.tsv"), "rb").read(), ev
        i = want["info"]
        said = ("Final contigs polished with the gapped reads (cover 3, 60 %%, insertions up to %d): %d + %d voters, %d substituted, %d deleted, %d inserted in %d slots, "
                "%d + %d ambiguous, columns %d -> %d;" % (max_ins, i["voters_hamming"], i["voters_gapped"], i["substituted"], i["deleted"], i["inserted_bases"],
                                                          i["inserted_slots"], i["ambiguous_columns"], i["ambiguous_slots"], i["columns"], i["columns_after"]))
        print(said)
        assert said in res.stderr, res.stderr[-3000:]
    assert i["voters_gapped"] >= 1


def test_many_reads_and_columns_and_texts_of_several_chunks(eng, tmp_path):
    """`many` (tests/ipolish_cases.py: many): 2 101 440 reads drawn 48 times from a pool of 43 780 windows, 2.2 M columns in 220 targets, 54 120
    planted events whose place, bases, votes and cover follow from the planting (tests/test_ipolish_cpu.py holds that derivation against the
    checker on a small instance).  The per-read loops (k_ip_check, k_ip_vote_gapped, k_ip_span) and the per-column loops (k_ip_decide,
    k_ip_events) take a second pass at the real cap of 8192 blocks of 256; the FASTA (2.2 MB) and the TSV (1.2 MB) are written in more than
    one chunk of 1 MiB, so records of k_ip_fasta_write and k_ip_tsv_write lie across chunk ends.  k_ip_words (one lane per 16 new columns: a
    second pass needs 33.5 M columns), k_ip_targets and k_ip_ins_pick do not stride here: test_every_loop_strides_with_one_block"""
    import time
    import torch
    t0 = time.time()
    m = XC.many()
    want_fa, want_tsv = XC.many_texts(m)
    t_build = time.time() - t0
    t0 = time.time()
    pl, ip, got = run_planted_many(eng, m, tmp_path)
    t_dev = time.time() - t0
    T, n, ev = len(m["truths"]), m["n_reads"], m["events"]
    print({k: v for k, v in ip.info.items()})
    assert n > 8192 * 256 and ip.n_columns_before > 8192 * 256
    fa, tsv = str(tmp_path / "m.fasta"), str(tmp_path / "m.tsv")
    t0 = time.time()
    try:
        eng.set_option("gfa_chunk_mb", 1)
        i1, i2 = eng.write_ipolished_fasta(fa, ip), eng.write_ipolish_events_tsv(tsv, ip)
    finally:
        eng.set_option("gfa_chunk_mb", 256)
    t_text = time.time() - t0
    text = open(fa, "rb").read()
    assert len(text) > 2 << 20 and text.decode() == want_fa and i1["segments"] == T and i1["bytes"] == len(text)      # three chunks of 1 MiB
    text = open(tsv, "rb").read()
    assert len(text) > 1 << 20 and text.decode() == want_tsv and i2["segments"] == len(ev) and i2["bytes"] == len(text)   # two chunks
    print("many: built in %.2f s, device calls with read-backs %.2f s, texts %.2f s" % (t_build, t_dev, t_text))
