"""The scaffold stage on the GPU against the families of tests/scaffold_fuzz.py (tests/test_scaffold_fuzz_cpu.py asserts that each family holds what
it is for): the device's placement equal to the one the family writes down, then every output array, every counter, the FASTA bytes and the
layout TSV equal to the Python definition (tests/scaffold_checker.py), and what holds for every result (tests/scaffold_invariants.py); the same
with the grids of the k_sc_* kernels capped at 1 and at 3 blocks (option "scaffold_max_blocks"), so that every grid-stride loop takes further
passes and a last partial one, and a wave of the FASTA writer writes many records; the case of several FASTA chunks with the cap at 2; small
calls after large ones on one engine and the other way round; tensors on a caller's stream; a polish between placement and scaffolds.
Every test prints its own figures (-s); DESIGN.md holds the measured times."""
import collections
import time

import numpy as np
import pytest

import alga_amd
import polish_checker as Q
import scaffold_cases as QC
import scaffold_checker as SC
import scaffold_fuzz as F
import scaffold_invariants as INV

pytestmark = pytest.mark.gpu
SLOWEST = collections.defaultdict(float)                                         # test -> the largest ms_total of its calls
PLACED = ("target", "pos", "state", "col_off")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what):
    for k in SC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert (got[k] == want[k]).all(), (what, k, np.nonzero(got[k] != want[k])[0][:10], got[k][got[k] != want[k]][:10], want[k][got[k] != want[k]][:10])
    info = {k: v for k, v in got["info"].items() if not k.startswith("ms_")}
    assert info == want["info"], (what, info, want["info"])


def targets(c):
    return c["twords"], c["tbegin"], c["tlen"]


def device_args(c):
    import torch
    t = lambda a, view=None: None if a is None else torch.from_numpy(a.view(view) if view else a).cuda()
    return t(c["rows"], np.int32), t(c["lens"]), (t(c["twords"], np.int32), t(c["tbegin"]), t(c["tlen"])), t(c["pair_off"])


def placed(eng, c, what, args=None, **kw):
    """the placement of the case, equal field for field to the one the family writes down before anything else is compared"""
    rows, lens, tg, po = args or (c["rows"], c["lens"], targets(c), c["pair_off"])
    pl = eng.place_reads(rows, lens, targets=tg, pair_off=po, **kw, **c["params"])
    got = pl.to_host()
    for k in PLACED:
        assert got[k].dtype == c["written"][k].dtype and (got[k] == c["written"][k]).all(), (what, "the placement", k)
    assert pl.info["pairs_split"] == c["written"]["info"]["pairs_split"]
    return pl


def scaffolded(eng, c, pl, v, what, args=None, **kw):
    rows, lens, _, po = args or (c["rows"], c["lens"], None, c["pair_off"])
    sc = eng.scaffold(rows, lens, po, pl, **kw, **v)
    SLOWEST[what] = max(SLOWEST[what], sc.info["ms_total"])
    return sc


def run_case(eng, key, tmp_path, what, text=True):
    """every variant of the case: arrays, counters, invariants, the FASTA bytes and the layout"""
    c = F.case(key)
    t0 = time.time()
    wants = [F.checked(key, i) for i in range(len(c["variants"]))]
    texts = [F.fasta(key, i) for i in range(len(c["variants"]))] if text else None
    t_check, t0 = time.time() - t0, time.time()
    path = str(tmp_path / "s.fasta")
    pl = placed(eng, c, (what, key))
    for i, v in enumerate(c["variants"]):
        want = wants[i]
        sc = scaffolded(eng, c, pl, v, what)
        got = sc.to_host()
        assert_same(got, want, (what, key, i))
        assert (sc.n_targets, sc.n_bundles, sc.n_scaffolds, sc.n_members) == (len(c["tlen"]), len(want["b_a"]), len(want["s_len"]), len(want["s_members"]))
        INV.every_result(c, pl.info["pairs_split"], got, v, text=False)
        if text:
            info = eng.write_scaffold_fasta(path, pl, sc)
            data = open(path, "rb").read()
            assert data == texts[i], (what, key, i)
            assert info["segments"] == sc.n_scaffolds and info["bytes"] == len(data)
            assert sc.layout_tsv().encode() == SC.layout_tsv(want, c["tlen"]), (what, key, i)
    print("%s %s: the checker %.2f s, the device calls with their read-backs %.2f s, the slowest call %.2f ms, %s" % (
        what, key, t_check, time.time() - t0, SLOWEST[what], {k: wants[0]["info"][k] for k in ("links", "bundles", "joins", "joins_dropped_cycle", "scaffolds")}))


@pytest.mark.parametrize("key", list(F.CASES))
def test_case_equals_the_checker(eng, key, tmp_path):
    run_case(eng, key, tmp_path, "default")


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("key", list(F.CASES))
def test_every_grid_strides(eng, key, blocks, tmp_path):
    """scaffold_max_blocks 1: 256 threads, so every loop over reads, links, bundles, ends, states and contigs of the larger cases takes further
    passes, and the four waves of the FASTA writer write every record; 3: 768 threads, so the last pass is a partial one"""
    try:
        eng.set_option("scaffold_max_blocks", blocks)
        run_case(eng, key, tmp_path, "%d blocks" % blocks)
    finally:
        eng.set_option("scaffold_max_blocks", 8192)


def test_the_capped_grids_do_stride():
    """what the capped runs rely on: the families hold more items of every kind than three blocks have threads"""
    n = 3 * 256 + 30
    assert len(F.case("many_targets")["tlen"]) > n and F.checked("many_targets")["info"]["bundles"] > n and F.checked("many_targets")["info"]["scaffolds"] > 4 * 3 * 30
    assert all(len(F.case(k)["lens"]) // 2 > n and F.checked(k)["info"]["links"] > n for k in ("bundle_edges", "wide_span", "rivals", "many_scaffolds", "whole_chains/513/first"))
    assert 2 * len(F.case("whole_chains/512/last")["tlen"]) > n and 2 * len(F.case("rings/257")["tlen"]) > 256


def test_the_option_has_its_range(eng):
    for bad in (0, -1, 8193):
        with pytest.raises(alga_amd.AlgaError):
            eng.set_option("scaffold_max_blocks", bad)
    c = F.case("rings/mixed")
    pl = placed(eng, c, "range")
    assert_same(scaffolded(eng, c, pl, c["variants"][0], "range").to_host(), F.checked("rings/mixed"), "after the refused values")


def test_fasta_in_several_chunks_with_the_grids_capped(eng, tmp_path):
    """the case of tests/test_gpu_scaffold.py with more than 2 MB of records, at 2 blocks and chunks of 1 MB: a chunk's records are written by
    eight waves"""
    c, want_pl = QC.chunks()
    v = c["variants"][0]
    want = SC.scaffold_dicts(*QC.scaffold_args(c, want_pl), **v)
    text = SC.fasta(want, c["seqs"])
    path = str(tmp_path / "s.fasta")
    try:
        eng.set_option("scaffold_max_blocks", 2)
        eng.set_option("gfa_chunk_mb", 1)
        pl = eng.place_reads(c["rows"], c["lens"], targets=targets(c), pair_off=c["pair_off"])
        got_pl = pl.to_host()
        for k in PLACED:
            assert (got_pl[k] == want_pl[k]).all(), k
        sc = scaffolded(eng, c, pl, v, "chunks")
        assert_same(sc.to_host(), want, "chunks at 2 blocks")
        info = eng.write_scaffold_fasta(path, pl, sc)
    finally:
        eng.set_option("gfa_chunk_mb", 256)
        eng.set_option("scaffold_max_blocks", 8192)
    data = open(path, "rb").read()
    assert len(data) > 2 << 20 and data == text and info["bytes"] == len(data) and info["segments"] == sc.n_scaffolds


@pytest.mark.parametrize("order", [("many_targets", "whole_chains/1/first", "whole_chains/3/last", "many_targets"),
                                   ("whole_chains/1/first", "whole_chains/3/last", "many_targets", "whole_chains/1/first", "whole_chains/3/last")])
def test_small_calls_after_large_ones_on_one_engine(order, tmp_path):
    """an engine of its own: the workspaces (best, partner, the lists, b_start[n_bundles]) are sized by the large call and reused by the small
    one, which must read nothing the large one left"""
    e = alga_amd.Engine(0)
    try:
        for step, key in enumerate(order):
            c = F.case(key)
            pl = placed(e, c, ("order", step, key))
            for i, v in enumerate(c["variants"]):
                sc = scaffolded(e, c, pl, v, "order")
                assert_same(sc.to_host(), F.checked(key, i), ("order", step, key, i))
                e.write_scaffold_fasta(str(tmp_path / "s.fasta"), pl, sc)
                assert open(str(tmp_path / "s.fasta"), "rb").read() == F.fasta(key, i), ("order", step, key, i)
    finally:
        e.close()


def test_tensors_on_the_callers_stream(eng):
    import torch
    c = F.case("rivals")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        args = device_args(c)
    s.synchronize()
    keep = [x.clone() for x in (args[0], args[1], *args[2], args[3])]
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    pl = placed(eng, c, "stream", args=args, stream=s.cuda_stream)
    for i, v in enumerate(c["variants"]):
        sc = scaffolded(eng, c, pl, v, "stream", args=args, stream=s.cuda_stream)
        assert s.query()                                                         # the call returns with its work on the stream done
        assert_same(sc.to_host(), F.checked("rivals", i), ("rivals", i, "on the caller's stream"))
    for a, b in zip((args[0], args[1], *args[2], args[3]), keep):
        assert (a == b).all()                                                    # the tensors are used where they are and left untouched


def test_a_polish_between_placement_and_scaffolds(eng, tmp_path):
    """rings/257 placed, polished, scaffolded: the scaffolds are the checker's and the FASTA takes its bases from the polished words"""
    key = "rings/257"
    c, want = F.case(key), F.checked(key)
    pl = placed(eng, c, "polish")
    pol = eng.polish(c["rows"], c["lens"], pl)
    want_pol = Q.polish_scatter(c["rows"], c["lens"], c["written"], *targets(c))
    assert (pol.to_host()["words"] == want_pol["words"]).all()
    sc = scaffolded(eng, c, pl, c["variants"][0], "polish")
    assert_same(sc.to_host(), want, "after a polish")
    plain, polished = str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta")
    eng.write_scaffold_fasta(plain, pl, sc)
    eng.write_scaffold_fasta(polished, pl, sc, polished=pol)
    assert open(plain, "rb").read() == F.fasta(key)
    assert open(polished, "rb").read() == SC.fasta(want, Q.sequences(want_pol))
