"""The grow stage on the GPU against the families of tests/grow_fuzz.py: every output array, every counter, the FASTA bytes and the TSV bytes equal
to the Python definition (tests/grow_checker.py) on a thousand targets of every length around the word and min_anchor, overhangs of up to 237
bases, one-letter, periodic and shared ends, ends with 1 to 200 voters on the bounds of the decision, and the bounds of k, min_anchor, W, the
mismatches and max_grow (tests/test_grow_fuzz_cpu.py asserts that each family holds what it is for); the same with every grid of the k_gr_*
kernels capped at 1 and at 3 blocks (option grow_max_blocks), so that every grid-stride and wave-stride loop takes further passes and a last
partial one, and 2 000 reads behind eight 66-seed reads through four waves of k_gr_place; the option's range; a polish between; a second round
on Grown.targets(); a placement at another k between two calls on one engine.

Measured on an MI355X: the whole file in 8.1 s, nearly all of it the checker's (`many_targets` 1.9 s, its polished variants 1.3 s) and the
engine's start (2.2 s); the slowest test is `many_targets` (2.6 s); the device calls of a family with their read-backs take 0.01 to 0.08 s; the
slowest call's ms_total is 1.4 ms at the default cap (`many_targets`), 10.1 ms for `many_targets` with one block of 256 threads and 3.9 ms with
three.  Every test prints its own figures (-s)."""
import collections
import time

import numpy as np
import pytest

import alga_amd
import grow_cases as QC
import grow_checker as GC
import grow_fuzz as F
import place_checker as P

pytestmark = pytest.mark.gpu
SLOWEST = collections.defaultdict(float)                                         # test -> the largest ms_total of its calls
SHOWN = ("candidates", "voting", "multi", "hits_saturated", "ends_grown", "bases_added", "longest_growth", "stops_cover", "stops_percent", "stops_max")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what, seed):
    diff = F.first_difference(got, want)
    if diff is not None:
        print("%s, seed %d: first difference (array, index, got, want): %s" % (what, seed, diff))
    for k in GC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, seed, k, got[k].dtype, got[k].shape, want[k].shape, diff)
        assert (got[k] == want[k]).all(), (what, seed, k, diff, np.nonzero(got[k] != want[k])[0][:10])
    info = {k: v for k, v in got["info"].items() if not k.startswith("ms_")}
    assert info == want["info"], (what, seed, diff, info, want["info"])


def targets(c):
    return c["twords"], c["tbegin"], c["tlen"]


def device_args(c):
    import torch
    t = lambda a, view=None: torch.from_numpy(a.view(view) if view else a).cuda()
    return t(c["rows"], np.int32), t(c["lens"]), (t(c["twords"], np.int32), t(c["tbegin"]), t(c["tlen"]))


def placed_on_device(eng, c, want_pl, reads=None, tg=None):
    """the placement of the case; its state is the checker's (the placement has its own tests: here it is the input)"""
    rows, lens = reads if reads is not None else (c["rows"], c["lens"])
    pl = eng.place_reads(rows, lens, targets=tg if tg is not None else targets(c), **c["params"])
    assert (pl.to_host()["state"] == want_pl["state"]).all()
    return pl


def grown(eng, rows, lens, pl, what, **kw):
    gw = eng.grow_ends(rows, lens, pl, **kw)
    SLOWEST[what] = max(SLOWEST[what], gw.info["ms_total"])
    return gw


def run_family(eng, name, tmp_path, what, dir_bits=(1, 0), text=True, tensors=True):
    """every variant from host arrays at each directory width and from tensors, which are left untouched like the placement; the sizes of the
    result, the FASTA and the TSV"""
    c = F.case(name)
    seed = F.SEEDS.get(name, 117)
    path = str(tmp_path / "g.fasta")
    t0 = time.time()
    want_pl = F.placed(name)
    wants = [F.checked(name, i) for i in range(len(c["variants"]))]
    t_check, t_dev = time.time() - t0, 0.0
    pl = placed_on_device(eng, c, want_pl)
    try:
        for i, v in enumerate(c["variants"]):
            want = wants[i]
            for bits in dir_bits:
                eng.set_option("place_dir_bits", bits)
                t0 = time.time()
                gw = grown(eng, c["rows"], c["lens"], pl, what, **v)
                got = gw.to_host()
                t_dev += time.time() - t0
                assert_same(got, want, (name, i, "host arrays, directory bits", bits), seed)
            assert (gw.n_reads, gw.n_targets, gw.n_columns, gw.max_grow) == (len(c["lens"]) // 2, len(c["tlen"]), int(want["col_off"][-1]), dict(GC.DEFAULT, **v)["max_grow"])
            if text:
                info = eng.write_grown_fasta(path, gw)
                data = open(path, "rb").read()
                assert data == F.fasta(name, i), (name, i, seed)
                assert info["segments"] == int((want["len"] > 0).sum()) and info["bytes"] == len(data)
                assert gw.grow_tsv().encode() == gw.grow_tsv(got).encode() == GC.grow_tsv(want), (name, i, seed)
            print(name, i, {k: gw.info[k] for k in SHOWN})
    finally:
        eng.set_option("place_dir_bits", 0)
    if tensors:
        rows, lens, tg = device_args(c)
        keep = [x.clone() for x in (rows, lens, *tg)]
        pl = placed_on_device(eng, c, want_pl, (rows, lens), tg)
        before = pl.to_host()
        for i, v in enumerate(c["variants"]):
            t0 = time.time()
            got = grown(eng, rows, lens, pl, what, **v).to_host()
            t_dev += time.time() - t0
            assert_same(got, wants[i], (name, i, "tensors"), seed)
        for a, b in zip([rows, lens, *tg], keep):
            assert (a == b).all()
        after = pl.to_host()
        assert all((before[k] == after[k]).all() for k in P.ARRAYS)             # the placement is left as it was
    print("%s: the checkers %.2f s, the grow calls with their read-backs %.2f s, the slowest call %.2f ms" % (what, t_check, t_dev, SLOWEST[what]))


@pytest.mark.parametrize("name", F.GPU_FAMILIES)
def test_family_equals_the_checker(eng, name, tmp_path):
    run_family(eng, name, tmp_path, name)


@pytest.mark.parametrize("blocks", [1, 3])
def test_every_grid_strides(eng, blocks, tmp_path):
    """grow_max_blocks 1: 256 threads, four waves, for 2 000 ends, 1 000 targets, 3 100 candidates and more than 5 000 words of the old columns, of
    the end columns and of the result, so every per-end, per-target, per-word and per-candidate loop takes further passes; 3: 768 threads, so
    the last pass is a partial one"""
    c = F.case("many_targets")
    floor = 3 * 256 + 30
    assert len(c["tlen"]) + 1 > floor and all(F.checked("many_targets", i)["info"]["candidates"] > 3 * 1024 + 30 for i in range(3))
    assert int(c["tlen"].sum()) > 16 * floor
    try:
        eng.set_option("grow_max_blocks", blocks)
        run_family(eng, "many_targets", tmp_path, "many_targets at %d blocks" % blocks, dir_bits=(0,), tensors=blocks == 1)
    finally:
        eng.set_option("grow_max_blocks", 8192)
    pl = placed_on_device(eng, c, F.placed("many_targets"))
    assert_same(grown(eng, c["rows"], c["lens"], pl, "many_targets", **c["variants"][0]).to_host(), F.checked("many_targets"), ("many_targets", "the cap back at its default"),
                F.SEEDS["many_targets"])


def test_four_waves_take_two_thousand_reads(eng):
    """grow_cases.many_reads(2000) at one block: each of the four waves of k_gr_place takes about 440 candidates, the first two of them 1400-nt
    reads of 66 seeds, whose usable masks of two chunks stay in the wave's scratch under every short read after them"""
    c = QC.many_reads(2000)
    want_pl = P.place(*QC.place_args(c))
    t0 = time.time()
    want = GC.grow_index(c["rows"], c["lens"], want_pl, c["seqs"])
    t_check = time.time() - t0
    assert want["info"]["candidates"] > 4 * 400 and (want["over"][:8] == np.arange(10, 18)).all() and want["info"]["voting"] > 900
    pl = placed_on_device(eng, c, want_pl)
    try:
        eng.set_option("grow_max_blocks", 1)
        gw = grown(eng, c["rows"], c["lens"], pl, "many_reads")
        assert_same(gw.to_host(), want, "many_reads(2000) at one block", 117)
    finally:
        eng.set_option("grow_max_blocks", 8192)
    assert_same(grown(eng, c["rows"], c["lens"], pl, "many_reads").to_host(), want, "many_reads(2000), the cap back at its default", 117)
    c2 = F.case("edges")
    pl = placed_on_device(eng, c2, F.placed("edges"))
    assert_same(grown(eng, c2["rows"], c2["lens"], pl, "many_reads", **c2["variants"][1]).to_host(), F.checked("edges", 1), "edges after it", F.SEEDS["edges"])
    print("many_reads(2000): the checker %.2f s, %s, the slowest call %.2f ms" % (t_check, {k: gw.info[k] for k in SHOWN}, SLOWEST["many_reads"]))


def test_the_option_has_its_range(eng):
    for bad in (0, -1, 8193):
        with pytest.raises(alga_amd.AlgaError) as ei:
            eng.set_option("grow_max_blocks", bad)
        assert ei.value.code == -1
    c = F.case("votes")
    pl = placed_on_device(eng, c, F.placed("votes"))
    assert_same(grown(eng, c["rows"], c["lens"], pl, "votes", **c["variants"][1]).to_host(), F.checked("votes", 1), "after the refused values", F.SEEDS["votes"])
    eng.set_option("grow_max_blocks", 8192)                                      # the bounds themselves are taken
    eng.set_option("grow_max_blocks", 1)
    eng.set_option("grow_max_blocks", 8192)


@pytest.mark.parametrize("name", ["many_targets", "long_overhangs"])
def test_a_polish_between(eng, name):
    """the bases of the grown targets and of the ends the reads are laid on are the polished ones"""
    c = F.case(name)
    t0 = time.time()
    wants = [F.checked_polished(name, i) for i in range(len(c["variants"]))]
    t_check = time.time() - t0
    pl = placed_on_device(eng, c, F.placed(name))
    pol = eng.polish(c["rows"], c["lens"], pl)
    for i, v in enumerate(c["variants"]):
        assert_same(grown(eng, c["rows"], c["lens"], pl, name + " polished", polished=pol, **v).to_host(), wants[i], (name, i, "polished"), F.SEEDS[name])
    print("%s polished: the checkers %.2f s, the slowest call %.2f ms" % (name, t_check, SLOWEST[name + " polished"]))


def test_a_second_round_on_the_grown_targets(eng, tmp_path):
    """`long_overhangs` at max_grow 200: place -> grow -> place on Grown.targets() -> grow.  The second placement reads the first result's
    bases where they are, and the second grow call writes the other set of result buffers while that placement's columns are read"""
    name, i = "long_overhangs", 0
    c = F.case(name)
    v = c["variants"][i]
    assert v == dict(min_cover=1, max_grow=200)
    t0 = time.time()
    first = F.checked(name, i)
    c2, want_pl2, second = F.second_round(name, i)
    t_check = time.time() - t0
    assert first["info"]["ends_grown"] == 80 and want_pl2["info"]["placed"] > 100 and second["info"]["voting"] > 100 and second["info"]["ends_with_voters"] > 40 and second["info"]["ends_grown"] >= 3
    pl = placed_on_device(eng, c, F.placed(name))
    gw = grown(eng, c["rows"], c["lens"], pl, "two rounds", **v)
    assert_same(gw.to_host(), first, "round 1", F.SEEDS[name])
    assert [(a == b).all() for a, b in zip(GC.sequences(first), c2["seqs"])] == [True] * len(c2["seqs"])
    pl2 = eng.place_reads(c["rows"], c["lens"], targets=gw.targets(), **c["params"])
    got_pl2 = pl2.to_host()
    for k in P.ARRAYS:
        assert (got_pl2[k] == want_pl2[k]).all(), k
    gw2 = grown(eng, c["rows"], c["lens"], pl2, "two rounds", **v)
    got2 = gw2.to_host()
    assert_same(got2, second, "round 2", F.SEEDS[name])
    eng.write_grown_fasta(str(tmp_path / "g.fasta"), gw2)
    assert open(str(tmp_path / "g.fasta"), "rb").read() == GC.fasta(second)
    assert gw2.grow_tsv(got2).encode() == GC.grow_tsv(second)
    print("two rounds: the checkers %.2f s, round 2 %s, the slowest call %.2f ms" % (t_check, {k: second["info"][k] for k in SHOWN}, SLOWEST["two rounds"]))


def test_a_placement_between_two_calls(eng):
    """a placement with reads of more than 64 seeds (it uses the per-wave scratch and another k) between two family calls on one engine: the index
    workspace, the directory, k and the usable-seed masks of the call before leave nothing behind"""
    import place_cases as PC
    pc = PC.case("many_seeds")
    for name, i in (("repeats", 0), ("edges", 1), ("votes", 4), ("long_overhangs", 2)):
        c, want = F.case(name), F.checked(name, i)
        v = c["variants"][i]
        pl = placed_on_device(eng, c, F.placed(name))
        assert_same(grown(eng, c["rows"], c["lens"], pl, "between", **v).to_host(), want, (name, i, "before the placement"), F.SEEDS[name])
        got = eng.place_reads(pc["rows"], pc["lens"], targets=(pc["twords"], pc["tbegin"], pc["tlen"]), pair_off=pc.get("pair_off"), **pc["params"]).to_host()
        for k in P.ARRAYS:
            assert (got[k] == PC.checked("many_seeds")[k]).all(), (name, i, k)
        pl = placed_on_device(eng, c, F.placed(name))
        assert_same(grown(eng, c["rows"], c["lens"], pl, "between", **v).to_host(), want, (name, i, "after the placement"), F.SEEDS[name])
