"""The merge stage on the GPU against the families of tests/merge_fuzz.py: every output array, every counter, the FASTA bytes and the TSV bytes equal
to the Python definition (tests/merge_checker.py) on long chains and rings in shuffled id order, chains whose overlaps carry a substitution,
low-complexity, periodic and duplicated ends, the bounds of overlap, word and seed, and chains of long windows (tests/test_merge_fuzz_cpu.py
asserts that each family holds what it is for); the same with the grids of the k_mg_* kernels capped at 1 and at 3 blocks, so that every
grid-stride loop takes further passes and a last partial one; a second round on Merged.targets(); the merged FASTA in three chunks; a placement
between two merges on one engine.

Measured on an MI355X: the whole file in 6.7 s, nearly all of it the checker's (`long_windows` 1.9 s, `chains` 1.2 s); the device calls of a
family with their read-backs take 0.01 to 0.04 s; the slowest call's ms_total is the file's first (34 ms: it allocates the workspaces), after it
5.2 ms (`repeats`), and 3.5 ms for `chains` with one block of 256 threads.  Every test prints its own figures (-s)."""
import collections
import time

import numpy as np
import pytest

import alga_amd
import merge_checker as MC
import merge_fuzz as F
import place_checker as P

pytestmark = pytest.mark.gpu
SLOWEST = collections.defaultdict(float)                                         # test -> the largest ms_total of its calls


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what, seed):
    diff = F.first_difference(got, want)
    if diff is not None:
        print("%s, seed %d: first difference (array, index, got, want): %s" % (what, seed, diff))
    for k in MC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, seed, k, got[k].dtype, got[k].shape, want[k].shape, diff)
        assert (got[k] == want[k]).all(), (what, seed, k, diff, np.nonzero(got[k] != want[k])[0][:10])
    info = {k: v for k, v in got["info"].items() if not k.startswith("ms_")}
    assert info == want["info"], (what, seed, diff, info, want["info"])


def device_targets(c):
    import torch
    return torch.from_numpy(c["twords"].view(np.int32)).cuda(), torch.from_numpy(c["tbegin"]).cuda(), torch.from_numpy(c["tlen"]).cuda()


def merged(eng, tg, what, **v):
    mg = eng.merge_ends(tg, **v)
    SLOWEST[what] = max(SLOWEST[what], mg.info["ms_total"])
    return mg


def run_family(eng, name, tmp_path, what, dir_bits=(1, 0), text=True):
    """every variant from host arrays at each directory width and from tensors, which are left untouched; the FASTA and the TSV"""
    c = F.case(name)
    path = str(tmp_path / "m.fasta")
    t0 = time.time()
    wants = [F.checked(name, i) for i in range(len(c["variants"]))]
    t_check, t_dev = time.time() - t0, 0.0
    tg = device_targets(c)
    keep = [x.clone() for x in tg]
    try:
        for i, v in enumerate(c["variants"]):
            want = wants[i]
            for bits in dir_bits:
                eng.set_option("place_dir_bits", bits)
                t0 = time.time()
                mg = merged(eng, F.targets(c), what, **v)
                got = mg.to_host()
                t_dev += time.time() - t0
                assert_same(got, want, (name, i, "host arrays, directory bits", bits), F.SEEDS[name])
            assert (mg.n_targets, mg.n_merged, mg.n_members, mg.n_columns) == (len(c["tlen"]), len(want["len"]), len(want["m_members"]), int(want["col_off"][-1]))
            if text:
                info = eng.write_merged_fasta(path, mg)
                data = open(path, "rb").read()
                assert data == F.fasta(name, i), (name, i)
                assert info["segments"] == len(want["len"]) and info["bytes"] == len(data)
                assert mg.merge_tsv().encode() == mg.merge_tsv(c["tlen"], got).encode() == MC.merge_tsv(want, c["tlen"]), (name, i)
            t0 = time.time()
            got = merged(eng, tg, what, **v).to_host()
            t_dev += time.time() - t0
            assert_same(got, want, (name, i, "tensors"), F.SEEDS[name])
            print(name, i, {k: mg.info[k] for k in ("ends_with_overlap", "ends_ambiguous", "joins", "joins_dropped_cycle", "merged", "hits_saturated", "seeds_over_max_occ")})
    finally:
        eng.set_option("place_dir_bits", 0)
    for a, b in zip(tg, keep):
        assert (a == b).all()
    print("%s: the checker %.2f s, the device calls with their read-backs %.2f s, the slowest call %.2f ms" % (what, t_check, t_dev, SLOWEST[what]))


@pytest.mark.parametrize("name", [n for n in F.GPU_FAMILIES if n != "long_windows"])      # (long_windows: in the test of its chunks, below)
def test_family_equals_the_checker(eng, name, tmp_path):
    run_family(eng, name, tmp_path, name)


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("name", ["chains", "chain_mismatches"])
def test_every_grid_strides(eng, name, blocks, tmp_path):
    """merge_max_blocks 1: 256 threads for more than 1 600 ends, 800 contigs and 4 700 words, so every per-end, per-state, per-contig and per-word
    loop takes further passes; 3: 768 threads, so the last pass is a partial one"""
    c = F.case(name)
    assert len(c["tlen"]) > 3 * 256 + 30 and all(F.checked(name, i)["info"]["columns_after"] > 16 * (3 * 256 + 30) for i in range(len(c["variants"])))
    try:
        eng.set_option("merge_max_blocks", blocks)
        run_family(eng, name, tmp_path, "%s at %d blocks" % (name, blocks), dir_bits=(0,), text=blocks == 1)
    finally:
        eng.set_option("merge_max_blocks", 8192)
    want = F.checked(name)
    assert_same(merged(eng, F.targets(c), name).to_host(), want, (name, "the cap back at its default"), F.SEEDS[name])


def test_the_option_has_its_range(eng):
    for bad in (0, -1, 8193):
        with pytest.raises(alga_amd.AlgaError):
            eng.set_option("merge_max_blocks", bad)
    c = F.case("edges")
    assert_same(merged(eng, F.targets(c), "edges", **c["variants"][1]).to_host(), F.checked("edges", 1), "after the refused values", F.SEEDS["edges"])


def test_a_second_round_on_the_merged_targets(eng, tmp_path):
    """`chains` at max_overlap 50 joins what overlaps by up to 50 and leaves the longer overlaps to a second round at the default, whose targets
    are the first round's result: it is read while the other set is written"""
    c = F.case("chains")
    v = c["variants"][1]
    assert v == dict(max_overlap=50)
    t0 = time.time()
    first = F.checked("chains", 1)
    c2, second = F.second_round("chains", 1)
    t_check = time.time() - t0
    assert first["info"]["joins"] > 1000 and second["info"]["joins"] > 1000 and second["info"]["merged_multi"] >= 20
    mg = merged(eng, F.targets(c), "two rounds", **v)
    assert_same(mg.to_host(), first, "round 1", F.SEEDS["chains"])
    mg2 = merged(eng, mg.targets(), "two rounds")
    got2 = mg2.to_host()
    assert_same(got2, second, "round 2", F.SEEDS["chains"])
    eng.write_merged_fasta(str(tmp_path / "m.fasta"), mg2)
    assert open(str(tmp_path / "m.fasta"), "rb").read() == MC.fasta(second)
    assert mg2.merge_tsv(first["len"], got2).encode() == MC.merge_tsv(second, first["len"])
    print("two rounds: the checker %.2f s, round 2 %s, the slowest call %.2f ms" % (t_check, {k: second["info"][k] for k in ("joins", "joins_dropped_cycle", "merged")}, SLOWEST["two rounds"]))


def test_long_windows_and_their_fasta_in_three_chunks(eng, tmp_path):
    """the family as every other (host arrays at both directory widths, tensors left untouched, the FASTA in one chunk, the TSV), then the FASTA
    at gfa_chunk_mb 1.  The library reports no chunk count: that there are three or more follows from the bytes by the writer's rule (a chunk
    ends at a record boundary and holds at most the chunk size, so the step is the chunk less the longest record)"""
    c = F.case("long_windows")
    run_family(eng, "long_windows", tmp_path, "long_windows")
    want, text = F.checked("long_windows"), F.fasta("long_windows")
    mg = merged(eng, F.targets(c), "long_windows")
    path = str(tmp_path / "m.fasta")
    t0 = time.time()
    try:
        eng.set_option("gfa_chunk_mb", 1)
        out = eng.write_merged_fasta(path, mg)
    finally:
        eng.set_option("gfa_chunk_mb", 256)
    t_fasta = time.time() - t0
    data = open(path, "rb").read()
    longest = max(len(r) for r in data.split(b">")) + 1
    assert len(data) > 2 << 20 and 2 * longest < 1 << 20 and -(-len(data) // ((1 << 20) - longest)) >= 3   # three chunks of 1 MiB or more
    assert data == text
    assert out["segments"] == len(want["len"]) and out["bytes"] == len(data)
    print("long_windows: the chunked FASTA %.2f s (%d bytes, the longest record %d), the slowest call %.2f ms" % (t_fasta, len(data), longest, SLOWEST["long_windows"]))


def test_a_placement_between_two_merges(eng):
    """a placement with reads of more than 64 seeds (it uses the per-wave scratch and another k) between two family calls on one engine: the index
    workspace, the directory, k and the usable-seed masks of the call before leave nothing behind"""
    import place_cases as PC
    pc = PC.case("many_seeds")
    for name, i in (("repeats", 0), ("repeats", 3), ("chains", 0), ("edges", 2)):
        c, want = F.case(name), F.checked(name, i)
        v = c["variants"][i]
        assert_same(merged(eng, F.targets(c), "between", **v).to_host(), want, (name, i, "before the placement"), F.SEEDS[name])
        got = eng.place_reads(pc["rows"], pc["lens"], targets=(pc["twords"], pc["tbegin"], pc["tlen"]), pair_off=pc.get("pair_off"), **pc["params"]).to_host()
        for k in P.ARRAYS:
            assert (got[k] == PC.checked("many_seeds")[k]).all(), (name, i, k)
        assert_same(merged(eng, F.targets(c), "between", **v).to_host(), want, (name, i, "after the placement"), F.SEEDS[name])
