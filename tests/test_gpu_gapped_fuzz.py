"""The gapped placement on the GPU against the families of tests/gapped_fuzz.py: every output array, counter, CIGAR and the TSV bytes equal to the
Python definition (tests/gapped_checker.py) on low-complexity sequence, tandem repeats, duplicated segments, reads of two chunks of seeds and the
edges of targets, seeds and the band (tests/test_gapped_fuzz_cpu.py asserts that each family holds what it is for); 70 000 reads from a pool of 255
different ones, so that a wave of k_gp_trace takes a second, different read, k_gp_cigar strides, and the TSV is written in three chunks.

Measured on an MI355X: the whole file in 14 s, of which the device calls with their read-backs take under 0.1 s and the checker the rest
(`tandem` 3.4 s, `two_letter` 2.1 s, `long_reads` 1.4 s; the 70 000 reads 2.9 s: 0.6 s to build them, 1.9 s the checker, 0.01 s the device call);
every test prints its own figures (-s)."""
import time

import numpy as np
import pytest

import alga_amd
import gapped_checker as GC
import gapped_fuzz as F
import place_checker as P

pytestmark = pytest.mark.gpu


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
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, seed, k, got[k].dtype, got[k].shape, want[k].shape)
        assert (got[k] == want[k]).all(), (what, seed, k, np.nonzero(got[k] != want[k])[0][:10], got[k][got[k] != want[k]][:10], want[k][got[k] != want[k]][:10])
    info = {k: v for k, v in got["info"].items() if not k.startswith("ms_")}
    assert info == want["info"], (what, seed, info, want["info"])


def place(eng, c):
    return eng.place_reads(c["rows"], c["lens"], targets=F.targets(c), **c["place"])


def assert_placed(pl, want, what=""):
    got = pl.to_host()
    for k in P.ARRAYS:
        assert (got[k] == want[k]).all(), (what, k)


def run_family(eng, name, tmp_path):
    c = F.case(name)
    path = str(tmp_path / "g.tsv")
    t0 = time.time()
    wants = [F.checked(name, i) for i in range(len(c["variants"]))]
    t_check, t_dev = time.time() - t0, 0.0
    pl = place(eng, c)
    assert_placed(pl, F.placed(name), name)
    try:
        for i, v in enumerate(c["variants"]):
            want = wants[i]
            for bits in (0, 3):
                eng.set_option("place_dir_bits", bits)
                t0 = time.time()
                gp = eng.place_gapped(c["rows"], c["lens"], pl, targets=F.targets(c), **v)
                got = gp.to_host()
                t_dev += time.time() - t0
                assert_same(got, want, (name, i, "directory bits", bits), F.SEEDS[name])
            assert (gp.n_reads, gp.n_targets, gp.n_columns, gp.n_cigar) == (len(c["lens"]) // 2, len(c["tlen"]), int(c["tlen"].sum()), len(want["cigar"]))
            assert gp.cigar_strings() == gp.cigar_strings(got) == GC.cigar_strings(want)
            info = eng.write_gapped_tsv(path, gp)
            text = open(path, "rb").read()
            assert text == GC.tsv(want), (name, i)
            assert info["segments"] == want["info"]["placed"] and info["bytes"] == len(text)
            assert_placed(pl, F.placed(name), (name, i, "the placement after the call"))
            print(name, i, {k: gp.info[k] for k in ("tried", "placed", "unique", "candidates")})
    finally:
        eng.set_option("place_dir_bits", 0)
    print("%s: the checker %.2f s, the device calls with their read-backs %.2f s" % (name, t_check, t_dev))


@pytest.mark.parametrize("name", sorted(set(F.CASES) - {"pool"}))
def test_family_equals_the_checker(eng, name, tmp_path):
    run_family(eng, name, tmp_path)


def test_the_pool_equals_the_checker(eng, tmp_path):
    """the 255 reads that test_waves_take_a_second_and_a_different_read draws from, once each: a difference there can be read off this one first"""
    run_family(eng, "pool", tmp_path)


def test_waves_take_a_second_and_a_different_read(eng, tmp_path):
    n = 70000
    t0 = time.time()
    c = F.many_different_reads(n)
    t_build = time.time() - t0
    pl = place(eng, c)
    t0 = time.time()
    want = GC.gapped_banded(c["rows"], c["lens"], pl.to_host(), *F.targets(c))
    t_check = time.time() - t0
    t0 = time.time()
    gp = eng.place_gapped(c["rows"], c["lens"], pl, targets=F.targets(c))
    got = gp.to_host()
    t_dev = time.time() - t0
    assert_same(got, want, "70 000 reads", F.SEEDS["pool"])
    info = gp.info
    print({k: v for k, v in info.items() if not k.startswith("ms_")})
    assert info["placed"] > 2 * 8192 + 300                                      # k_gp_trace: at most 8192 blocks of 2 waves
    assert info["tried"] * 31 > 8192 * 256                                       # k_gp_cigar: 31 runs a read, at most 8192 blocks of 256
    on = (got["state"] & GC.PLACED) > 0
    plh = pl.to_host()
    tried = np.array([GC.takes_part(plh, c["lens"], r, GC.DEFAULT["k"]) for r in range(3 * F.POOL)])
    assert any(tried[r] and on[r - 1] and not on[r] and on[r + 1] for r in range(1, 3 * F.POOL - 1))    # a read that is not placed between two that are
    assert any(c["lens"][2 * r + 1] != c["lens"][2 * (r + 16384) + 1] for r in range(64))
    assert gp.cigar_strings(got) == GC.cigar_strings(want)
    path = str(tmp_path / "g.tsv")
    t0 = time.time()
    try:
        eng.set_option("gfa_chunk_mb", 1)
        out = eng.write_gapped_tsv(path, gp)
    finally:
        eng.set_option("gfa_chunk_mb", 256)
    t_tsv = time.time() - t0
    text = open(path, "rb").read()
    assert len(text) > 2 << 20                                                   # more than two chunks of 1 MiB: three
    assert text == GC.tsv(want)
    assert out["segments"] == want["info"]["placed"] and out["bytes"] == len(text)
    print("building the reads %.2f s, the checker %.2f s, the device call with its read-back %.2f s, the TSV %.2f s (%d bytes)" % (t_build, t_check, t_dev, t_tsv, len(text)))
