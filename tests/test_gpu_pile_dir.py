"""Engine option pile_dir (alga_amd/csrc/prefsuf_pile.hip, prefsuf_cluster.hip, engine.hip): where the pile path takes a bucket's record from.

  0  k_pile_build reads the bucket directory k_tgt_dir made (until round 7);
  1  k_pile_build takes bucket starts, counts of at most 64 and the class offsets from the sorted keys of its tile and never reads the directory;
  2  ... and a build of the pure pile form neither fills nor builds the directory: the pairwise kernels behind the pile kernels read the
     bucket records from the piles' table.

The value may only change how a graph is computed: every input is built with all three values in the pure form (pile 1), the forced mixed
form (pile 3), through the pairwise kernels (pile 0) and in the forced pure form (pile 2); the edge lists must be identical and equal to the
CPU oracle's, and the counters of the pile path must agree.  The inputs are the smallest that reach the places where a directory derived from the keys can go wrong; that they
do is asserted from the host, on the sorted keys."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import alga_amd
import oracle_lib as O
from alga_amd.engine import device_view
from test_gpu_index_build import _duplicates, _nodes, _repeats_genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PB_TILE, PB_HALO = 192, 64                                 # prefsuf_pile.hip
VALUES = (0, 1, 2)
DEFAULTS = {"pile": 1, "pile_dir": 2, "pile_check": 0, "cluster_bucket_bias": 0, "test_unsorted_index": 0}
COUNTERS = ("pile_buckets", "pile_irregular", "pile_own_lists", "deferred_sources", "edges")
BIAS_SEED = 5                                              # a seed for which the lowered-bias inputs hold every bucket shape (asserted below)
BIASES = (-4, -6, -8)


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def _tile_multiple():
    """Exactly PB_TILE * k live nodes: the last tile of the key order is full and nothing follows it."""
    words, lens = _nodes(PB_TILE * 5, 150, 6000, 31)       # (a read and its reverse complement are two nodes; equal reads are one)
    m = len(lens) // PB_TILE * PB_TILE                     # even: whole twin pairs
    words, lens = np.ascontiguousarray(words[:m]), np.ascontiguousarray(lens[:m])
    assert m >= 4 * PB_TILE and (lens > 0).all()
    return words, lens


# name, maker, mean length, cluster_bucket_bias
CASES = [("len150_cov30", (lambda: _nodes(12_000, 150, 60_000, BIAS_SEED)), 144.0, 0),
         ("len100_cov40", (lambda: _nodes(60_000 * 40 // 100, 100, 60_000, 5 + 100 + 40)), 94.0, 0)]
CASES += [("bias%d" % b, (lambda: _nodes(12_000, 150, 60_000, BIAS_SEED)), 144.0, b) for b in BIASES]
CASES += [("duplicates", _duplicates, 144.0, 0),
          ("repeats_tandems", (lambda: _nodes(9000, 150, None, 19, genome=_repeats_genome(11))), 144.0, 0),
          ("one_tile_not_full", (lambda: _nodes(50, 150, 400, 7)), 144.0, 0),
          ("tile_multiple", _tile_multiple, 144.0, 0),
          ("errors", (lambda: _nodes(10_000, 150, 40_000, 61, err=0.02)), 144.0, 0)]

_ORACLE = {}


def _case(name):
    """The input of a case and the oracle's edges: computed once, shared by the tests, never written to."""
    if name not in _ORACLE:
        _, make, mean_len, bias = next(c for c in CASES if c[0] == name)
        words, lens = make()
        lo, rs = alga_amd.derive_params(mean_len)
        want, _, _ = O.prefsuf(words, lens, lo, rs)
        want.setflags(write=False)
        _ORACLE[name] = (words, lens, lo, rs, want, bias)
    return _ORACLE[name]


def _build(eng, words, lens, lo, rs, settings):
    for k, v in settings.items():
        eng.set_option(k, v)
    try:
        got = eng.prefsuf_host(words, lens, lo, rs, reduction="source_side")
        st = eng.last_stats()
    finally:
        for k in settings:
            eng.set_option(k, DEFAULTS[k])
    return got, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_every_value_gives_the_same_graph_and_counters(eng, name):
    words, lens, lo, rs, want, bias = _case(name)
    for pile in (1, 3, 0, 2):                              # (2: the pure form forced -- with value 2 the pairwise kernels then read every bucket's record, the long buckets' too, from the piles' table)
        # (how the key pass of a build is laid out follows the verdict on the build before it -- pile_own_lists counts what that layout lists: every
        #  compared build comes behind one of the same form)
        _build(eng, words, lens, lo, rs, {"pile": pile, "pile_dir": 0, "cluster_bucket_bias": bias})
        stats = {}
        for v in VALUES:
            got, st = _build(eng, words, lens, lo, rs, {"pile": pile, "pile_dir": v, "cluster_bucket_bias": bias})
            assert got.shape == want.shape and (got == want).all(), (name, pile, v, got.shape, want.shape)
            stats[v] = {k: st[k] for k in COUNTERS}
        assert stats[0] == stats[1] == stats[2], (name, pile, stats)
        if pile == 0:
            assert st["ms_pile"] == 0.0
    if name == "errors":                                   # the sample declines: value 2 builds the directory, the pairwise kernels work
        got, st = _build(eng, words, lens, lo, rs, {"pile_dir": 2})
        assert st["pile_irregular"] * alga_amd.engine.PILE_DECLINE_ONE_IN > st["pile_buckets"] > 0
    for v in VALUES:
        got, st = _build(eng, words, lens, lo, rs, {"pile_check": 1, "pile_dir": v, "cluster_bucket_bias": bias})
        assert got.shape == want.shape and (got == want).all(), (name, v)
        assert st["pile_list_mismatch"] == 0, (name, v, st)


@pytest.mark.gpu
def test_the_lowered_bias_inputs_hold_every_bucket_shape(eng):
    """From the host, on the sorted keys of alga_prefsuf_keys_device: the inputs with a lowered cluster_bucket_bias hold a bucket of exactly 64
    entries and one of exactly 65 (the two sides of "part"), buckets that straddle a tile boundary, buckets whose first entry is the last
    thread of the tile proper, and buckets longer than tile plus halo."""
    words, lens, lo, rs, _, _ = _case("bias%d" % BIASES[0])
    dw = torch.from_numpy(words.view(np.int32)).cuda()
    dl = torch.from_numpy(lens.astype(np.int32)).cuda()
    n = len(lens)
    seen = set()
    for bias in BIASES:
        eng.set_option("cluster_bucket_bias", bias)
        try:
            _, st = _build(eng, words, lens, lo, rs, {})
            k = eng.keys_device(dw, dl, lo, rs, 0, n)
            assert k is not None
            keys = device_view(k[0], (n,), dw.device).cpu().numpy().view(np.uint32).astype(np.uint64)
        finally:
            eng.set_option("cluster_bucket_bias", 0)
        n_buckets = int(st["table_slots"])
        assert n_buckets & (n_buckets - 1) == 0
        shift = 32 - (n_buckets.bit_length() - 1)
        bucket = np.sort(np.where(keys == 0xFFFFFFFF, n_buckets, keys >> np.uint64(shift)))      # the key order, as far as the buckets go
        first = np.flatnonzero(np.r_[True, bucket[1:] != bucket[:-1]])
        count = np.diff(np.r_[first, len(bucket)])
        real = bucket[first] != n_buckets
        first, count = first[real], count[real]
        if (count == 64).any():
            seen.add("exactly 64")
        if (count == 65).any():
            seen.add("exactly 65")
        if (first // PB_TILE != (first + count - 1) // PB_TILE).any():
            seen.add("straddles a tile boundary")
        if (first % PB_TILE == PB_TILE - 1).any():
            seen.add("starts at thread PB_TILE - 1")
        if (count > PB_TILE + PB_HALO).any():
            seen.add("longer than tile plus halo")
    assert seen == {"exactly 64", "exactly 65", "straddles a tile boundary", "starts at thread PB_TILE - 1", "longer than tile plus halo"}, seen


@pytest.mark.gpu
def test_a_further_piece_after_a_pure_and_after_a_declined_build(eng):
    """keys_shared = 2 behind a build with pile_dir = 2: a pure build left no directory and serves the next piece from its piles' table, a declined
    one (reads with errors) built the directory and serves it from there."""
    lo, rs = alga_amd.derive_params(144.0)
    for err, kept in ((0.0, True), (0.02, False)):
        words, lens = _nodes(12_000, 150, 40_000, 23, err=err)
        want, _, _ = O.prefsuf(words, lens, lo, rs)
        dw = torch.from_numpy(words.view(np.int32)).cuda()
        dl = torch.from_numpy(lens.astype(np.int32)).cuda()
        n = len(lens)
        half = (n // 4) * 2
        for v in VALUES:
            eng.set_option("pile_dir", v)
            try:
                ptr, m = eng.build_range_device(dw, dl, lo, rs, 0, n)
                st = eng.last_stats()
                assert (st["pile_irregular"] * alga_amd.engine.PILE_DECLINE_ONE_IN <= st["pile_buckets"]) == kept and st["pile_buckets"] > 0
                full = device_view(ptr, (m, 3), dw.device).cpu().numpy()
                assert full.shape == want.shape and (full == want).all(), (err, v)
                for a, b in ((0, half), (half, n), (half - 6, half + 10)):
                    ptr, m = eng.build_range_device(dw, dl, lo, rs, a, b, keys_shared=2)
                    got = device_view(ptr, (m, 3), dw.device).cpu().numpy()
                    sel = want[(want[:, 0] >= a) & (want[:, 0] < b)]
                    assert got.shape == sel.shape and (got == sel).all(), (err, v, a, b)
            finally:
                eng.set_option("pile_dir", DEFAULTS["pile_dir"])


@pytest.mark.gpu
def test_unsorted_index_fails_closed_without_a_directory_pass():
    """pile_dir = 2 on an input of the pure form: k_tgt_dir leaves at once, so k_pile_build carries its order check -- an index over UNSORTED keys
    (test-only option) fails the build with the directory error instead of faulting, and the same engine then builds the right graph."""
    words, lens, lo, rs, want, _ = _case("len150_cov30")
    e = alga_amd.Engine(0)
    try:
        e.set_option("pile_dir", 2)
        got = e.prefsuf_host(words, lens, lo, rs, reduction="source_side")
        st = e.last_stats()
        assert (got == want).all() and st["pile_irregular"] * alga_amd.engine.PILE_IRREGULAR_ONE_IN <= st["pile_buckets"] and st["pile_buckets"] > 0       # the pure form
        e.set_option("test_unsorted_index", 1)
        with pytest.raises(alga_amd.AlgaError) as ei:
            e.prefsuf_host(words, lens, lo, rs, reduction="source_side")
        assert ei.value.code == -3 and "not in order" in str(ei.value)
        e.set_option("test_unsorted_index", 0)
        got = e.prefsuf_host(words, lens, lo, rs, reduction="source_side")
        assert got.shape == want.shape and (got == want).all()
        assert e.last_stats()["pile_buckets"] > 0
    finally:
        e.close()


def test_k_pile_build_keeps_its_resources():
    """The compiler's resource report for k_pile_build, sample and build, with the bucket records from the directory and from the keys: no scratch, no
    VGPR or SGPR spill, and an occupancy not below the one the report gave before the keys-derived form existed (7 waves per SIMD for both
    k_pile_build<true> and k_pile_build<false>, 22 800 bytes of LDS per block: seven blocks of four waves per CU)."""
    src = os.path.join(ROOT, "alga_amd", "csrc", "prefsuf_pile.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_pile_dir_report_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    finally:
        if os.path.exists(out):
            os.remove(out)
    lines = r.stderr.splitlines()
    at = [i for i, s in enumerate(lines) if "Function Name:" in s and "k_pile_build" in s]
    assert len(at) == 4, "k_pile_build<sample | build, directory | keys>: four instances expected in the report"
    for a in at:
        rep = {}
        for s in lines[a + 1:]:
            if "Function Name:" in s:
                break
            m = re.search(r"remark:\s+(.+?):\s+(\S+)\s+\[-Rpass", s)
            if m:
                rep[m.group(1)] = m.group(2)
        assert int(rep["Occupancy [waves/SIMD]"]) >= 7, (lines[a], rep)
        assert int(rep["VGPRs Spill"]) == 0 and int(rep["SGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, (lines[a], rep)
