"""The end of k_pile_probe's tile with its dependent loads batched (alga_amd/csrc/prefsuf_pile.hip; engine option "pile_probe_tail"):

  pile_probe_tail  1: k_pile_probe<true, true> -- the look-ups of a source's one or two standing targets share two round trips (both bucket
                   lines, then the first four candidates of both m_C classes; further batches while a class has more), and the first entry of a
                   further group's bucket is read an iteration ahead of the group's record;
                   0: k_pile_probe<true, false>, load by load.

The option changes when loads are issued and nothing that is decided: every case is built with it off and on, in the pure (pile 2) and the
mixed (pile 3) form, and must equal the pairwise kernels' list and the CPU oracle's, with the same sources handed on.  The inputs are the
smallest at which the new code can go wrong -- classes of fewer and of more entries than a batch, sources with two standing items, buckets
shared by several k-mers, node counts at the edges of a tile, a rank's id range -- and each is shown on the host to be what it is meant to be.
The compiler's resource report of every instantiation the launcher can select is checked without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import alga_amd
import oracle_lib as O
from alga_amd.engine import device_view
from pile_option_common import PP_TAIL_K, PP_TILE, key_shapes, nodes, option_off_and_on, repeats_genome, sorted_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = "pile_probe_tail"
DEFAULTS = {"pile": 1, OPT: 1, "cluster_bucket_bias": 0}
# SGPR spills of k_pile_probe<true> in the compiler's report of the commit before this option (hipcc -O3 --offload-arch=gfx950
# -Rpass-analysis=kernel-resource-usage on prefsuf_pile.hip: 124 VGPRs, no scratch, 112 SGPRs spilled): no instantiation may spill more
PARENT_SGPR_SPILLS = 112
# 150-bp reads at 120x on 60 kb: with the table size the engine picks, 45 of the 3 528 buckets hold two k-mers and four hold more than 64 entries
# (76 the largest); 64 times as many buckets give every k-mer its own -- 47 entries the largest, classes of up to 8
BIAS_120X = 6


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("coverage,seed,bias", [(8, 163, 0), (30, 185, 0), (120, 275, BIAS_120X)])
def test_classes_below_and_above_a_batch(eng, coverage, seed, bias):
    """150-bp reads on a 60 kb genome.  At 8x most m_C >> 3 classes of a bucket are empty or hold one entry, at 30x one or two; at 120x a class
    holds more than a batch takes, so the remainder loop runs -- in buckets of no more than 64 entries, the only ones a look-up reads: that
    input gets 64 times the buckets (BIAS_120X), or the k-mers that share a bucket push four of them past 64."""
    G = 60_000
    words, lens = nodes(G * coverage // 150, 150, G, seed)
    lo, rs = alga_amd.derive_params(144.0)
    keys, shift = sorted_keys(eng, words, lens, lo, rs, {"cluster_bucket_bias": bias}, DEFAULTS)
    bucket_n, class_n, _, _ = key_shapes(keys, shift)
    print("coverage %d: largest bucket %d, largest class %d, classes beyond a batch %d of %d" % (coverage, bucket_n.max(), class_n.max(), int((class_n > PP_TAIL_K).sum()), len(class_n)))
    if coverage == 120:
        assert class_n.max() > PP_TAIL_K and bucket_n.max() <= 64, (class_n.max(), bucket_n.max())
    else:
        assert (class_n <= PP_TAIL_K).any() and (class_n == 1).any()
    _, st = option_off_and_on(eng, words, lens, lo, rs, OPT, DEFAULTS, {"cluster_bucket_bias": bias})
    assert st["deferred_sources"] <= int((lens > 0).sum()) // 10, st       # the look-ups ran: nearly every source finished in k_pile_probe


@pytest.mark.gpu
def test_two_standing_items_in_one_tile(eng):
    """A genome of repeats and a tandem stretch: sources that keep two items, so both look-ups of a lane share the batch."""
    words, lens = nodes(9000, 150, None, 19, genome=repeats_genome(11))
    lo, rs = alga_amd.derive_params(144.0)
    want, _ = option_off_and_on(eng, words, lens, lo, rs, OPT, DEFAULTS)
    out_degree = np.bincount(want[:, 0].astype(np.int64), minlength=len(lens))
    print("sources of out-degree 0, 1, 2, ...: %s" % np.bincount(out_degree).tolist())
    assert (out_degree == 2).sum() > 0, np.bincount(out_degree)


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [-1, -2, -3])
def test_buckets_shared_by_several_kmers(eng, bias):
    """Fewer buckets (option cluster_bucket_bias): buckets of two, three and four k-mer groups, so the loop over the further groups of a
    run's tag runs once and more than once for a lane."""
    words, lens = nodes(6000, 150, 30_000, 311)
    lo, rs = alga_amd.derive_params(144.0)
    keys, shift = sorted_keys(eng, words, lens, lo, rs, {"cluster_bucket_bias": bias}, DEFAULTS)
    bucket_n, _, groups, _ = key_shapes(keys, shift)
    assert len(groups) == len(bucket_n)
    small = bucket_n <= 64
    print("bias %d: buckets of 1 / 2 / 3 / 4 / more groups: %s" % (bias, [int(((groups == g) & small).sum()) for g in (1, 2, 3, 4)] + [int((groups > 4).sum())]))
    assert ((groups == 2) & small).sum() > 0 and (((groups == 3) | (groups == 4)) & small).sum() > 0
    option_off_and_on(eng, words, lens, lo, rs, OPT, DEFAULTS, {"cluster_bucket_bias": bias})


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes", [PP_TILE - 2, PP_TILE, PP_TILE + 2, 2 * PP_TILE + 2])
def test_node_counts_at_the_edges_of_a_tile(eng, n_nodes):
    """Fewer sources than a tile of 256, exactly one tile, and a last tile of two lanes (a node set holds a read and its twin: even counts;
    the one-lane last tile is an id range of the next test)."""
    words, lens = nodes(n_nodes, 150, 1500, 400 + n_nodes)                  # (duplicate reads are dropped: twice as many sampled, the first n_nodes nodes kept)
    assert len(lens) >= n_nodes
    words, lens = np.ascontiguousarray(words[:n_nodes]), np.ascontiguousarray(lens[:n_nodes])
    lo, rs = alga_amd.derive_params(144.0)
    option_off_and_on(eng, words, lens, lo, rs, OPT, DEFAULTS)


@pytest.mark.gpu
def test_a_rank_s_id_range_and_a_one_lane_last_tile(eng):
    """k_pile_probe over the side records of an id range (k_pile_side_range), with the option on and off: ranges of one source less than a tile,
    a tile, a tile and one lane, two tiles and one lane, and a rank's share, each equal to the oracle's edges of its sources."""
    words, lens = nodes(4000, 150, 20_000, 41)
    lo, rs = alga_amd.derive_params(144.0)
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    dw = torch.from_numpy(words.view(np.int32)).cuda()
    dl = torch.from_numpy(lens.astype(np.int32)).cuda()
    n = len(lens)
    ranges = [(0, PP_TILE - 1), (0, PP_TILE), (0, PP_TILE + 1), (5, 5 + 2 * PP_TILE + 1), (n // 3, n // 2 + 1), (1, n - 1)]
    eng.set_option("pile", 2)
    try:
        for a, b in ranges:
            sel = want[(want[:, 0] >= a) & (want[:, 0] < b)]
            deferred = {}
            for v in (0, 1):
                eng.set_option(OPT, v)
                ptr, m = eng.build_range_device(dw, dl, lo, rs, a, b)
                st = eng.last_stats()
                got = device_view(ptr, (m, 3), dw.device).cpu().numpy()
                assert got.shape == sel.shape and (got == sel).all(), (a, b, v)
                assert st["ms_pile"] > 0, (a, b, v)
                deferred[v] = st["deferred_sources"]
            assert deferred[0] == deferred[1], (a, b, deferred)
    finally:
        eng.set_option("pile", DEFAULTS["pile"])
        eng.set_option(OPT, DEFAULTS[OPT])


def test_every_probe_instantiation_keeps_the_budget():
    """The compiler's resource report for the forms of k_pile_probe the launcher selects -- <lean, tail> = <0, 0>, <1, 0>, <1, 1>: four waves
    per SIMD, no scratch, no VGPR spill, no more SGPR spills than the lean kernel had before the tail option, LDS for four blocks per CU."""
    src = os.path.join(ROOT, "alga_amd", "csrc", "prefsuf_pile.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_pile_probe_tail_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    finally:
        if os.path.exists(out):
            os.remove(out)
    lines = r.stderr.splitlines()
    reps = {}
    for i, s in enumerate(lines):
        m = re.search(r"Function Name: _ZN4alga12k_pile_probeILb([01])ELb([01])EE", s)
        if not m:
            continue
        rep = {}
        for t in lines[i + 1:]:
            if "Function Name:" in t:
                break
            mm = re.search(r"remark:\s+(.+?):\s+(\S+)\s+\[-Rpass", t)
            if mm:
                rep[mm.group(1)] = mm.group(2)
        reps[(int(m.group(1)), int(m.group(2)))] = rep
    assert set(reps) == {(0, 0), (1, 0), (1, 1)}, sorted(reps)
    for form, rep in reps.items():
        assert int(rep["Occupancy [waves/SIMD]"]) == 4, (form, rep)
        assert int(rep["ScratchSize [bytes/lane]"]) == 0 and int(rep["VGPRs Spill"]) == 0, (form, rep)
        assert int(rep["SGPRs Spill"]) <= PARENT_SGPR_SPILLS, (form, rep)
        assert int(rep["LDS Size [bytes/block]"]) <= 40960, (form, rep)
