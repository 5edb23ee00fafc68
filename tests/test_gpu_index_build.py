"""GPU parity of the index-build options of the pile path (alga_amd/csrc/prefsuf_pile.hip, prefsuf_kernels.hip):

  pile_runs_list  1: k_pile_build lists its piles per workgroup and k_pile_runs_consensus_list makes their run lists at four waves per SIMD;
                  0: k_pile_runs_consensus sweeps the side records for the piles (round 5).
  pile_deg_fold   1: the first pass of the out-degree scan moves the out-degrees k_pile_probe left in the slots; 0: k_pile_deg does, as a pass of its own.

Either setting may only change how a graph is computed: every case is built with the option off and on, in the pure pile form (pile 1), the
mixed form (pile 3) and through the pairwise kernels (pile 0), and the edge lists must be identical -- and equal to the CPU oracle's."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import alga_amd
import gen_reads
import oracle_lib as O
from alga_amd import workload
from alga_amd.engine import device_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = ("pile_runs_list", "pile_deg_fold")


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def _nodes(n, length, G, seed, err=0.0, genome=None):
    if genome is None:
        codes, _ = gen_reads.sample_reads(n, length, G, seed, err)
    else:
        rng = np.random.default_rng(seed)
        starts = rng.integers(0, len(genome) - length + 1, size=n)
        codes = np.stack([genome[s:s + length] for s in starts]).astype(np.uint8)
        flip = rng.random(n) < 0.5
        codes[flip] = (3 - codes[flip])[:, ::-1]
    words, lens, _ = workload.make_nodes(codes)
    return words, lens


def _repeats_genome(seed):
    rng = np.random.default_rng(seed)
    unit = rng.integers(0, 4, size=700).astype(np.uint8)
    parts = []
    for k in range(12):
        u = unit.copy()
        pos = rng.integers(0, len(u), size=3)
        u[pos] = (u[pos] + 1 + rng.integers(0, 3, size=3)) % 4
        parts.append(u)
        parts.append(rng.integers(0, 4, size=300).astype(np.uint8))
    motif = rng.integers(0, 4, size=37).astype(np.uint8)
    parts.append(np.tile(motif, 30))
    return np.concatenate(parts)


def _duplicates():
    codes, _ = gen_reads.sample_reads(6000, 150, 30_000, 3)
    codes = np.concatenate([codes, codes[:1500], codes[100:400]])
    fw = alga_amd.pack_reads(np.ascontiguousarray(codes[:, 3:147]))
    rv = alga_amd.pack_reads(np.ascontiguousarray((3 - codes[:, 3:147])[:, ::-1]))
    words = np.empty((2 * len(codes), fw.shape[1]), dtype=np.uint32)
    words[0::2], words[1::2] = fw, rv
    return words, np.full(2 * len(codes), 144, dtype=np.int32)


# the inputs of tests/test_gpu_pile.py: the shapes the pile path takes, the reduction gaps, duplicate reads, repeats and tandems, reads with errors
CASES = [("len%d_cov%d" % (length, cov), (lambda length=length, cov=cov: _nodes(60_000 * cov // length, length, 60_000, 5 + length + cov)), float(length - 6), None)
         for length, cov in ((150, 30), (150, 8), (100, 40), (126, 25), (150, 120))]
CASES += [("gap_rs%d" % rs, (lambda: _nodes(9000, 150, 40_000, 77)), 144.0, rs) for rs in (82, 116, 140, 144, 145)]
CASES += [("duplicates", _duplicates, 144.0, None),
          ("repeats_tandems", (lambda: _nodes(9000, 150, None, 19, genome=_repeats_genome(11))), 144.0, None),
          ("errors", (lambda: _nodes(10_000, 150, 40_000, 61, err=0.02)), 144.0, None)]


DEFAULTS = {"pile": 1, "pile_runs_list": 1, "pile_deg_fold": 1, "pile_check": 0}


def _build(eng, words, lens, lo, rs, settings):
    for k, v in settings.items():
        eng.set_option(k, v)
    try:
        got = eng.prefsuf_host(words, lens, lo, rs, reduction="source_side")
    finally:
        for k in settings:
            eng.set_option(k, DEFAULTS[k])
    return got, eng.last_stats()


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,mean_len,rs", CASES, ids=[c[0] for c in CASES])
def test_options_off_and_on_give_the_same_graph(eng, name, make, mean_len, rs):
    words, lens = make()
    lo, rs0 = alga_amd.derive_params(mean_len)
    rs = rs0 if rs is None else rs
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    for pile in (1, 3, 0):
        for opt in OPTIONS:
            base = None
            for v in (0, 1):
                got, st = _build(eng, words, lens, lo, rs, {"pile": pile, opt: v})
                assert got.shape == want.shape and (got == want).all(), (name, pile, opt, v, got.shape, want.shape)
                if base is None:
                    base = got
                assert np.array_equal(got, base), (name, pile, opt)
            if pile == 0:
                assert st["ms_pile"] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("length,coverage,G", [(150, 30, 400_000), (100, 40, 200_000), (132, 25, 200_000)])
def test_run_list_harness_with_the_list_driven_kernel(eng, length, coverage, G):
    """pile_check (every first-group member's own run list against its pile's, clipped to its windows) over the lists of
    k_pile_runs_consensus_list, and over the tile sweep's: not one may differ, and both check the same members."""
    words, lens = _nodes(G * coverage // length, length, G, 900 + length + coverage)
    lo, rs = alga_amd.derive_params(float(length - 6))
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    checked = {}
    for v in (1, 0):
        got, st = _build(eng, words, lens, lo, rs, {"pile_check": 1, "pile_runs_list": v})
        assert got.shape == want.shape and (got == want).all()
        assert st["pile_list_checked"] > int((lens > 0).sum()) // 2, st
        assert st["pile_list_mismatch"] == 0, st
        checked[v] = st["pile_list_checked"]
    assert checked[0] == checked[1]


@pytest.mark.gpu
def test_options_off_and_on_at_a_few_million_reads(eng):
    """A resident node set of two million 150-bp reads (30x): the graph of every setting equals the defaults', edge for edge."""
    wl = workload.device_build(2_000_000, 150, 10_000_000, 11)
    torch.cuda.synchronize()
    dw, dl, lo, rs = wl["words"], wl["lens"], wl["min_overlap"], wl["rsoemo"]
    ptr, m = eng.prefsuf_device(dw, dl, lo, rs)
    want = device_view(ptr, (m, 3), dw.device).clone()
    st = eng.last_stats()
    assert st["ms_pile"] > 0 and m > 0
    for pile in (1, 3, 0):
        for opt in OPTIONS:
            for v in (0, 1):
                eng.set_option("pile", pile)
                eng.set_option(opt, v)
                try:
                    ptr, m = eng.prefsuf_device(dw, dl, lo, rs)
                    got = device_view(ptr, (m, 3), dw.device)
                    assert got.shape == want.shape and bool(torch.equal(got, want)), (pile, opt, v)
                finally:
                    eng.set_option("pile", 1)
                    eng.set_option(opt, 1)


def test_list_driven_consensus_kernel_runs_at_four_waves_per_simd():
    """The compiler's resource report for k_pile_runs_consensus_list: at least four waves per SIMD, no VGPR or SGPR spill, no scratch."""
    src = os.path.join(ROOT, "alga_amd", "csrc", "prefsuf_pile.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_pile_occupancy_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    finally:
        if os.path.exists(out):
            os.remove(out)
    lines = r.stderr.splitlines()
    at = [i for i, s in enumerate(lines) if "Function Name:" in s and "k_pile_runs_consensus_list" in s]
    assert len(at) == 1, "k_pile_runs_consensus_list not in the report"
    rep = {}
    for s in lines[at[0] + 1:]:
        if "Function Name:" in s:
            break
        m = re.search(r"remark:\s+(.+?):\s+(\S+)\s+\[-Rpass", s)
        if m:
            rep[m.group(1)] = m.group(2)
    assert int(rep["Occupancy [waves/SIMD]"]) >= 4, rep
    assert int(rep["VGPRs Spill"]) == 0 and int(rep["SGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, rep
    assert int(rep["LDS Size [bytes/block]"]) <= 20480, rep
