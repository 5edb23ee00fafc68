"""The two forms of k_pile_probe (alga_amd/csrc/prefsuf_pile.hip; engine option "pile_probe_lean"):

  pile_probe_lean  1: k_pile_probe<true> takes a source's row from its home run in slot 0 only and looks for the last mismatch of a record
                   below position 64 only (a mismatch from 64 on clears the whole offset set);
                   0: k_pile_probe<false>, the round-5 kernel.

The option may only change how a graph is computed: every case is built with it off and on, in the pure (pile 1) and mixed (pile 3) forms and
for a rank's id range, and the edge lists must be identical -- and equal to the CPU oracle's -- with no more sources handed to the general
kernel.  The compiler's resource report of both instantiations is checked without a GPU."""
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
OPT = "pile_probe_lean"


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


# the inputs of tests/test_gpu_pile.py: lengths and coverages, the reduction gaps, duplicate reads, repeats and tandems (further groups of a
# bucket, members that differ from the consensus, the same minimizer twice)
CASES = [("len%d_cov%d" % (length, cov), (lambda length=length, cov=cov: _nodes(60_000 * cov // length, length, 60_000, 5 + length + cov)), float(length - 6), None)
         for length, cov in ((150, 30), (150, 8), (100, 40), (126, 25), (150, 120))]
CASES += [("gap_rs%d" % rs, (lambda: _nodes(9000, 150, 40_000, 77)), 144.0, rs) for rs in (82, 116, 140, 144, 145)]
CASES += [("duplicates", _duplicates, 144.0, None),
          ("repeats_tandems", (lambda: _nodes(9000, 150, None, 19, genome=_repeats_genome(11))), 144.0, None)]


def _build(eng, words, lens, lo, rs, pile, lean):
    eng.set_option("pile", pile)
    eng.set_option(OPT, lean)
    try:
        got = eng.prefsuf_host(words, lens, lo, rs, reduction="source_side")
    finally:
        eng.set_option("pile", 1)
        eng.set_option(OPT, 1)
    return got, eng.last_stats()


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,mean_len,rs", CASES, ids=[c[0] for c in CASES])
def test_lean_probe_gives_the_same_graph(eng, name, make, mean_len, rs):
    words, lens = make()
    lo, rs0 = alga_amd.derive_params(mean_len)
    rs = rs0 if rs is None else rs
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    for pile in (1, 3):
        st = {}
        for v in (0, 1):
            got, st[v] = _build(eng, words, lens, lo, rs, pile, v)
            assert got.shape == want.shape and (got == want).all(), (name, pile, v, got.shape, want.shape)
        assert st[1]["ms_pile"] > 0 and st[0]["ms_pile"] > 0, (name, pile)
        assert st[1]["deferred_sources"] <= st[0]["deferred_sources"], (name, pile, st[0]["deferred_sources"], st[1]["deferred_sources"])
        assert st[1]["pile_deferred"] <= st[0]["pile_deferred"], (name, pile)


@pytest.mark.gpu
@pytest.mark.parametrize("pile", [1, 3])
def test_lean_probe_for_a_rank_s_id_range(eng, pile):
    """k_pile_probe over the side records of an id range (k_pile_side_range): each range equals the oracle's edges of its sources in both forms."""
    lo, rs = alga_amd.derive_params(144.0)
    rng = np.random.default_rng(5)
    unit = rng.integers(0, 4, 3000, dtype=np.uint8)
    genome = np.concatenate([rng.integers(0, 4, 60_000, dtype=np.uint8), unit, rng.integers(0, 4, 20_000, dtype=np.uint8), unit, rng.integers(0, 4, 30_000, dtype=np.uint8)])
    for words, lens in (_nodes(20_000, 150, 100_000, 41), _nodes(24_000, 150, 0, 42, genome=genome)):
        want, _, _ = O.prefsuf(words, lens, lo, rs)
        dw = torch.from_numpy(words.view(np.int32)).cuda()
        dl = torch.from_numpy(lens.astype(np.int32)).cuda()
        n = len(lens)
        ranges = [(0, n // 3), (n // 3, n // 2 + 1), (n // 2 + 1, n), (n // 2, n // 2 + 2), (1, n - 1)]
        eng.set_option("pile", pile)
        try:
            for a, b in ranges:
                sel = want[(want[:, 0] >= a) & (want[:, 0] < b)]
                deferred = {}
                for v in (0, 1):
                    eng.set_option(OPT, v)
                    ptr, m = eng.build_range_device(dw, dl, lo, rs, a, b)
                    st = eng.last_stats()
                    got = device_view(ptr, (m, 3), dw.device).cpu().numpy()
                    assert got.shape == sel.shape and (got == sel).all(), (pile, a, b, v)
                    assert st["ms_pile"] > 0, (pile, a, b, v)
                    deferred[v] = st["deferred_sources"]
                assert deferred[1] <= deferred[0], (pile, a, b, deferred)
        finally:
            eng.set_option("pile", 1)
            eng.set_option(OPT, 1)


@pytest.mark.gpu
def test_lean_probe_at_a_few_million_reads(eng):
    """A resident node set of two million 150-bp reads (30x): option off and on give the same graph, edge for edge, and hand on no more sources."""
    wl = workload.device_build(2_000_000, 150, 10_000_000, 11)
    torch.cuda.synchronize()
    dw, dl, lo, rs = wl["words"], wl["lens"], wl["min_overlap"], wl["rsoemo"]
    try:
        eng.set_option(OPT, 0)
        ptr, m = eng.prefsuf_device(dw, dl, lo, rs)
        st0 = eng.last_stats()
        want = device_view(ptr, (m, 3), dw.device).clone()
        eng.set_option(OPT, 1)
        ptr, m = eng.prefsuf_device(dw, dl, lo, rs)
        st1 = eng.last_stats()
        got = device_view(ptr, (m, 3), dw.device)
        assert got.shape == want.shape and bool(torch.equal(got, want))
        assert st0["ms_pile"] > 0 and st1["ms_pile"] > 0
        assert st1["deferred_sources"] <= st0["deferred_sources"], (st0["deferred_sources"], st1["deferred_sources"])
    finally:
        eng.set_option(OPT, 1)


def _resource_report():
    src = os.path.join(ROOT, "alga_amd", "csrc", "prefsuf_pile.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_pile_probe_occupancy_%d.o" % os.getpid())
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
        m = re.search(r"Function Name: (_ZN4alga12k_pile_probeILb([01])E\S*)", s)
        if not m:
            continue
        rep = {}
        for t in lines[i + 1:]:
            if "Function Name:" in t:
                break
            mm = re.search(r"remark:\s+(.+?):\s+(\S+)\s+\[-Rpass", t)
            if mm:
                rep[mm.group(1)] = mm.group(2)
        reps[m.group(2) == "1"] = rep
    return reps


def test_probe_kernel_resources():
    """The compiler's resource report for both forms of k_pile_probe: at least four waves per SIMD, no VGPR spill, no scratch, LDS within
    what lets four 256-thread blocks share a CU."""
    reps = _resource_report()
    assert set(reps) == {False, True}, "k_pile_probe<false> / <true> not in the report"
    for lean, rep in reps.items():
        assert int(rep["Occupancy [waves/SIMD]"]) >= 4, (lean, rep)
        assert int(rep["VGPRs"]) <= 128, (lean, rep)
        assert int(rep["VGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, (lean, rep)
        assert int(rep["LDS Size [bytes/block]"]) <= 40960, (lean, rep)
