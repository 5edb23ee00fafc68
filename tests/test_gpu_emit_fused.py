"""Engine option emit_fused (alga_amd/csrc/prefsuf_kernels.hip, engine.hip): how the source-side emit turns out-degrees and slots into rows.

  0  the scan of deg[] first (its first pass moves the out-degrees k_pile_probe left in the slots), k_local_emit_first behind it (until round 8);
  1  two passes over deg[] and first[]: k_emit_tile_sums sums the out-degrees of every tile of EMIT_TILE sources, k_scan_spine_serial scans the
     sums, k_emit_scan_tiles forms the prefix inside the tile and writes row pointers and slot edges from it.  Nothing is moved to deg[].

The value may only change how a graph is computed: every input is built with both values in the pure pile form (pile 1), the forced mixed
form (pile 3), through the pairwise kernels (pile 0) and in the forced pure form (pile 2), with pile_deg_fold 1 and 0; the edge lists must be
identical and equal to the CPU oracle's.  The inputs are the smallest that reach the places where a tiled prefix can go wrong: one partial
tile, a last tile that is full, a tail tile of two sources, every out-degree class on both sides of a tile border (asserted from the host),
rows filled from records, a build the sample declines behind one it kept, a source range that begins inside a tile, and more tiles than
the spine's block has threads."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import alga_amd
import oracle_lib as O
from alga_amd import workload
from alga_amd.engine import device_view
from test_gpu_index_build import _duplicates, _nodes, _repeats_genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMIT_TILE = 4096                                           # SCAN_TILE of prefsuf_kernels.hip: sources per workgroup of both passes
SPINE_THREADS = 1024                                       # k_scan_spine_serial
DEFAULTS = {"pile": 1, "pile_deg_fold": 1, "emit_fused": 1}


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def _trimmed(extra):
    """Whole twin pairs, exactly two tiles of them plus `extra` sources."""
    words, lens = _nodes(4800, 150, 24_000, 31)
    m = 2 * EMIT_TILE + extra
    assert len(lens) >= m and m % 2 == 0
    words, lens = np.ascontiguousarray(words[:m]), np.ascontiguousarray(lens[:m])
    assert (lens > 0).all()
    return words, lens


BORDER_CLASSES = (0, 1, 2, 3)                              # out-degree 0, 1, 2 and >= 3


def _tile_borders():
    """A 30x read set of five tiles and a part: four random contigs (eight dead ends) and the repeats of _repeats_genome (sources with three and
    more edges).  Which read sits next to a tile border is a matter of the node order alone: twin pairs found on the CPU, from the oracle's
    edges of the set as sampled, are swapped into the pairs on both sides of four borders, so that the last sources of the tiles and the
    first sources of the next ones each hold every out-degree class.  (Sampling seeds until the classes fall there by chance would need
    thousands of sets: a few sources in twenty thousand have no edge.)  The test asserts the classes on the oracle's edges of the set as built."""
    rng = np.random.default_rng(23)
    codes = []
    for g in [rng.integers(0, 4, size=11_000).astype(np.uint8) for _ in range(4)] + [_repeats_genome(11)]:
        starts = rng.integers(0, len(g) - 150 + 1, size=len(g) * 30 // 150)
        c = np.stack([g[s:s + 150] for s in starts]).astype(np.uint8)
        flip = rng.random(len(c)) < 0.5
        c[flip] = (3 - c[flip])[:, ::-1]
        codes.append(c)
    words, lens, _ = workload.make_nodes(np.concatenate(codes))
    n = len(lens)
    assert n > 4 * EMIT_TILE + 2 and (lens > 0).all()
    lo, rs = alga_amd.derive_params(144.0)
    edges, _, _ = O.prefsuf(words, lens, lo, rs)
    cls = np.minimum(np.bincount(edges[:, 0], minlength=n), 3)
    # (pair, node of the pair, class): the odd node of the pair in front of border j, the even node of the pair behind it
    places = [(t // 2 - 1, 1, j) for j, t in enumerate(range(EMIT_TILE, 5 * EMIT_TILE, EMIT_TILE))]
    places += [(t // 2, 0, (j + 1) % 4) for j, t in enumerate(range(EMIT_TILE, 5 * EMIT_TILE, EMIT_TILE))]
    perm = np.arange(n // 2)
    used = {slot for slot, _, _ in places}
    for slot, side, c in places:
        p = next(int(p) for p in np.flatnonzero(cls[side::2] == c) if int(p) not in used)
        used.add(p)
        perm[slot], perm[p] = perm[p], perm[slot]
    order = np.stack([2 * perm, 2 * perm + 1], axis=1).ravel()
    return np.ascontiguousarray(words[order]), np.ascontiguousarray(lens[order])


# name, maker
CASES = [("one_partial_tile", (lambda: _nodes(50, 150, 400, 7))),
         ("two_full_tiles", (lambda: _trimmed(0))),
         ("two_tiles_and_two_sources", (lambda: _trimmed(2))),
         ("tile_borders", _tile_borders),
         ("repeats_tandems", (lambda: _nodes(9000, 150, None, 19, genome=_repeats_genome(11)))),
         ("duplicates", _duplicates)]

_ORACLE = {}


def _case(name):
    """The input of a case and the oracle's edges: computed once, shared by the tests, never written to."""
    if name not in _ORACLE:
        make = next(c[1] for c in CASES if c[0] == name)
        words, lens = make()
        lo, rs = alga_amd.derive_params(144.0)
        want, _, _ = O.prefsuf(words, lens, lo, rs)
        want.setflags(write=False)
        _ORACLE[name] = (words, lens, lo, rs, want)
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
def test_both_values_give_the_oracle_s_graph_in_every_form(eng, name):
    words, lens, lo, rs, want = _case(name)
    n = len(lens)
    if name == "one_partial_tile":
        assert 0 < n < EMIT_TILE
    if name == "two_full_tiles":
        assert n == 2 * EMIT_TILE
    if name == "two_tiles_and_two_sources":
        assert n == 2 * EMIT_TILE + 2
    deg = np.bincount(want[:, 0], minlength=n)
    if name == "tile_borders":
        borders = list(range(EMIT_TILE, n - 1, EMIT_TILE))
        assert len(borders) >= 4
        last = {min(int(deg[t - 1]), 3) for t in borders}
        first = {min(int(deg[t]), 3) for t in borders}
        assert last == set(BORDER_CLASSES) and first == set(BORDER_CLASSES), (last, first)      # every class on either side of a border
    if name in ("repeats_tandems", "duplicates"):
        assert {1, 2} <= set(deg.tolist()) and deg.max() >= 3 and (name != "duplicates" or (deg == 0).any())
    for pile in (1, 3, 0, 2):
        for fold in (1, 0):
            got = {}
            for v in (0, 1):
                got[v], st = _build(eng, words, lens, lo, rs, {"pile": pile, "pile_deg_fold": fold, "emit_fused": v})
                assert got[v].shape == want.shape and (got[v] == want).all(), (name, pile, fold, v, got[v].shape, want.shape)
                if pile == 0:
                    assert st["ms_pile"] == 0.0
                if pile == 3:
                    assert st["pile_mixed"] == 1, st
            assert np.array_equal(got[0], got[1]), (name, pile, fold)
    if name in ("repeats_tandems", "duplicates"):          # rows filled from records: deferred sources of every out-degree class
        _, st = _build(eng, words, lens, lo, rs, {"emit_fused": 1})
        assert st["deferred_sources"] > 0, st


@pytest.mark.gpu
def test_a_declined_build_behind_a_kept_one_does_not_read_the_stale_slots(eng):
    """Reads with 2 % errors straight behind a build the pile path kept, on one engine: the sample declines on the device, the pairwise kernels
    write deg[] and the slots of the sources with edges, and the slots k_pile_probe left for the build before lie under every other source."""
    kept = _case("two_tiles_and_two_sources")
    words, lens = _nodes(4000, 150, 16_000, 61, err=0.02)
    assert len(lens) <= len(kept[1])                       # every source of the second build lies on a slot of the first
    lo, rs = alga_amd.derive_params(144.0)
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    assert (np.bincount(want[:, 0], minlength=len(lens)) == 0).any()
    for fold in (1, 0):
        for v in (0, 1):
            got, st = _build(eng, *kept[:4], {"pile_deg_fold": fold, "emit_fused": v})
            assert (got == kept[4]).all() and st["pile_irregular"] * alga_amd.engine.PILE_DECLINE_ONE_IN <= st["pile_buckets"] and st["pile_buckets"] > 0
            got, st = _build(eng, words, lens, lo, rs, {"pile_deg_fold": fold, "emit_fused": v})
            assert st["pile_irregular"] * alga_amd.engine.PILE_DECLINE_ONE_IN > st["pile_buckets"] > 0, st
            assert got.shape == want.shape and (got == want).all(), (fold, v)


@pytest.mark.gpu
@pytest.mark.parametrize("pile", [1, 3, 0, 2])
def test_a_source_range_that_begins_inside_a_tile(eng, pile):
    """src_base != 0: the rows of the sources [a, b) with a neither 0 nor a tile multiple; the range spans a tile border of its own."""
    words, lens, lo, rs, want = _case("tile_borders")
    dw = torch.from_numpy(words.view(np.int32)).cuda()
    dl = torch.from_numpy(lens.astype(np.int32)).cuda()
    n = len(lens)
    for a, b in ((EMIT_TILE // 2 + 3, n - 1), (EMIT_TILE + 2, 2 * EMIT_TILE + 2), (n // 3 - 1, n // 3 + 1)):
        assert a % EMIT_TILE != 0 and 0 < a < b <= n
        sel = want[(want[:, 0] >= a) & (want[:, 0] < b)]
        for fold in (1, 0):
            for v in (0, 1):
                for k, x in (("pile", pile), ("pile_deg_fold", fold), ("emit_fused", v)):
                    eng.set_option(k, x)
                try:
                    ptr, m = eng.build_range_device(dw, dl, lo, rs, a, b)
                    got = device_view(ptr, (m, 3), dw.device).cpu().numpy()
                finally:
                    for k, x in DEFAULTS.items():
                        eng.set_option(k, x)
                assert got.shape == sel.shape and (got == sel).all(), (pile, fold, v, a, b)


@pytest.mark.gpu
def test_more_tiles_than_the_spine_has_threads(eng):
    """A set generated on the device with more than SPINE_THREADS tiles: every thread of the spine sums a stretch of more than one tile sum."""
    wl = workload.device_build(2_600_000, 150, 13_000_000, 11)
    torch.cuda.synchronize()
    dw, dl, lo, rs = wl["words"], wl["lens"], wl["min_overlap"], wl["rsoemo"]
    assert int(dl.shape[0]) > SPINE_THREADS * EMIT_TILE
    got = {}
    try:
        for v in (0, 1):
            eng.set_option("emit_fused", v)
            ptr, m = eng.prefsuf_device(dw, dl, lo, rs)
            got[v] = device_view(ptr, (m, 3), dw.device).clone()
            assert m > 0 and eng.last_stats()["ms_pile"] > 0
    finally:
        eng.set_option("emit_fused", DEFAULTS["emit_fused"])
    assert got[0].shape == got[1].shape and bool(torch.equal(got[0], got[1]))


def test_the_two_passes_keep_their_registers():
    """The compiler's resource report for k_emit_tile_sums and k_emit_scan_tiles: no scratch, no VGPR or SGPR spill."""
    src = os.path.join(ROOT, "alga_amd", "csrc", "prefsuf_kernels.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_emit_fused_report_%d.o" % os.getpid())
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    try:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    finally:
        if os.path.exists(out):
            os.remove(out)
    lines = r.stderr.splitlines()
    for kernel in ("k_emit_tile_sums", "k_emit_scan_tiles"):
        at = [i for i, s in enumerate(lines) if "Function Name:" in s and kernel in s]
        assert len(at) == 1, "%s not in the report" % kernel
        rep = {}
        for s in lines[at[0] + 1:]:
            if "Function Name:" in s:
                break
            m = re.search(r"remark:\s+(.+?):\s+(\S+)\s+\[-Rpass", s)
            if m:
                rep[m.group(1)] = m.group(2)
        assert int(rep["VGPRs Spill"]) == 0 and int(rep["SGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, (kernel, rep)
