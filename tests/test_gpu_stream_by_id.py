"""The pile path's handed-on sources through k_probe_stream BY ID (alga_amd/csrc/prefsuf_cluster.hip; engine option "pile_stream_by_id"):

  pile_stream_by_id  1: a build the pile path keeps in its pure form sends the sources k_pile_probe hands on through k_probe_stream (list mode,
                     the entries taken by id from the sorted (key, id) pairs: it has no entry array) and the general kernel gets what is left;
                     0: the general kernel takes them all.

The option may only change how a graph is computed.  Every list is compared byte for byte with the CPU oracle's.  Option pile = 2 forces the
pure form whatever the sample says (every handed-on source takes the new pass), pile = 3 the mixed form (which keeps its entry-array pass).
The compiler's resource report of the new instantiations is checked without a GPU.

State: the GPU tests of this file were written with the pass and have not yet been run on a GPU; the option's
default is 0 until they have passed there and the pass has been measured."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import alga_amd
import oracle_lib as O
from alga_amd.engine import device_view
from test_gpu_pile_probe import CASES, _nodes, _repeats_genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = "pile_stream_by_id"
DEFAULT = 0                                                               # what the engine starts with (include/alga_amd.h)


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def _second_locus_genome(G, n_seg, seed):
    """A random genome with n_seg segments of 50 nt copied elsewhere: a 19-mer at two loci (an irregular bucket), and no overlap across the
    loci reaches the minimum length (82).  Sources in the first half, copies on a grid in the second: no copy touches another."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, size=G).astype(np.uint8)
    pitch = (G // 2) // n_seg
    for k in range(n_seg):
        a = int(rng.integers(0, G // 2 - 50))
        b = G // 2 + k * pitch + int(rng.integers(0, pitch - 50))
        g[b:b + 50] = g[a:a + 50]
    return g


def _second_locus(G, n_seg, seed):
    return _nodes(G * 30 // 150, 150, None, seed + 1, genome=_second_locus_genome(G, n_seg, seed))


def _build(eng, words, lens, lo, rs, pile, by_id):
    eng.set_option("pile", pile)
    eng.set_option(OPT, by_id)
    try:
        got = eng.prefsuf_host(words, lens, lo, rs, reduction="source_side")
    finally:
        eng.set_option("pile", 1)
        eng.set_option(OPT, DEFAULT)
    return got, eng.last_stats()


def _device(words, lens):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()


def _kept(st, pile):
    return st["ms_pile"] > 0 and (pile == 2 or st["pile_irregular"] * alga_amd.engine.PILE_DECLINE_ONE_IN <= st["pile_buckets"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,mean_len,rs", CASES, ids=[c[0] for c in CASES])
def test_every_form_gives_the_oracle_s_graph(eng, name, make, mean_len, rs):
    words, lens = make()
    lo, rs0 = alga_amd.derive_params(mean_len)
    rs = rs0 if rs is None else rs
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    for pile in (1, 2, 3):
        st = {}
        for v in (0, 1):
            got, st[v] = _build(eng, words, lens, lo, rs, pile, v)
            assert got.shape == want.shape and (got == want).all(), (name, pile, v, got.shape, want.shape)
        assert st[0]["ms_pile"] > 0 and st[1]["ms_pile"] > 0, (name, pile)
        assert _kept(st[0], pile) == _kept(st[1], pile) and st[0]["pile_mixed"] == st[1]["pile_mixed"], (name, pile)
        if pile == 2:
            assert _kept(st[1], pile) and st[1]["pile_mixed"] == 0, (name, st[1])
        if pile == 3:
            assert st[1]["pile_mixed"] == 1, (name, st[1])
        if _kept(st[1], pile) and st[1]["pile_mixed"] == 0:            # the pure form: the new pass between the pile kernel and the general kernel
            assert st[1]["deferred_sources"] <= st[1]["pile_deferred"], (name, pile, st[1])
            assert st[1]["pile_deferred"] == st[0]["deferred_sources"], (name, pile, st[0], st[1])       # the pile kernel hands on the same set
        else:                                                          # mixed or declined: the option changes nothing
            assert st[1]["deferred_sources"] == st[0]["deferred_sources"] and st[1]["pile_deferred"] == st[0]["pile_deferred"], (name, pile, st[0], st[1])


@pytest.fixture(scope="module")
def second_locus():
    words, lens = _second_locus(300_000, 60, 601)
    lo, rs = alga_amd.derive_params(144.0)
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    return words, lens, lo, rs, want


@pytest.mark.gpu
def test_second_locus_sources_finish_in_the_stream_kernel(eng, second_locus):
    """One 19-mer at two loci: every source with a run in such a bucket is handed on by the pile kernel although it is regular -- the other
    locus' entries simply fail the exact compare -- and the by-id pass finishes it."""
    words, lens, lo, rs, want = second_locus
    got, st = _build(eng, words, lens, lo, rs, 2, 1)
    print("second locus: nodes %d, pile_deferred %d, deferred_sources %d" % (len(lens), st["pile_deferred"], st["deferred_sources"]))
    assert got.shape == want.shape and (got == want).all()
    assert st["pile_mixed"] == 0 and st["pile_deferred"] > 0 and st["deferred_sources"] < st["pile_deferred"], st


@pytest.mark.gpu
def test_reads_with_errors_in_the_forced_pure_form(eng):
    """2 % errors: nearly every source is handed on -- the by-id pass bails out wave by wave, flushes its second list, and the swap moves it."""
    words, lens = _nodes(12_000, 150, 40_000, 23, err=0.02)
    lo, rs = alga_amd.derive_params(144.0)
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    st = {}
    for v in (0, 1):
        got, st[v] = _build(eng, words, lens, lo, rs, 2, v)
        assert got.shape == want.shape and (got == want).all(), (v, got.shape, want.shape)
    print("reads with errors: pile_deferred %d, deferred_sources %d (option off: %d)" % (st[1]["pile_deferred"], st[1]["deferred_sources"], st[0]["deferred_sources"]))
    assert st[1]["pile_deferred"] == st[0]["deferred_sources"] and st[1]["deferred_sources"] <= st[1]["pile_deferred"], (st[0], st[1])


@pytest.mark.gpu
@pytest.mark.parametrize("v", [0, 1])
def test_id_ranges_and_a_further_piece(eng, v):
    """Three id ranges with odd borders, the middle one in two pieces with the second at keys_shared = 2 (the index of the piece before):
    concatenated, the lists are the whole build's."""
    lo, rs = alga_amd.derive_params(144.0)
    words, lens = _second_locus(100_000, 40, 611)
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    dw, dl = _device(words, lens)
    n = len(lens)
    a, b = n // 3 - 1, 2 * (n // 3) + 3
    mid = (a + b) // 2 | 1
    eng.set_option("pile", 2)
    eng.set_option(OPT, v)
    try:
        ptr, m = eng.prefsuf_device(dw, dl, lo, rs, reduction="source_side")
        whole = device_view(ptr, (m, 3), dw.device).cpu().numpy()
        assert whole.shape == want.shape and (whole == want).all()
        parts = []
        for lo_id, hi_id, shared in ((0, a, 0), (a, mid, 0), (mid, b, 2), (b, n, 0)):
            ptr, m = eng.build_range_device(dw, dl, lo, rs, lo_id, hi_id, keys_shared=shared)
            assert eng.last_stats()["ms_pile"] > 0 or shared == 2, (lo_id, hi_id)
            got = device_view(ptr, (m, 3), dw.device).cpu().numpy()
            sel = whole[(whole[:, 0] >= lo_id) & (whole[:, 0] < hi_id)]
            assert got.shape == sel.shape and (got == sel).all(), (v, lo_id, hi_id, shared)
            parts.append(got)
        cat = np.concatenate(parts)                                         # (each piece is in the whole list's order: the rows, sorted, are the same)
        assert cat.shape == whole.shape and (cat[np.lexsort(cat.T[::-1])] == whole[np.lexsort(whole.T[::-1])]).all()
    finally:
        eng.set_option("pile", 1)
        eng.set_option(OPT, DEFAULT)


@pytest.fixture(scope="module")
def strided():
    words, lens = _second_locus(100_000, 40, 621)
    lo, rs = alga_amd.derive_params(144.0)
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    return words, lens, lo, rs, want


@pytest.mark.gpu
@pytest.mark.parametrize("stride,shift", [(9, 0), (10, 0), (12, 0), (13, 0), (16, 0), (12, 1), (16, 3)])
def test_rows_by_id_with_any_row_stride_and_base(eng, strided, stride, shift):
    """The by-id pass reads the rows from the caller's node array: two 16-byte loads and a word where the stride is a multiple of four words,
    at least twelve, and the base 16-byte aligned -- word by word for tight rows, odd strides and a base `shift` words off the alignment."""
    words, lens, lo, rs, want = strided
    n = len(lens)
    flat = np.full(n * stride + 8, 0xDEADBEEF, dtype=np.uint32)             # what lies between the rows is never looked at
    wide = flat[shift:shift + n * stride].reshape(n, stride)
    wide[:, :9] = words[:, :9]
    dflat = torch.from_numpy(flat.view(np.int32)).cuda()
    dw = dflat[shift:shift + n * stride].view(n, stride)
    assert dw.is_contiguous() and dw.data_ptr() % 16 == 4 * shift
    dl = torch.from_numpy(lens.astype(np.int32)).cuda()
    eng.set_option("pile", 2)
    eng.set_option(OPT, 1)
    try:
        ptr, m = eng.prefsuf_device(dw, dl, lo, rs, reduction="source_side")
    finally:
        eng.set_option("pile", 1)
        eng.set_option(OPT, DEFAULT)
    st = eng.last_stats()
    got = device_view(ptr, (m, 3), dw.device).cpu().numpy()
    assert got.shape == want.shape and (got == want).all(), (stride, shift, got.shape, want.shape)
    assert st["ms_pile"] > 0 and st["pile_deferred"] > 0 and st["deferred_sources"] < st["pile_deferred"], st      # the pass had entries to load


@pytest.mark.gpu
def test_repeat_builds_and_a_build_after_a_pairwise_one(eng, strided):
    """The same engine built twice gives the same bytes; and after a pairwise build of OTHER reads, which leaves an entry array behind, the
    by-id pass must read none of it."""
    words, lens, lo, rs, want = strided
    got1, _ = _build(eng, words, lens, lo, rs, 2, 1)
    got2, _ = _build(eng, words, lens, lo, rs, 2, 1)
    assert got1.tobytes() == got2.tobytes() and got1.shape == want.shape and (got1 == want).all()
    other, olens = _nodes(9000, 150, None, 19, genome=_repeats_genome(11))
    eng.set_option("pile", 0)
    try:
        eng.prefsuf_host(other, olens, lo, rs)
    finally:
        eng.set_option("pile", 1)
    for pile in (2, 1):
        got3, st = _build(eng, words, lens, lo, rs, pile, 1)
        assert got3.shape == want.shape and (got3 == want).all(), pile
        assert st["ms_pile"] > 0, pile


@pytest.mark.gpu
def test_empty_lists(eng):
    """40 reads; and an input on which the pile kernel hands on nothing: the pass and the swap see an empty list."""
    lo, rs = alga_amd.derive_params(144.0)
    words, lens = _nodes(40, 150, 1500, 631)
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    for v in (0, 1):
        got, _ = _build(eng, words, lens, lo, rs, 2, v)
        assert got.shape == want.shape and (got == want).all(), v
    # an input whose pile kernel hands on nothing: the property is looked for with the option OFF (deferred_sources is then what it handed on)
    for seed in range(641, 649):
        words, lens = _nodes(300, 150, 3000, seed)
        got0, st0 = _build(eng, words, lens, lo, rs, 2, 0)
        if st0["deferred_sources"] == 0:
            break
    else:
        pytest.fail("no input among eight on which the pile kernel hands on nothing")
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    got1, st1 = _build(eng, words, lens, lo, rs, 2, 1)
    assert got0.shape == want.shape and (got0 == want).all() and got1.shape == want.shape and (got1 == want).all()
    assert st1["pile_deferred"] == 0 and st1["deferred_sources"] == 0, st1


def _resource_report():
    src = os.path.join(ROOT, "alga_amd", "csrc", "prefsuf_cluster.hip")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "alga_stream_by_id_occupancy_%d.o" % os.getpid())
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
        # k_probe_stream<STATS, EQ, KF, BYKEY, LIST, BYID>
        m = re.search(r"Function Name: _ZN4alga14k_probe_streamILb([01])ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])EE", s)
        if not m:
            continue
        rep = {}
        for t in lines[i + 1:]:
            if "Function Name:" in t:
                break
            mm = re.search(r"remark:\s+(.+?):\s+(\S+)\s+\[-Rpass", t)
            if mm:
                rep[mm.group(1)] = mm.group(2)
        reps[tuple(int(x) for x in m.groups())] = rep
    return reps


def test_stream_kernel_resources():
    """The compiler's resource report of k_probe_stream: the three by-id list instantiations at five waves per SIMD or more, without VGPR spill
    or scratch; the pairwise path's kernel (statistics off, 150-bp shape, key order) where it was: six waves per SIMD, at most 80 VGPRs."""
    reps = _resource_report()
    for kf in (5, 3, 0):
        rep = reps.get((0, 3, kf, 0, 1, 1))
        assert rep is not None, "k_probe_stream<false, 3, %d, false, true, true> not in the report" % kf
        assert int(rep["Occupancy [waves/SIMD]"]) >= 5, (kf, rep)
        assert int(rep["VGPRs Spill"]) == 0 and int(rep["ScratchSize [bytes/lane]"]) == 0, (kf, rep)
    rep = reps.get((0, 3, 5, 1, 0, 0))
    assert rep is not None, "k_probe_stream<false, 3, 5, true, false> not in the report"
    assert int(rep["Occupancy [waves/SIMD]"]) == 6 and int(rep["VGPRs"]) <= 80, rep
