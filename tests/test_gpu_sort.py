"""The engine's own radix sort of (u32 key, u32 value) pairs (alga_amd/csrc/radix_sort.hip; what orders the nodes of the index build by
minimizer key in place of the reference's per-length re-bucketing, src/GraphCreators/GraphCreatorPrefSuf.cpp:317-332) against torch's
stable sort: every size class (one partial tile, exact tiles, many chunks, both sides of 2^22),
every pass plan (1 .. 32 key bits: one to four passes, digits of 1 .. 10 bits), skewed keys (all equal, two values, sorted, reversed),
bit for bit including the order of equal keys (stability).  The rocPRIM path (option own_sort = 0) is held to the same on full keys, and on a
partial key to its documented contract: below 2^22 items it sorts on all 32 bits, from 2^22 on stably on the window (the last section).

The second half of the file holds the paths no sort test reached before, against np.argsort(kind="stable") of the looked-at bits on the host:
the implicit values 0, 1, 2, ... (vals=None: k_rs_scatter<.., IOTA = true>), the 12-byte records of the sharded build (sort_desc_device:
rsort_u32_u64 on a key window), the tiles of 16384 pairs (option rsort_variant = 1), key arrays that are not 16-byte aligned, a last tile whose
real keys share the padding's digit, the chunk and group seams of the scans, and that two runs give the same bytes."""
import contextlib
import functools

import numpy as np
import pytest

import alga_amd
from alga_amd.engine import device_view

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def _check(eng, keys_u32, begin_bit, own=True):
    import torch
    n = len(keys_u32)
    k = torch.from_numpy(keys_u32.view(np.int32)).cuda()
    v = torch.arange(n, dtype=torch.int32, device="cuda")
    kp, vp, _ = eng.sort_u32_pairs_device(k, v, begin_bit, own)
    torch.cuda.synchronize()
    if n == 0:
        return
    gk = device_view(kp, (n,), k.device).clone()
    gv = device_view(vp, (n,), k.device).clone()
    # the reference order: stable on the looked-at bits
    sk = (k.to(torch.int64) & 0xFFFFFFFF) >> begin_bit
    _, perm = torch.sort(sk, stable=True)
    assert torch.equal(gv.to(torch.int64), perm), "values (= stable order) differ, begin_bit %d n %d" % (begin_bit, n)
    assert torch.equal(gk, k[perm])
    assert torch.equal(k, torch.from_numpy(keys_u32.view(np.int32)).cuda())          # the input is left untouched


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 8191, 8192, 8193, 100_000, 3 * 8192 * 512 + 17, (1 << 22) - 5, (1 << 22) + 12345])
def test_random_keys_every_size_class(eng, n):
    rng = np.random.default_rng(n + 7)
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    _check(eng, keys, 3)                                   # 29 bits: 10 + 10 + 9, the north-star plan
    _check(eng, keys, 0)                                   # 32 bits: four passes of 8


@pytest.mark.parametrize("begin_bit", list(range(0, 32)))
def test_every_pass_plan(eng, begin_bit):
    rng = np.random.default_rng(100 + begin_bit)
    keys = rng.integers(0, 1 << 32, size=200_003, dtype=np.uint64).astype(np.uint32)
    _check(eng, keys, begin_bit)


@pytest.mark.parametrize("kind", ["equal", "two", "sorted", "reversed", "few_high_bits", "one_digit_hot"])
def test_skewed_keys(eng, kind):
    n = 300_000
    rng = np.random.default_rng(5)
    if kind == "equal":
        keys = np.full(n, 0xDEADBEE8, dtype=np.uint32)
    elif kind == "two":
        keys = np.where(rng.random(n) < 0.5, 0x00000008, 0xFFFFFFF8).astype(np.uint32)
    elif kind == "sorted":
        keys = np.sort(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))
    elif kind == "reversed":
        keys = np.sort(rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))[::-1].copy()
    elif kind == "few_high_bits":
        keys = (rng.integers(0, 4, size=n, dtype=np.uint64) << 30).astype(np.uint32) | rng.integers(0, 8, size=n, dtype=np.uint64).astype(np.uint32)
    else:
        keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        keys[rng.random(n) < 0.9] = 0x12345678                  # nine items in ten share every digit: one wave-match group of 64 lanes per step
    _check(eng, keys, 3)
    _check(eng, keys, 0)


def test_library_path_on_full_keys(eng):
    rng = np.random.default_rng(9)
    for n in (100_000, (1 << 22) + 999):
        keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        _check(eng, keys, 0, own=False)


def test_index_build_same_graph_with_either_sort(eng):
    """the whole build with the engine's sort and with the library's: same edges (the order of equal keys is the same for both -- stable)."""
    import gen_reads
    from alga_amd import workload
    codes, _ = gen_reads.sample_reads(20_000, 150, 60_000, 77)
    words, lens, _ = workload.make_nodes(codes)
    lo, rs = alga_amd.derive_params(144.0)
    # What this compares: at this size (< 2^22 nodes) the library path sorts on all 32 key bits and the engine's on [idx_shift - 3, 32), so the two
    # SORTED ARRAYS are the same only where the bits below begin_bit do not differ inside a group (the condition pinned by
    # test_library_and_own_sort_agree_when_the_low_bits_are_zero below).  A target's key has hash bits there (tgt_sort_key), so the entries of one
    # (bucket, m_C >> 3) group can come in two orders: the equality below is about the GRAPH, which must not depend on the order inside a group.
    a = eng.prefsuf_host(words, lens, lo, rs)
    eng.set_option("own_sort", 0)
    try:
        b = eng.prefsuf_host(words, lens, lo, rs)
    finally:
        eng.set_option("own_sort", 1)
    assert a.shape == b.shape and (a == b).all()


# ---- the 16-byte records of the supplement (radix_sort.hip: rsort_u64_pairs) ---------------------------------------------------------------

def _check64(eng, keys_u64, bits, own=True):
    import torch
    n = len(keys_u64)
    k = torch.from_numpy(keys_u64.view(np.int64)).cuda()
    v = (torch.arange(n, dtype=torch.int64, device="cuda") << 33) | 5          # values wider than 32 bits
    kp, vp, ms = eng.sort_u64_pairs_device(k, v, bits, own)
    torch.cuda.synchronize()
    if n == 0:
        return ms
    gk = device_view(kp, (n,), k.device, "<i8").clone()
    gv = device_view(vp, (n,), k.device, "<i8").clone()
    low = k & ((1 << bits) - 1) if bits < 63 else k
    _, perm = torch.sort(low, stable=True)
    assert torch.equal(gv, v[perm]), "values (= stable order) differ, bits %d n %d" % (bits, n)
    assert torch.equal(gk, k[perm])
    assert torch.equal(k, torch.from_numpy(keys_u64.view(np.int64)).cuda())
    return ms


@pytest.mark.parametrize("n", [0, 1, 63, 65, 4095, 4096, 4097, 100_000, 3 * 4096 * 512 + 17, (1 << 22) + 12345])
def test_u64_records_every_size_class(eng, n):
    rng = np.random.default_rng(n + 11)
    keys = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * 2 + rng.integers(0, 2, size=n, dtype=np.uint64)
    _check64(eng, keys, 30)                                # the supplement's plan at 10 M reads: 10 + 10 + 10
    _check64(eng, keys, 40)


@pytest.mark.parametrize("bits", [1, 7, 8, 9, 10, 11, 19, 20, 21, 29, 31, 32, 33, 41, 50])
def test_u64_records_every_pass_plan(eng, bits):
    rng = np.random.default_rng(300 + bits)
    keys = rng.integers(0, 1 << 63, size=150_001, dtype=np.uint64)
    _check64(eng, keys, bits)


@pytest.mark.parametrize("kind", ["equal", "two", "sorted", "reversed", "one_digit_hot"])
def test_u64_records_skewed_keys(eng, kind):
    n = 200_000
    rng = np.random.default_rng(6)
    if kind == "equal":
        keys = np.full(n, 0x123456789ABCDEF, dtype=np.uint64)
    elif kind == "two":
        keys = np.where(rng.random(n) < 0.5, np.uint64(0x3FFFFFFF), np.uint64(1 << 40)).astype(np.uint64)
    elif kind == "sorted":
        keys = np.sort(rng.integers(0, 1 << 62, size=n, dtype=np.uint64))
    elif kind == "reversed":
        keys = np.sort(rng.integers(0, 1 << 62, size=n, dtype=np.uint64))[::-1].copy()
    else:
        keys = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
        keys[rng.random(n) < 0.9] = np.uint64(0x2AAAAAAA)
    _check64(eng, keys, 30)


def test_u64_records_library_path_agrees(eng):
    rng = np.random.default_rng(8)
    keys = rng.integers(0, 1 << 62, size=500_000, dtype=np.uint64)
    _check64(eng, keys, 32, own=False)
    _check64(eng, keys, 40, own=False)


# ---- the paths below were reached by no sort test: everything against the host ---------------------------------------------------------------
# Reference of every test from here on: np.argsort(kind="stable") of the looked-at key bits, computed in uint64 on the host; the whole key
# array and the whole value array must be equal to it (a permutation of integers: no tolerance), and the inputs must come back unchanged.

TILE32 = {0: 8192, 1: 16384}                               # pairs per tile of rsort_u32_pairs by option rsort_variant
TILE64 = 4096                                              # records per tile of rsort_u64_pairs and rsort_u32_u64


def _bits(keys, begin_bit, end_bit):
    return (keys.astype(np.uint64) >> np.uint64(begin_bit)) & np.uint64((1 << (end_bit - begin_bit)) - 1)


def _perm(keys, begin_bit, end_bit):
    return np.argsort(_bits(keys, begin_bit, end_bit), kind="stable")


@functools.lru_cache(maxsize=4)
def _rand32(seed, n):
    k = np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=4)
def _rand32_perm(seed, n, begin_bit, end_bit):
    """the reference order of _rand32(seed, n), computed once and shared (read-only)"""
    p = _perm(_rand32(seed, n), begin_bit, end_bit)
    p.setflags(write=False)
    return p


def _vals_for(shape, n):
    if shape == "u32":
        return np.arange(n, dtype=np.uint32)
    return (np.arange(n, dtype=np.uint64) << np.uint64(33)) | np.uint64(5)          # values wider than 32 bits


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a).view(np.int32 if a.dtype == np.uint32 else np.int64)).cuda()       # (a copy: the shared inputs are read-only)


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _sort(eng, shape, k, v, window, own=True):
    """shape: "u32" (u32 key, u32 value), "u64" (u64, u64; the window is [0, end)), "desc" (u32 key, u64 value) -> sorted (keys, values) on the
    host, and the engine's two output pointers"""
    import torch
    n = int(k.shape[0])
    b, e = window
    if shape == "u32":
        assert e == 32
        kp, vp, _ = eng.sort_u32_pairs_device(k, v, b, own)
    elif shape == "u64":
        assert b == 0
        kp, vp, _ = eng.sort_u64_pairs_device(k, v, e, own)
    else:
        kp, vp, _ = eng.sort_desc_device(k, v, b, e, own)
    torch.cuda.synchronize()
    kd, vd = ("<i8", np.uint64) if shape == "u64" else ("<i4", np.uint32), ("<i4", np.uint32) if shape == "u32" else ("<i8", np.uint64)
    return _host(device_view(kp, (n,), k.device, kd[0]), kd[1]), _host(device_view(vp, (n,), k.device, vd[0]), vd[1]), kp, vp


def _check_host(eng, shape, keys, window, own=True, iota=False, ref_window=None, perm=None, vals=None):
    """sort `keys` (numpy) with values 0, 1, 2, ... (u32; implicit with iota) or (i << 33) | 5 and hold the result to the host reference on
    ref_window (default: the window asked for) -> the sorted (keys, values)"""
    n = len(keys)
    if vals is None:
        vals = _vals_for(shape, n)
    k = _dev(keys)
    v = None if iota else _dev(vals)
    gk, gv, _, _ = _sort(eng, shape, k, v, window, own)
    if perm is None:
        perm = _perm(keys, *(ref_window or window))
    assert np.array_equal(gv, vals[perm]), "values (= stable order) differ: %s window %s n %d" % (shape, window, n)
    assert np.array_equal(gk, keys[perm]), "keys differ: %s window %s n %d" % (shape, window, n)
    assert np.array_equal(_host(k, keys.dtype), keys), "the key input was written"
    if v is not None:
        assert np.array_equal(_host(v, vals.dtype), vals), "the value input was written"
    return gk, gv


@contextlib.contextmanager
def _variant(eng, v):
    """option rsort_variant is process-wide: always back to 0"""
    try:
        eng.set_option("rsort_variant", v)
        yield
    finally:
        eng.set_option("rsort_variant", 0)


# ---- 1. implicit values: vals_in == nullptr, k_rs_scatter<.., IOTA = true> (the index build, the final-contig filter, the supplement) ------------

@pytest.mark.parametrize("begin_bit", [0, 3, 12, 22, 31])         # 4, 3, 2, 1, 1 passes: the first (IOTA) pass ends in the intermediate buffer and in the output
@pytest.mark.parametrize("n", [1, 64, 8191, 8192, 8193, 100_000, 512 * 8192 + 1])      # the last: 513 tiles, two per chunk, a last chunk of one tile, a last tile of one item
def test_implicit_values(eng, n, begin_bit):
    keys = _rand32(1000 + n, n)
    perm = _rand32_perm(1000 + n, n, begin_bit, 32)
    ik, iv = _check_host(eng, "u32", keys, (begin_bit, 32), iota=True, perm=perm)
    ek, ev = _check_host(eng, "u32", keys, (begin_bit, 32), perm=perm)               # the same call with an explicit arange
    assert np.array_equal(ik, ek) and np.array_equal(iv, ev)


def test_implicit_values_are_refused_by_the_library_path(eng):
    keys = _rand32(77, 10_000)
    with pytest.raises(alga_amd.AlgaError) as ei:
        eng.sort_u32_pairs_device(_dev(keys), None, 3, own=False)
    assert ei.value.code == -1                             # ALGA_ERR_INVALID_ARGUMENT: rocPRIM needs values
    _check_host(eng, "u32", keys, (3, 32))                 # and the engine goes on
    _check_host(eng, "u32", keys, (0, 32), own=False)


# ---- 2. the 12-byte records of the sharded build: sort_desc -> rsort_u32_u64 on a key window ---------------------------------------------------

DESC_WINDOWS = [(0, 32), (0, 1), (3, 32), (5, 15), (5, 16), (7, 28), (12, 20), (31, 32)]      # (5, 15): one pass of 10; (5, 16): 6 + 5; (7, 28): three passes


@pytest.mark.parametrize("window", DESC_WINDOWS, ids=lambda w: "%d-%d" % w)
@pytest.mark.parametrize("n", [1, 63, 4095, 4096, 4097, 100_000, 512 * 4096 + 1])
def test_desc_records_every_window_and_size(eng, n, window):
    # full-range keys: the bits outside the window vary, so a wrong shift or mask changes the order
    _check_host(eng, "desc", _rand32(2000 + n, n), window, perm=_rand32_perm(2000 + n, n, *window))


@pytest.mark.parametrize("window", [(3, 32), (12, 20)], ids=lambda w: "%d-%d" % w)
@pytest.mark.parametrize("kind", ["equal", "two", "sorted", "reversed", "one_digit_hot"])
def test_desc_records_skewed_keys(eng, kind, window):
    n = 200_000
    rng = np.random.default_rng(12)
    if kind == "equal":
        keys = np.full(n, 0xDEADBEE8, dtype=np.uint32)
    elif kind == "two":
        keys = np.where(rng.random(n) < 0.5, 0x00003008, 0xFFFC5FF8).astype(np.uint32)      # (they differ inside both windows)
    elif kind == "sorted":
        keys = np.sort(_rand32(13, n))
    elif kind == "reversed":
        keys = np.sort(_rand32(13, n))[::-1].copy()
    else:
        keys = _rand32(13, n).copy()
        keys[rng.random(n) < 0.9] = 0x12345678
    _check_host(eng, "desc", keys, window)


@pytest.mark.parametrize("window", [(5, 5), (-1, 8), (4, 33)], ids=lambda w: "%d_%d" % w)
def test_desc_records_invalid_window_is_all_32_bits(eng, window):
    for n in (4097, 100_000):
        _check_host(eng, "desc", _rand32(2100 + n, n), window, ref_window=(0, 32))


def test_desc_records_nothing_to_sort(eng):
    import torch
    keys = _rand32(2200, 5000)
    gk, gv, kp, vp = _sort(eng, "desc", _dev(keys), _dev(_vals_for("desc", 5000)), (3, 32))
    k0, v0 = torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda")
    ek, ev, _, _ = _sort(eng, "desc", k0, v0, (3, 32))
    assert len(ek) == 0 and len(ev) == 0
    _sort(eng, "desc", k0, v0, (3, 32), own=False)
    # the result of the call before is still there, untouched
    assert np.array_equal(_host(device_view(kp, (5000,), k0.device), np.uint32), gk)
    assert np.array_equal(_host(device_view(vp, (5000,), k0.device, "<i8"), np.uint64), gv)


# ---- 3. the wide tile: option rsort_variant = 1, 16384 pairs and 1024 threads per tile ------------------------------------------------------------

@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n", [16383, 16384, 16385, 100_000, 512 * 16384 + 1])
def test_variant_random_keys_every_size_class(eng, n, variant):
    keys = _rand32(3000 + n, n)
    with _variant(eng, variant):
        _check_host(eng, "u32", keys, (3, 32), perm=_rand32_perm(3000 + n, n, 3, 32))
        _check_host(eng, "u32", keys, (0, 32), perm=_rand32_perm(3000 + n, n, 0, 32))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("begin_bit", list(range(0, 32)))
def test_variant_every_pass_plan(eng, begin_bit, variant):
    with _variant(eng, variant):
        _check_host(eng, "u32", _rand32(3100 + begin_bit, 200_003), (begin_bit, 32), perm=_rand32_perm(3100 + begin_bit, 200_003, begin_bit, 32))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("kind", ["equal", "two", "sorted", "reversed", "few_high_bits", "one_digit_hot"])
def test_variant_skewed_keys(eng, kind, variant):
    n = 300_000
    rng = np.random.default_rng(5)
    if kind == "equal":                                    # a wave's counter of one digit reaches 1024, the tile's 16384: the 16-bit halves of the packed scan
        keys = np.full(n, 0xDEADBEE8, dtype=np.uint32)
    elif kind == "two":
        keys = np.where(rng.random(n) < 0.5, 0x00000008, 0xFFFFFFF8).astype(np.uint32)
    elif kind == "sorted":
        keys = np.sort(_rand32(31, n))
    elif kind == "reversed":
        keys = np.sort(_rand32(31, n))[::-1].copy()
    elif kind == "few_high_bits":
        keys = (rng.integers(0, 4, size=n, dtype=np.uint64) << 30).astype(np.uint32) | rng.integers(0, 8, size=n, dtype=np.uint64).astype(np.uint32)
    else:
        keys = _rand32(31, n).copy()
        keys[rng.random(n) < 0.9] = 0x12345678
    with _variant(eng, variant):
        _check_host(eng, "u32", keys, (3, 32))
        _check_host(eng, "u32", keys, (0, 32))


@pytest.mark.parametrize("n", [16385, 100_000, 512 * 16384 + 1])
def test_variant_wide_tile_implicit_values(eng, n):
    keys = _rand32(3000 + n, n)
    with _variant(eng, 1):
        for begin_bit in (0, 3):
            _check_host(eng, "u32", keys, (begin_bit, 32), iota=True, perm=_rand32_perm(3000 + n, n, begin_bit, 32))


def test_variant_outside_0_and_1_is_refused(eng):
    """variant 2 is rs_plan's internal code of the 4096-record tiles: it must never reach rsort_u32_pairs through the option"""
    keys = _rand32(3200, 100_000)
    try:
        for v in (-1, 2, 3):
            with pytest.raises(alga_amd.AlgaError) as ei:
                eng.set_option("rsort_variant", v)
            assert ei.value.code == -1
        _check_host(eng, "u32", keys, (3, 32))             # still variant 0 ...
        with _variant(eng, 1):
            _check_host(eng, "u32", keys, (3, 32))         # ... and variant 1 can still be had
    finally:
        eng.set_option("rsort_variant", 0)


# ---- 4. the first pass over keys that are not 16-byte aligned: the scalar loop of k_rs_hist (aligned == 0) ------------------------------------------

@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n", [8192 + 5, 3 * 8192, 512 * 8192 + 1])
def test_unaligned_keys(eng, n, variant):
    import torch
    keys = _rand32(4000 + n, n)
    vals = _vals_for("u32", n)
    with _variant(eng, variant):
        for begin_bit in (0, 3):
            perm = _rand32_perm(4000 + n, n, begin_bit, 32)
            ak, av = _check_host(eng, "u32", keys, (begin_bit, 32), perm=perm)       # the aligned copy
            for off in (1, 2, 3):
                hk, hv = np.full(n + 3, 0xA5A5A5A5, dtype=np.uint32), np.full(n + 3, 0x5A5A5A5A, dtype=np.uint32)
                hk[off:off + n] = keys
                hv[off:off + n] = vals
                bk, bv = _dev(hk), _dev(hv)
                k, v = bk[off:off + n], bv[off:off + n]
                assert k.data_ptr() % 16 == 4 * off and v.data_ptr() % 16 == 4 * off
                gk, gv, _, _ = _sort(eng, "u32", k, v, (begin_bit, 32))
                assert np.array_equal(gv, vals[perm]) and np.array_equal(gk, keys[perm]), "off %d begin_bit %d" % (off, begin_bit)
                assert np.array_equal(gk, ak) and np.array_equal(gv, av)
                assert np.array_equal(_host(bk, np.uint32), hk) and np.array_equal(_host(bv, np.uint32), hv)      # the inputs and what lies around them


# ---- 5. the last tile's padding (~0) against real keys with every looked-at bit set ------------------------------------------------------------------

PAD_CASES = [("u32", 0, (0, 32)), ("u32", 0, (3, 32)), ("u32", 1, (0, 32)), ("u32", 1, (3, 32)),
             ("u64", 0, (0, 30)), ("u64", 0, (0, 40)), ("desc", 0, (3, 32)), ("desc", 0, (5, 16))]


@pytest.mark.parametrize("where", ["everywhere", "last_tile"])
@pytest.mark.parametrize("shape,variant,window", PAD_CASES, ids=lambda x: "%d-%d" % x if isinstance(x, tuple) else str(x))
def test_padding_shares_its_digit_with_real_keys(eng, shape, variant, window, where):
    """the only place where the padding and real items meet in one digit: every real item must come out in front, in input order, nothing lost,
    and nothing of the padding written (the word behind the n-th output stays as it was)"""
    import torch
    tile = TILE32[variant] if shape == "u32" else TILE64
    dt = np.uint64 if shape == "u64" else np.uint32
    top = 64 if shape == "u64" else 32
    ones = np.uint64(((1 << (window[1] - window[0])) - 1) << window[0])
    with _variant(eng, variant):
        for n in (tile + 1, tile + 63, 2 * tile - 1):
            rng = np.random.default_rng(n)
            keys = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
            if top == 32:
                keys >>= np.uint64(32)
            lo = 0 if where == "everywhere" else tile
            if shape == "u32":
                keys[lo:] = 0xFFFFFFFF
            else:
                keys[lo:] |= ones                          # all ones in the window, the bits outside it stay random
            keys = keys.astype(dt)
            vals = _vals_for(shape, n) + dt(7) if shape == "u32" else _vals_for(shape, n)      # (no real value is the padding's 0)
            _check_host(eng, shape, keys, window, vals=vals)
            # once more with a mark behind the end of both outputs (the engine's buffers hold n + 1 items at least)
            k, v = _dev(keys), _dev(vals)
            _, _, kp, vp = _sort(eng, shape, k, v, window)
            kt = device_view(kp, (n + 1,), k.device, "<i8" if shape == "u64" else "<i4")
            vt = device_view(vp, (n + 1,), k.device, "<i4" if shape == "u32" else "<i8")
            kt[n] = 0x13572468
            vt[n] = 0x2468ACE
            torch.cuda.synchronize()
            gk, gv, kp2, vp2 = _sort(eng, shape, k, v, window)
            assert (kp2, vp2) == (kp, vp)
            assert int(kt[n]) == 0x13572468 and int(vt[n]) == 0x2468ACE, "the sort wrote behind its output: %s n %d" % (shape, n)
            perm = _perm(keys, *window)
            assert np.array_equal(gk, keys[perm]) and np.array_equal(gv, vals[perm])


# ---- 6. chunk and group seams of the scans ----------------------------------------------------------------------------------------------------------------
# up to 512 tiles a chunk is one tile; k_rs_scan_chunks deals the chunks to 32 groups: 31 .. 33 chunks go from one chunk per group (the last group
# empty) to two (the trailing groups empty); 513 tiles are the first with two tiles per chunk

@pytest.mark.parametrize("shape", ["u32", "desc"])
@pytest.mark.parametrize("tiles", [31, 32, 33, 511, 512, 513])
def test_chunk_and_group_seams(eng, tiles, shape):
    tile = TILE32[0] if shape == "u32" else TILE64
    n = (tiles - 1) * tile + 1234                          # not a multiple of the tile
    _check_host(eng, shape, _rand32(6000 + tiles, n), (3, 32), perm=_rand32_perm(6000 + tiles, n, 3, 32))


# ---- 7. the same input twice: the same bytes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["random", "one_digit_hot"])
@pytest.mark.parametrize("shape,window", [("u32", (3, 32)), ("u64", (0, 30)), ("desc", (3, 20))])
def test_two_runs_give_the_same_bytes(eng, shape, window, kind):
    n = 300_007
    rng = np.random.default_rng(70)
    keys = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    if kind == "one_digit_hot":
        keys[rng.random(n) < 0.9] = np.uint64(0x2AAAAAAA12345678)
    if shape != "u64":
        keys = (keys >> np.uint64(30)).astype(np.uint32)
    a = _check_host(eng, shape, keys, window)
    b = _check_host(eng, shape, keys, window)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 8. the library path's contract on a partial key (own = False) ---------------------------------------------------------------------------------------
# below 2^22 items it sorts on ALL 32 bits (rocPRIM's small-input comparison looks at the wrong bits of a partial key: sort_records.hip), from 2^22
# on stably on the window.

LIB_CASES = [("u32", (3, 32)), ("desc", (3, 20))]


@pytest.mark.parametrize("shape,window", LIB_CASES)
def test_library_path_small_inputs_sort_on_all_32_bits(eng, shape, window):
    _check_host(eng, shape, _rand32(8000, 100_000), window, own=False, ref_window=(0, 32))


@pytest.mark.parametrize("shape,window", LIB_CASES)
def test_library_path_large_inputs_sort_on_the_window(eng, shape, window):
    n = (1 << 22) + 999
    _check_host(eng, shape, _rand32(8001, n), window, own=False, perm=_rand32_perm(8001, n, *window))


@pytest.mark.parametrize("n", [100_000, (1 << 22) + 999])
@pytest.mark.parametrize("shape,window", LIB_CASES)
def test_library_and_own_sort_agree_when_the_low_bits_are_zero(eng, shape, window, n):
    """all 32 bits and the window give one order when no bit outside the window tells two keys apart: no bit set below begin_bit, and for the
    descriptors the bits from end_bit on the same for every key (as in the sharded build: one rank's bucket range)"""
    keys = _rand32(8002, n) & np.uint32(~((1 << window[0]) - 1) & 0xFFFFFFFF)
    if window[1] < 32:
        keys = (keys & np.uint32((1 << window[1]) - 1)) | np.uint32(0xABC00000)
    perm = _perm(keys, *window)
    assert np.array_equal(perm, _perm(keys, 0, 32))
    a = _check_host(eng, shape, keys, window, own=False, perm=perm)
    b = _check_host(eng, shape, keys, window, own=True, perm=perm)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
