"""What the tests of the pile kernels' scheduling options share (test_gpu_pile_probe_tail.py, test_gpu_pile_runs_ahead.py): the node generator
and the three-way comparison of tests/test_gpu_pile.py for ONE option switched off and on, and the sorted keys of a node set on the host."""
import numpy as np
import torch

import alga_amd
import gen_reads
import oracle_lib as O
from alga_amd import workload
from alga_amd.engine import device_view

PB_TILE = 192                                              # entries per workgroup of k_pile_build: one "segment" of pile lists
PR_SEGS = 32                                               # segments per block of k_pile_runs_consensus_list
TK_ROWS = 128                                              # piles per round of that block
PP_TILE = 256                                              # sources per tile of k_pile_probe
PP_TAIL_K = 4                                              # candidates per batch of k_pile_probe's look-up


def nodes(n_reads, length, G, seed, err=0.0, genome=None):
    if genome is None:
        codes, _ = gen_reads.sample_reads(n_reads, length, G, seed, err)
    else:
        rng = np.random.default_rng(seed)
        starts = rng.integers(0, len(genome) - length + 1, size=n_reads)
        codes = np.stack([genome[s:s + length] for s in starts]).astype(np.uint8)
        flip = rng.random(n_reads) < 0.5
        codes[flip] = (3 - codes[flip])[:, ::-1]
    words, lens, _ = workload.make_nodes(codes)
    return words, lens


def tiled_nodes(G, length, skip_every, seed):
    """One read at every start of a random genome but each `skip_every`-th, strands at random: coverage length * (1 - 1 / skip_every) with no
    more reads on a stretch of starts than it has positions -- a k-mer's bucket, the reads that start up to 63 positions before it, is bounded."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=G).astype(np.uint8)
    starts = np.array([p for p in range(G - length + 1) if p % skip_every != 0])
    codes = np.stack([genome[s:s + length] for s in starts]).astype(np.uint8)
    flip = rng.random(len(starts)) < 0.5
    codes[flip] = (3 - codes[flip])[:, ::-1]
    words, lens, _ = workload.make_nodes(codes)
    return words, lens


def repeats_genome(seed):
    """A few units repeated with point differences plus a short-period stretch (tests/test_gpu_pile.py: test_pile_path_on_repeats_and_tandems)."""
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


def build(eng, words, lens, lo, rs, settings, defaults):
    for k, v in settings.items():
        eng.set_option(k, v)
    try:
        got = eng.prefsuf_host(words, lens, lo, rs, reduction="source_side")
    finally:
        for k in settings:
            eng.set_option(k, defaults[k])
    return got, eng.last_stats()


def option_off_and_on(eng, words, lens, lo, rs, opt, defaults, extra=None):
    """The edge list with `opt` at 1 equals the list with it at 0, the pairwise kernels' (pile 0) and the oracle's, in the pure (pile 2) and the
    mixed (pile 3) form, and both values hand the same sources on.  -> the oracle's list, the stats of the pure form with the option on."""
    extra = extra or {}
    want, _, _ = O.prefsuf(words, lens, lo, rs)
    got, st = build(eng, words, lens, lo, rs, dict(extra, pile=0), defaults)
    assert got.shape == want.shape and (got == want).all(), ("pairwise", got.shape, want.shape)
    assert st["ms_pile"] == 0.0
    keep = None
    for pile in (2, 3):
        res = {}
        for v in (0, 1):
            got, st = build(eng, words, lens, lo, rs, dict(extra, **{"pile": pile, opt: v}), defaults)
            assert got.shape == want.shape and (got == want).all(), (opt, v, "pile", pile, got.shape, want.shape)
            assert st["ms_pile"] > 0, (opt, v, pile)
            res[v] = (got, st)
        assert np.array_equal(res[0][0], res[1][0]), (opt, pile)
        for k in ("deferred_sources", "edges"):
            assert res[0][1][k] == res[1][1][k], (opt, pile, k, res[0][1][k], res[1][1][k])
        assert res[1][1]["edges"] == len(want)
        if pile == 2:
            keep = res[1][1]
    return want, keep


def sorted_keys(eng, words, lens, lo, rs, settings=None, defaults=None):
    """The sort keys of the nodes (alga_prefsuf_keys_device) in key order with the nodes that are no target dropped, and the shift that gives
    a key's bucket -- the table size comes from the stats of a build of the same nodes under the same settings."""
    settings = settings or {}
    dw = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()
    dl = torch.from_numpy(lens.astype(np.int32)).cuda()
    n = len(lens)
    for k, v in settings.items():
        eng.set_option(k, v)
    try:
        eng.prefsuf_device(dw, dl, lo, rs)
        n_buckets = int(eng.last_stats()["table_slots"])
        k = eng.keys_device(dw, dl, lo, rs, 0, n)
        assert k is not None
        keys = device_view(k[0], (n,), dw.device).cpu().numpy().view(np.uint32).astype(np.uint64)
    finally:
        for k in settings:
            eng.set_option(k, defaults[k])
    assert n_buckets & (n_buckets - 1) == 0
    shift = 32 - (n_buckets.bit_length() - 1)
    keys = np.sort(keys[keys != 0xFFFFFFFF])
    return keys, shift


def counts_of(x):
    """-> (first index, length) of every stretch of equal values of a sorted array"""
    first = np.flatnonzero(np.r_[True, x[1:] != x[:-1]])
    return first, np.diff(np.r_[first, len(x)])


def key_shapes(keys, shift):
    """Buckets, m_C >> 3 classes and k-mer groups of sorted keys: the key is bucket | m_C (6 bits below the bucket) | the cluster key's low bits."""
    _, bucket_n = counts_of(keys >> np.uint64(shift))
    _, class_n = counts_of(keys >> np.uint64(shift - 3))
    low = np.uint64((1 << (shift - 6)) - 1)
    kmer = ((keys >> np.uint64(shift)) << np.uint64(shift - 6)) | (keys & low)       # bucket | the k-mer's own bits: one value per k-mer group
    order = np.argsort(kmer, kind="stable")
    gfirst, group_n = counts_of(kmer[order])
    _, groups_per_bucket = counts_of(kmer[order][gfirst] >> np.uint64(shift - 6))
    return bucket_n, class_n, groups_per_bucket, order[gfirst]
