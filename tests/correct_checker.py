"""The definition of the read error correction (include/alga_amd.h: alga_correct_reads_device), literally, in numpy and a dictionary.

Nothing here is shared with the device's method: the k-mers are encoded first base first (the device: last base first, then mixed), counted in
one dictionary (the device: sorted slices), and a run's candidates are tried one after the other on a copy of the read."""
import collections

import numpy as np


def blocks_of(length):
    return 0 if length <= 0 else (2 * length - 1) // 32 + 1


def codes_of(row, length):
    """the bases (0 .. 3) of a packed row"""
    w = np.asarray(row, dtype=np.uint32)
    i = np.arange(length)
    return ((w[i >> 4] >> ((i & 15) << 1).astype(np.uint32)) & 3).astype(np.uint8)


def pack(codes, stride):
    out = np.zeros(stride, dtype=np.uint32)
    c = np.asarray(codes, dtype=np.uint32)
    i = np.arange(len(c))
    np.bitwise_or.at(out, i >> 4, c << ((i & 15) << 1).astype(np.uint32))
    return out


def revcomp(codes):
    return (3 - np.asarray(codes, dtype=np.uint8)[::-1]).astype(np.uint8)


def nodes_of(reads, stride=None):
    """forward reads (arrays of codes; None = a removed pair, len -1) -> rows, lens in the parser's layout: node 2r = reverse complement,
    2r + 1 = read r"""
    need = max([blocks_of(len(r)) for r in reads if r is not None] + [1])
    stride = need if stride is None else stride
    assert stride >= need
    rows = np.zeros((2 * len(reads), stride), dtype=np.uint32)
    lens = np.full(2 * len(reads), -1, dtype=np.int32)
    for r, c in enumerate(reads):
        if c is None:
            continue
        lens[2 * r] = lens[2 * r + 1] = len(c)
        rows[2 * r + 1] = pack(c, stride)
        rows[2 * r] = pack(revcomp(c), stride)
    return rows, lens


def forward_reads(rows, lens):
    """the forward reads of a node set as code arrays (None for len < 0)"""
    return [codes_of(rows[2 * r + 1], lens[2 * r + 1]) if lens[2 * r + 1] >= 0 else None for r in range(len(lens) // 2)]


def canonical_kmers(codes, k):
    """canonical form of every k-mer of a read, as integers with the FIRST base most significant"""
    c = np.asarray(codes, dtype=np.uint64)
    win = np.lib.stride_tricks.sliding_window_view(c, k)
    wt = (np.uint64(4) ** np.arange(k - 1, -1, -1, dtype=np.uint64))
    fwd = (win * wt).sum(axis=1, dtype=np.uint64)
    rc = ((np.uint64(3) - win[:, ::-1]) * wt).sum(axis=1, dtype=np.uint64)
    return np.minimum(fwd, rc)


def check_params(k, solid_min, min_run):
    if k < 5 or k > 31 or k % 2 == 0:
        raise ValueError("k must be odd and in [5, 31]")
    if solid_min < 1 or min_run < 1:
        raise ValueError("solid_min and min_run must be >= 1")


def suspect(a, b, nk, k, min_run):
    """step 3: the position of the suspected base of the run [a, b], or None (skipped)"""
    length = b - a + 1
    if length < min_run:
        return None
    if a == 0 and b == nk - 1:
        return None
    if a > 0 and b < nk - 1:
        return b if length == k else None
    if a == 0:
        return b if b <= k - 1 else None
    return a + k - 1 if length <= k else None


def correct(rows, lens, k=21, solid_min=3, min_run=1):
    """-> (new rows, info dict with the counters of alga_correct_info); ValueError where the device refuses"""
    check_params(k, solid_min, min_run)
    rows = np.asarray(rows, dtype=np.uint32)
    lens = np.asarray(lens, dtype=np.int32)
    n = len(lens)
    if n % 2:
        raise ValueError("n_nodes must be even")
    stride = rows.shape[1] if rows.ndim == 2 else 1
    for r in range(n // 2):
        lf, lr = int(lens[2 * r + 1]), int(lens[2 * r])
        if lf != lr:
            raise ValueError("twin lengths differ")
        if lf > 0:
            if blocks_of(lf) > stride:
                raise ValueError("a length exceeds the stride")
            nw = blocks_of(lf)
            if not (pack(revcomp(codes_of(rows[2 * r + 1], lf)), stride)[:nw] == rows[2 * r][:nw]).all():
                raise ValueError("row 2r is not the reverse complement of row 2r + 1")
    out = rows.copy()
    info = dict(reads=0, kmers_total=0, kmers_distinct=0, kmers_solid=0, runs=0, runs_fixed=0, runs_ambiguous=0, runs_no_candidate=0, runs_skipped=0,
                reads_changed=0)
    # 1. the spectrum of the reads as they came in
    count = collections.Counter()
    reads = {}
    for r in range(n // 2):
        length = int(lens[2 * r + 1])
        if length < k:
            continue
        reads[r] = codes_of(rows[2 * r + 1], length)
        kms = canonical_kmers(reads[r], k)
        count.update(kms.tolist())
        info["reads"] += 1
        info["kmers_total"] += len(kms)
    info["kmers_distinct"] = len(count)
    info["kmers_solid"] = sum(1 for v in count.values() if v >= solid_min)

    def solid(x):
        return count.get(int(x), 0) >= solid_min

    for r, read in reads.items():
        nk = len(read) - k + 1
        weak = [not solid(x) for x in canonical_kmers(read, k)]
        # 2. maximal runs of weak k-mers of the unmodified read
        runs, i = [], 0
        while i < nk:
            if weak[i]:
                j = i
                while j + 1 < nk and weak[j + 1]:
                    j += 1
                runs.append((i, j))
                i = j + 1
            else:
                i += 1
        fixes = []
        for a, b in runs:
            info["runs"] += 1
            p = suspect(a, b, nk, k, min_run)
            if p is None:
                info["runs_skipped"] += 1
                continue
            # 4. the bases that work
            works = []
            for x in range(4):
                if x == read[p]:
                    continue
                trial = read.copy()
                trial[p] = x
                if all(solid(y) for y in canonical_kmers(trial[a:b + k], k)):
                    works.append(x)
            if len(works) == 1:
                info["runs_fixed"] += 1
                fixes.append((p, works[0]))
            elif not works:
                info["runs_no_candidate"] += 1
            else:
                info["runs_ambiguous"] += 1
        # 5. all fixes of a read together
        if fixes:
            new = read.copy()
            for p, x in fixes:
                new[p] = x
            nw = blocks_of(len(new))
            out[2 * r + 1][:nw] = pack(new, stride)[:nw]
            out[2 * r][:nw] = pack(revcomp(new), stride)[:nw]
            info["reads_changed"] += 1
    return out, info


def mirror(rows, lens):
    """the node set of the reverse complements: every pair's two rows swapped"""
    out = np.asarray(rows).copy()
    out[0::2], out[1::2] = np.asarray(rows)[1::2], np.asarray(rows)[0::2]
    return out, np.asarray(lens).copy()


COUNTERS = ("reads", "kmers_total", "kmers_distinct", "kmers_solid", "runs", "runs_fixed", "runs_ambiguous", "runs_no_candidate", "runs_skipped",
            "reads_changed")
