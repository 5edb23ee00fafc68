"""Inputs for the final contig set (include/alga_amd.h: alga_final_contigs_device, alga_contig_trim_device) with their answers written out:
tests/test_final_cpu.py holds the Python definition (tests/final_checker.py) to them, tests/test_gpu_final.py the device.

Verdict cases are graphs built like tests/contig_cases.py: lengths only (read k = node 2k+1, its twin 2k, 100 nt) over pseudo-random rows, edges
in the forward direction; the contigs come from the contig call, the windows from the consensus at min_votes 0 (the whole contig).  A contig is
named by the sorted read indices of its path entries, which no orientation or pair numbering changes; `want` maps that name to
(verdict, new_reads, id) at the case's min_length / percent.  The contig of a chain r0 .. rk with offsets o1 .. ok is 100 + o1 + .. + ok long."""
import numpy as np

import contig_cases as CC
import final_checker as F

S, R, A = F.SHORT, F.REJECTED, F.ACCEPTED


def _chain(reads, offset=10):
    return [(2 * a + 1, 2 * b + 1, offset) for a, b in zip(reads[:-1], reads[1:])]


def _boundaries():
    """X (50 reads) -> J1; J1 -> 37 reads -> J2 and J1 -> 38 reads -> J2 (parallel, too heavy to be dropped at max_offset 5); J2 -> Y (45 reads);
    J1 -> 17 reads -> a dead end and J1 -> 18 reads -> a dead end.  X and Y are the longest and mark J1 and J2."""
    nxt = [0]

    def fresh(k):
        out = list(range(nxt[0], nxt[0] + k))
        nxt[0] += k
        return out

    (J1,), (J2,) = fresh(1), fresh(1)
    X, Y, c37, c38, c17, c18 = fresh(50), fresh(45), fresh(37), fresh(38), fresh(17), fresh(18)
    e1, e2 = fresh(1), fresh(1)
    paths = dict(X=X + [J1], Y=[J2] + Y, c37=[J1] + c37 + [J2], c38=[J1] + c38 + [J2], c17=[J1] + c17 + e1, c18=[J1] + c18 + e2)
    edges = [x for p in paths.values() for x in _chain(p)]
    name = lambda p: tuple(sorted(p))
    want = {name(paths["X"]): (A, 51, 0), name(paths["Y"]): (A, 46, 1),
            name(paths["c38"]): (A, 38, 2),                                   # 100 * (38 / 40) = 95: not below 95
            name(paths["c37"]): (R, 37, -1),                                  # 37 / 39 = 94.87 %
            name(paths["c18"]): (A, 19, 3),                                   # 19 / 20: J1 is marked, the dead end is not
            name(paths["c17"]): (R, 18, -1)}                                  # 18 / 19 = 94.74 %
    return dict(reads=nxt[0], max_offset=5, edges=edges, min_length=1, percent=95, want=want)


LADDER_JUNCTIONS = 40


def _ladder():
    """Junctions J0 .. J39 in a line, rung i = Ji -> Ii -> J(i+1) with both offsets 90 - i (so the rungs get shorter along the line: 280 - 2i nt), a
    stub Ji -> Si (110 nt) at every junction and a second one at the last, so that every junction branches.  At 95 per cent a rung needs all three
    reads new: rung 0 is accepted, rung 1 shares J1 with it and is rejected, rung 2 shares J2 with a rejected rung and is accepted, ...; every
    junction ends up marked, every stub has one new read of two."""
    n = LADDER_JUNCTIONS
    J = list(range(n))
    I = list(range(n, 2 * n - 1))
    St = list(range(2 * n - 1, 3 * n - 1))
    last = 3 * n - 1
    edges, want = [], {}
    for i in range(n - 1):
        edges += [(2 * J[i] + 1, 2 * I[i] + 1, 90 - i), (2 * I[i] + 1, 2 * J[i + 1] + 1, 90 - i)]
        want[tuple(sorted((J[i], I[i], J[i + 1])))] = (A, 3, i // 2) if i % 2 == 0 else (R, 2, -1)
    for i in range(n):
        edges.append((2 * J[i] + 1, 2 * St[i] + 1, 10))
        want[tuple(sorted((J[i], St[i])))] = (R, 1, -1)
    edges.append((2 * J[n - 1] + 1, 2 * last + 1, 20))
    want[tuple(sorted((J[n - 1], last)))] = (R, 1, -1)
    return dict(reads=3 * n, max_offset=5, edges=edges, min_length=1, percent=95, want=want)


_FORK = [(7, 1, 10), (1, 3, 10), (1, 5, 20)]                                  # Z -> A, A -> B, A -> C: reads A = 0, B = 1, C = 2, Z = 3

CASES = {
    # the junction read A is in all three contigs: {A, C} is the longest, the other two have one new read of two
    "fork": dict(reads=4, max_offset=100, edges=_FORK, min_length=1, percent=95, want={(0, 2): (A, 2, 0), (0, 3): (R, 1, -1), (0, 1): (R, 1, -1)}),
    # 100 * (1 / 2) = 50 is not below 50: all three; the two of 110 nt in pair order ({A, Z} is pair 0: its `+` starts at node 0)
    "fork_at_50": dict(reads=4, max_offset=100, edges=_FORK, min_length=1, percent=50, want={(0, 2): (A, 2, 0), (0, 3): (A, 1, 1), (0, 1): (A, 1, 2)}),
    "fork_at_0": dict(reads=4, max_offset=100, edges=_FORK, min_length=1, percent=0, want={(0, 2): (A, 2, 0), (0, 3): (A, 1, 1), (0, 1): (A, 1, 2)}),
    "fork_at_100": dict(reads=4, max_offset=100, edges=_FORK, min_length=1, percent=100, want={(0, 2): (A, 2, 0), (0, 3): (R, 1, -1), (0, 1): (R, 1, -1)}),
    # 120 nt is the longest contig: the other two are short, and a short contig marks nothing
    "fork_min_length": dict(reads=4, max_offset=100, edges=_FORK, min_length=111, percent=95, want={(0, 2): (A, 2, 0), (0, 3): (S, -1, -1), (0, 1): (S, -1, -1)}),
    "fork_all_short": dict(reads=4, max_offset=100, edges=_FORK, min_length=121, percent=95, want={(0, 2): (S, -1, -1), (0, 3): (S, -1, -1), (0, 1): (S, -1, -1)}),
    # A -> B and A -> C, both 110 nt: `+` of the pairs are 1 -> 3 and 1 -> 5, the smaller pair number ranks first and takes A
    "equal_lengths": dict(reads=3, max_offset=100, edges=[(1, 3, 10), (1, 5, 10)], min_length=1, percent=95, want={(0, 1): (A, 2, 0), (0, 2): (R, 1, -1)}),
    # T -> R1 (offset 80: 180 nt) and the ring R1 -> R2 -> R3 -> R1 (a closed chain of 130 nt with R1 at both ends): R1 is marked by the longer
    # contig and counts twice, 2 new of 4 = 50 %; counted once it would be 3 of 4 = 75 % and pass 60
    "closed_chain_counts_twice": dict(reads=4, max_offset=100, edges=[(1, 3, 80), (3, 5, 10), (5, 7, 10), (7, 3, 10)], min_length=1, percent=60,
                                      want={(0, 1): (A, 2, 0), (1, 1, 2, 3): (R, 2, -1)}),
    "closed_chain_at_50": dict(reads=4, max_offset=100, edges=[(1, 3, 80), (3, 5, 10), (5, 7, 10), (7, 3, 10)], min_length=1, percent=50,
                               want={(0, 1): (A, 2, 0), (1, 1, 2, 3): (A, 2, 1)}),
    # the two boundaries of 95 per cent: 19 / 20 and 38 / 40 pass, 18 / 19 and 37 / 39 do not
    "boundaries_at_95": _boundaries(),
    "ladder": _ladder(),
}


def inputs(name):
    c = CASES[name]
    words, lens = CC.nodes_of(c["reads"])
    return words, lens, np.array(c["edges"], dtype=np.int32).reshape(-1, 3), c["max_offset"]


def name_of(u, k):
    po = np.asarray(u["path_off"]).astype(np.int64)
    return tuple(sorted(int(v) >> 1 for v in np.asarray(u["path_node"])[po[k]: po[k + 1]]))


def assert_equals_expected(u, fin, name):
    """fin: verdict / new_reads / id per pair (the checker's dict or the device's host copy)"""
    want = CASES[name]["want"]
    got = {name_of(u, k): (int(fin["verdict"][k]), int(fin["new_reads"][k]), int(fin["id"][k])) for k in range(int(u["n_pairs"]))}
    assert len(got) == int(u["n_pairs"]), "two pairs with the same reads"
    assert got == want, (name, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)})


# ---- the reference's graph dumps: (dump, bound of the cut); the settings every verdict test runs ----------------------------------------------
DUMPS = [("f2_err2.aftersimplifier.graph", 262), ("f4_varlen.aftersimplifier.graph", 250), ("f5_messy.aftercut.graph", 250)]
SETTINGS = [(200, 95), (150, 95), (1, 95), (1, 50)]                          # (min_length, per cent)
MIN_VOTES = (0, 3)
_cache = {}


def golden_contigs(golden_dir, graph, bound, min_votes):
    """one checker run per dump and min_votes, shared by the tests (read only) -> (words, lens, edges, contigs, consensus)"""
    import consensus_checker as SC
    import contig_checker as CT
    import unitig_cases as K
    if graph not in _cache:
        words, lens, edges = K.golden(golden_dir, graph)
        _cache[graph] = (words, lens, edges, CT.contigs(words, lens, edges, bound))
    if (graph, min_votes) not in _cache:
        words, lens, edges, u = _cache[graph]
        _cache[graph, min_votes] = SC.consensus_pileup(words, lens, u, min_votes)
    return _cache[graph] + (_cache[graph, min_votes],)


# ---- sequences for the trim: chained, branching, on both strands, with lengths round the cap ----------------------------------------------------
def trim_set(seed=11, n_chains=40):
    """-> list of code arrays.  Every chain walks along its own random genome: contig i + 1 starts `overlap` bases before the end of contig i
    (25 .. 500, now and then below the threshold or past the cap), every third contig is written as its reverse complement, one contig in six
    gets a branch: a second contig that starts with its end and goes on with other bases.  Lengths: 1001, 1002, 1003 (the cap and its two
    neighbours), 2000 .. 3500, and a few short ones."""
    if ("trim", seed, n_chains) in _cache:
        return _cache["trim", seed, n_chains]
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n_chains):
        g = rng.integers(0, 4, size=40000, dtype=np.uint8)
        p = 0
        for i in range(10):
            L = int(rng.choice([1001, 1002, 1003])) if rng.random() < 0.3 else int(rng.integers(2000, 3501)) if rng.random() < 0.8 else int(rng.integers(200, 1001))
            s = g[p: p + L].copy()
            ov = int(rng.choice([25, 26, 100, 499, 500, 501])) if rng.random() < 0.4 else int(rng.integers(25, 501)) if rng.random() < 0.9 else int(rng.choice([20, 24, 520]))
            ov = min(ov, L - 1)
            if rng.random() < 1 / 6:                                           # a branch off the end of this contig
                b = np.concatenate([s[L - min(ov, 300):], rng.integers(0, 4, size=int(rng.integers(900, 1200)), dtype=np.uint8)])
                out.append(b if rng.random() < 0.5 else (3 - b)[::-1])
            out.append((3 - s)[::-1] if (len(out) % 3) == 2 else s)
            p += L - ov
    _cache["trim", seed, n_chains] = out
    return out


def ragged(seqs, shifts):
    """the sequences laid into one packed word array, sequence i starting at a base index = shifts[i] mod 16 -> (words uint32, begin int64, len int32)"""
    begin, at = [], 0
    for s, sh in zip(seqs, shifts):
        at += (sh - at) % 16
        begin.append(at)
        at += len(s)
    codes = np.zeros(16 * ((at + 15) // 16 + 1), dtype=np.uint64)
    for s, b in zip(seqs, begin):
        codes[b: b + len(s)] = s
    words = (codes.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
    return words, np.array(begin, dtype=np.int64), np.array([len(s) for s in seqs], dtype=np.int32)
