"""The families of tests/merge_fuzz.py without a GPU: the two Python statements of the merge stage (tests/merge_checker.py) agree on every family
and variant (`chains` and `chain_mismatches` on the reduced draws `*_small` of the same generators, `long_windows` not at all: the quadratic statement cannot take
them), the invariants of every result hold (tests/merge_invariants.py), and every family holds what it was made for, asserted from the inputs and
the checker's output so that a later change of a generator cannot empty a family in silence.

Measured on one CPU core: the whole file in 21 s, of which the quadratic statement takes about 16 s (`repeats` 5 x 1.7 s, `edges` 3 x 2 s, the
reduced draws of the chains 3.5 s) and merge_index on `long_windows` 2.5 s (0.6 s on `chains`).  The times are recorded, not asserted."""
import collections
import time

import numpy as np
import pytest

import merge_checker as MC
import merge_fuzz as F
import merge_invariants as MI
import place_checker as P

# (ends_with_overlap, ends_ambiguous, joins, joins_dropped_cycle, merged) of every variant of every family
OUTCOMES = {"chains": [(4978, 0, 2476, 13, 62), (2438, 0, 1218, 1, 1320)], "chains_small": [(110, 0, 54, 1, 7), (62, 0, 31, 0, 30)],
            "chain_mismatches": [(1558, 0, 779, 0, 39), (798, 0, 399, 0, 419)], "chain_mismatches_small": [(182, 0, 91, 0, 9), (92, 0, 46, 0, 54)],
            "repeats": [(49, 18, 13, 0, 37), (49, 18, 13, 0, 37), (49, 18, 13, 0, 37), (55, 27, 10, 0, 40), (19, 6, 4, 0, 46)],
            "edges": [(68, 0, 34, 0, 95), (68, 0, 34, 0, 95), (68, 0, 34, 0, 95)], "long_windows": [(2560, 0, 1280, 0, 20)]}


def assert_same(got, want, name, i):
    diff = F.first_difference(got, want)
    if diff is not None:
        print("family %s variant %d seed %d: first difference (array, index, got, want): %s" % (name, i, F.SEEDS[name], diff))
    for k in MC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (name, i, F.SEEDS[name], k, diff)
    assert got["info"] == want["info"], (name, i, F.SEEDS[name], got["info"], want["info"])


@pytest.mark.parametrize("name,i", F.every(set(F.BRUTE.values())))
def test_the_two_statements_agree(name, i):
    c, want = F.case(name), F.checked(name, i)
    t0 = time.time()
    assert_same(MC.merge_bruteforce(c["seqs"], **c["variants"][i]), want, name, i)
    print(name, i, "merge_bruteforce %.2f s" % (time.time() - t0), want["info"])


@pytest.mark.parametrize("name,i", F.every())
def test_outcomes_and_invariants(name, i):
    c = F.case(name)
    t0 = time.time()
    want = F.checked(name, i)
    t = time.time() - t0
    info = want["info"]
    print(name, i, "merge_index %.2f s (0 when another test computed it)" % t, info)
    assert (info["ends_with_overlap"], info["ends_ambiguous"], info["joins"], info["joins_dropped_cycle"], info["merged"]) == OUTCOMES[name][i], info
    MI.assert_invariants(c, want, c["variants"][i])


def test_every_family_is_listed():
    assert sorted(OUTCOMES) == sorted(F.CASES) == sorted(F.SEEDS) and all(len(OUTCOMES[n]) == len(F.case(n)["variants"]) for n in F.CASES)
    assert set(F.GPU_FAMILIES) | {"chains_small", "chain_mismatches_small"} == set(F.CASES) and set(F.BRUTE) | {"long_windows"} == set(F.GPU_FAMILIES)
    assert len(set(F.SEEDS.values())) == len(F.SEEDS)
    for name in F.CASES:
        tb = F.case(name)["tbegin"]
        assert (tb & 15).tolist() == [3 * i % 16 for i in range(len(tb))]


def _members(w, j):
    return w["m_members"][int(w["m_off"][j]):int(w["m_off"][j + 1])].tolist()


@pytest.mark.parametrize("name", ["chains", "chains_small"])
def test_chains_are_laid_out_whole(name):
    c, w = F.case(name), F.checked(name)
    chains, rings = (F.CHAIN_LENGTHS, F.RING_LENGTHS) if name == "chains" else (F.SMALL_CHAINS, F.SMALL_RINGS)
    sizes = collections.Counter((w["m_off"][1:].astype(np.int64) - w["m_off"][:-1]).tolist())
    planted = collections.Counter(chains + rings)
    assert all(sizes[m] >= n for m, n in planted.items()) and sum(sizes.values()) - sizes[1] == len(chains) + len(rings), sizes
    assert w["info"]["joins_dropped_cycle"] == len(rings) and w["info"]["joins"] == sum(chains) - len(chains) + sum(rings) - len(rings)
    assert sorted(len(ids) for _, ids, _, _ in c["groups"]) == sorted(chains + rings)
    tlen = c["tlen"]
    assert (tlen == 0).sum() >= 2 and (tlen == 1).sum() >= 2 and (w["merged"][tlen == 0] == -1).all()
    far = near = flipped_smallest = 0
    first_orient = set()
    for kind, ids, flipped, o in c["groups"]:
        j = int(w["merged"][ids[0]])
        mem = _members(w, j)
        if kind == "ring":
            # one contig of all its members, opened at its smallest contig, whose left end loses its join and which is laid out first, as it is
            s = min(ids)
            at = ids.index(s)
            assert sorted(mem) == sorted(ids) and mem[0] == s and w["rank"][s] == 0 and w["orient"][s] == 0
            assert w["end_state"][2 * s] & MC.DROPPED_CYCLE and not w["end_state"][2 * s] & MC.JOINED and w["end_state"][2 * s + 1] & MC.JOINED
            assert int((w["end_state"][[2 * x + e for x in ids for e in (0, 1)]] & MC.DROPPED_CYCLE > 0).sum()) == 2
            # around the ring from s: in the direction of the generator if s is as it was made, against it if it is reverse complemented
            step = -1 if flipped[at] else 1
            assert mem == [ids[(at + step * r) % len(ids)] for r in range(len(ids))]
            flipped_smallest += flipped[at]
        else:
            # from the terminal of smaller id; the starts are the lengths less the overlaps
            rev = ids[-1] < ids[0]
            order, ov = (ids[::-1], o[::-1]) if rev else (ids, o)
            assert mem == order and w["overlap_after"][order].tolist() == ov + [0]
            assert w["start"][order].tolist() == np.concatenate([[0], np.cumsum(tlen[order[:-1]] - np.array(ov))]).tolist()
            assert w["orient"][order].tolist() == [f ^ int(rev) for f in (flipped[::-1] if rev else flipped)]
            far, near = far + rev, near + (not rev)
            first_orient.add(int(w["orient"][order[0]]))
    assert far >= 1 and near >= 1 and first_orient == {0, 1} and flipped_smallest >= 1, (far, near, first_orient, flipped_smallest)
    if name == "chains":
        assert max(sizes) == 1025 and far >= 4 and near >= 4 and 2 <= flipped_smallest <= len(rings) - 2
        first = F.checked(name, 1)                                               # the first of two rounds leaves joins to the second
        assert 0 < first["info"]["joins"] < w["info"]["joins"] and first["info"]["merged_multi"] > 100 and first["info"]["joins_dropped_cycle"] >= 1


@pytest.mark.parametrize("name", ["chain_mismatches", "chain_mismatches_small"])
def test_chain_mismatches_take_the_earlier_members_base(name):
    c, w = F.case(name), F.checked(name)
    info = w["info"]
    assert info["join_mismatches"] == len(c["made"]) > 30 and info["joins"] == sum(c["lengths"]) - len(c["lengths"])
    assert {col == 0 for _, _, o, col, _ in c["made"]} == {col == o - 1 for _, _, o, col, _ in c["made"]} == {0 < col < o - 1 for _, _, o, col, _ in c["made"]} == {True, False}
    assert {later for _, _, _, _, later in c["made"]} == {0, 1}
    new = MC.sequences(w)
    deep = twice = 0
    for j in range(len(w["len"])):
        mem = _members(w, j)
        for r in range(len(mem) - 1):
            a, b = mem[r], mem[r + 1]
            out = 2 * a + (int(w["orient"][a]) ^ 1)
            ov = int(w["overlap_after"][a])
            assert ov == w["olen"][out] and int(w["start"][b]) == int(w["start"][a]) + int(c["tlen"][a]) - ov
            sa, sb = (P.revcomp(c["seqs"][x]) if w["orient"][x] else c["seqs"][x] for x in (a, b))
            cols = np.nonzero(sa[len(sa) - ov:] != sb[:ov])[0]
            assert len(cols) == int(w["mm"][out]) <= 1
            for col in cols:                                                     # the merged base is the earlier member's, not the later one's
                at = int(w["start"][b]) + int(col)
                assert new[j][at] == sa[len(sa) - ov + col] != sb[col]
                deep += r + 1 >= 2
            if r >= 1 and int(w["overlap_after"][mem[r - 1]]) + ov == int(c["tlen"][a]):
                # a is covered twice over its whole length: b begins where the member before a ends
                assert int(w["start"][b]) == int(w["start"][mem[r - 1]]) + int(c["tlen"][mem[r - 1]])
                twice += 1
    assert deep >= 20 and twice >= 8, (deep, twice)
    # the planted joins, by the ids of their windows
    for a, b, o, col, later in c["made"]:
        x = [e for e in (2 * a, 2 * a + 1) if w["partner"][e] >> 1 == b]
        assert len(x) == 1 and w["olen"][x[0]] == o and w["mm"][x[0]] == 1 and w["end_state"][x[0]] & MC.JOINED
    strict = F.checked(name, 1)
    assert strict["info"]["joins"] == info["joins"] - len(c["made"]) and strict["info"]["join_mismatches"] == 0
    for a, b, o, col, later in c["made"]:
        assert (strict["partner"][2 * a:2 * a + 2] >> 1 != b).all()


def _at(name, i, x):
    c = F.case(name)
    found, usable, occ = F.found_at(c["seqs"], x, **c["variants"][i])
    w = F.checked(name, i)
    assert int(w["hits"][x]) == min(len(found), 255)
    if found:
        mm, y, o = min((mm, y, -o) for mm, y, o in found)
        assert (int(w["mm"][x]), int(w["partner"][x]), -int(w["olen"][x])) == (mm, y, o)
    return found, usable, occ


def test_repeats_saturate_and_tie():
    c = F.case("repeats")
    made = c["made"]
    # hits saturates at the ends of AT
    v = c["variants"][3]
    assert v == dict(k=8, max_occ=65535, max_mismatches=0, min_overlap=8, max_overlap=512)
    w = F.checked("repeats", 3)
    at_ends = [2 * t + (0 if (t - made["at_ends"]) % 2 else 1) for t in range(made["at_ends"], made["n"])]
    assert w["info"]["hits_saturated"] == F.AT_ENDS == len(at_ends) and (w["hits"][at_ends] == 255).all() and (np.delete(w["hits"], at_ends) < 255).all()
    found, _, _ = _at("repeats", 3, at_ends[0])
    assert len(found) == (F.AT_ENDS - 1) * ((512 - 8) // 2 + 1) > 255 and (w["olen"][at_ends] == 512).all()
    assert all(F.checked("repeats", i)["info"]["hits_saturated"] == 0 for i in (0, 1, 2, 4))
    assert all(F.checked("repeats", i)["info"]["ends_ambiguous"] > 0 for i in range(5))
    # more than 64 usable (seed, occurrence) pairs at one end: a second pass of the candidate loop
    x = 2 * made["two_letter"] + 1
    for i, least in ((0, 65), (3, 65)):
        found, usable, occ = _at("repeats", i, x)
        assert usable >= least and max(occ) <= c["variants"][i].get("max_occ", 256), (i, usable, occ)
        print("variant", i, "end", x, "usable (seed, occurrence) pairs", usable, "of", len(occ), "seeds; overlaps", found)
    # a small max_occ: many seeds over it, overlaps found through the others
    small = F.checked("repeats", 4)
    assert c["variants"][4]["max_occ"] == 4 and small["info"]["seeds_over_max_occ"] > 500 and small["info"]["joins"] >= 4
    through_others = 0
    for t in range(made["shared"], made["at_ends"]):
        for x in (2 * t, 2 * t + 1):
            if small["end_state"][x] & MC.JOINED:
                found, usable, occ = _at("repeats", 4, x)
                through_others += any(n > 4 for n in occ[:int(small["olen"][x]) // 8]) and len(found) == 1
    assert through_others >= 4
    assert F.checked("repeats", 0)["info"]["seeds_over_max_occ"] > F.checked("repeats", 3)["info"]["seeds_over_max_occ"] == 0


@pytest.mark.parametrize("i", [0, 1, 2])
def test_repeats_winners_by_mm_by_y_and_by_o(i):
    """the key (mm, y, o descending): an end whose winner has a rival of smaller end id and larger mm, one with a rival of equal mm and o and a
    larger end id, one whose rivals differ in o alone"""
    c, w = F.case("repeats"), F.checked("repeats", i)
    made = c["made"]
    a = made["duplicates"]
    x = 2 * a + 1
    found, _, _ = _at("repeats", i, x)
    win = (int(w["mm"][x]), int(w["partner"][x]), int(w["olen"][x]))
    assert win in found and len(found) == 3 and win == (0, 2 * (a + 2) + 1, 90)          # the reverse complemented copy c, at its right end
    assert any(mm > win[0] and y < win[1] and o == win[2] for mm, y, o in found)        # b: one substitution, the smaller id
    assert any(mm == win[0] and y > win[1] and o == win[2] for mm, y, o in found)       # d: as good, the larger id
    for t in (a + 1, a + 2, a + 3):                                                      # each of the three chooses a and is alone there
        e = 2 * t + (1 if t == a + 2 else 0)
        assert w["partner"][e] == x and w["hits"][e] == 1 and not w["end_state"][e] & MC.JOINED
    x2 = 2 * (a + 4) + 1                                                                 # the second group: b is out of reach, c and d tie but for y
    assert w["hits"][x2] == 2 and w["partner"][x2] == 2 * (a + 6) + 1 and w["mm"][x2] == 0
    by_o = 0
    for n, p in enumerate(F.TANDEM_PERIODS):
        x = 2 * (made["tandem"] + 2 * n) + 1
        found, _, _ = _at("repeats", i, x)
        k = c["variants"][i].get("k", 21)
        want_o = [o for o in range(96, 41, -p) if o >= k]
        if not found:
            continue                                                                     # (every seed of a short period is over max_occ, or no whole seed is usable)
        assert len({(mm, y) for mm, y, o in found}) == 1 and sorted((o for _, _, o in found), reverse=True) == want_o[:len(found)] and w["olen"][x] == 96
        by_o += len(found) > 1
    assert by_o >= 4


def test_edges_bounds_residues_and_seeds():
    c = F.case("edges")
    ks = [v.get("k", 21) for v in c["variants"]]
    assert ks == [8, 21, 31] and all(dict(MC.DEFAULT, **v)["max_overlap"] == 512 == 64 * 8 for v in c["variants"])
    for i, k in enumerate(ks):
        w = F.checked("edges", i)
        seen = collections.defaultdict(set)
        for part, t, o, pairing, col in c["pairs"]:
            ends = [2 * t + (pairing[0] == "R"), 2 * (t + 1) + (pairing[1] == "R")]
            others = [e ^ 1 for e in ends]
            assert (w["hits"][others] == 0).all()
            if part == "bounds" and o in (41, 513):
                assert (w["hits"][ends] == 0).all() and (w["partner"][ends] == -1).all(), (part, o, pairing)
            else:
                assert w["partner"][ends].tolist() == ends[::-1] and (w["olen"][ends] == o).all() and (w["end_state"][ends] == MC.HAS_OVERLAP | MC.JOINED).all(), (part, o, pairing)
                assert (w["mm"][ends] == (1 if part == "mismatches" else 0)).all()
            seen[part, o].add(pairing)
            if part == "mismatches":                                             # the seed of either end's P that holds the column
                S = o // k
                for cc in (col, o - 1 - col):
                    seen["where"].add("first" if cc < k else "tail" if cc >= S * k else "last" if cc >= (S - 1) * k else "middle")
        assert all(seen["bounds", o] == set(F.PAIRINGS) for o in F.EDGE_BOUNDS)
        assert {o % 16 for o in F.EDGE_RESIDUES} == set(range(16)) and {0, 1, k - 1} <= {o % k for o in F.EDGE_RESIDUES}
        assert seen["where"] >= {"first", "last", "tail"}, seen["where"]
        # an end of 64 seeds: at k = 8 every end of the 16 long targets of `bounds` has W = 512 = max_overlap
        S = [min(int(c["tlen"][t + d]) // 2, dict(MC.DEFAULT, **c["variants"][i])["max_overlap"]) // k for part, t, o, _, _ in c["pairs"] if part == "bounds" and o > 100 for d in (0, 1)]
        assert len(S) == 16 and set(S) == {512 // k} and (k != 8 or set(S) == {64})
        assert int((c["tlen"] >= 1024).sum()) == 16 and w["info"]["seeds"] == sum(min(int(n) // 2, 512) // k for n in c["tlen"] if n >= 84) * 2
        # merged contigs of 1 to 15 bases side by side: a word of the output holds several
        tiny = w["len"] < 16
        assert int(tiny.sum()) == F.EDGE_TINY and sorted(set(w["len"][tiny].tolist())) == list(range(1, 16))
        assert np.bincount(w["col_off"][:-1] >> 4).max() >= 4


def test_long_windows_take_three_chunks():
    c, w = F.case("long_windows"), F.checked("long_windows")
    text = F.fasta("long_windows")
    longest = max(len(s) for s in text.split(b">"))
    step = (1 << 20) - (longest + 1)                                             # the writer's chunk step at gfa_chunk_mb 1: the chunk less the longest record
    assert len(text) > 2 << 20 and 2 * longest < 1 << 20 and -(-len(text) // step) >= 3
    assert w["info"]["columns_after"] > 2 << 20 and sorted(collections.Counter((w["m_off"][1:] - w["m_off"][:-1]).tolist()).elements()) == sorted(F.LONG_CHAINS)
    assert 42 <= int(w["olen"][w["olen"] > 0].min()) <= 50 and 500 <= w["info"]["longest_overlap"] <= 512
