"""The families of tests/gapped_fuzz.py without a GPU: the two Python statements of the gapped placement (tests/gapped_checker.py) agree on every
family and variant, the invariants of every result hold (tests/gapped_invariants.py), and every family does what it was made for, asserted from
the checker's output so that a later change of a generator cannot empty a family in silence.

Measured on one CPU core: the whole file in 26 s, of which `tandem` takes 9 s (4 369 counting candidates, both statements), `two_letter` 6.5 s and
`long_reads` 3 s."""
import math

import pytest

import gapped_checker as GC
import gapped_fuzz as F
import gapped_invariants as GI
import place_checker as P

# (tried, placed, unique, with_indel, edits) of every variant of every family
OUTCOMES = {"duplicates": [(31, 30, 14, 28, 30), (31, 30, 14, 28, 30)],
            "edges": [(55, 49, 48, 45, 295), (55, 27, 27, 24, 56), (55, 29, 29, 25, 60), (55, 47, 46, 44, 291)],
            "long_reads": [(11, 8, 8, 6, 29)], "pool": [(249, 221, 221, 204, 631)], "tandem": [(65, 64, 61, 57, 78)],
            "three_letter": [(31, 9, 9, 7, 13), (31, 29, 29, 27, 96)], "two_letter": [(33, 11, 11, 7, 18), (33, 31, 31, 25, 102)],
            "two_letter_k12": [(35, 14, 14, 12, 23), (35, 31, 31, 28, 96)]}
FAMILIES = sorted(set(F.CASES) - {"pool"})


def assert_same(got, want, name, i):
    diff = F.first_difference(got, want)
    if diff is not None:
        print("family %s variant %d seed %d: first difference (array, index, got, want): %s" % (name, i, F.SEEDS[name], diff))
    for k in GC.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (name, i, F.SEEDS[name], k, diff)
    assert got["info"] == want["info"], (name, i, F.SEEDS[name], got["info"], want["info"])


@pytest.mark.parametrize("name,i", F.every())
def test_the_two_statements_agree(name, i):
    """gapped_full == gapped_banded.  On `long_reads` gapped_full is skipped for the reads above F.FULL_LIMIT = 200 nt (a full table of a
    1 024-nt part has a million cells): it runs on the case with those reads taken out, against gapped_banded on the same."""
    c, want, pl = F.case(name), F.checked(name, i), F.placed(name)
    v = dict(GC.DEFAULT, **c["variants"][i])
    if name == "long_reads":
        s = F.shortened(name)
        spl = P.place(s["rows"], s["lens"], None, *F.targets(s), **s["place"])
        short = GC.gapped_banded(s["rows"], s["lens"], spl, *F.targets(s), **s["variants"][i])
        assert short["info"]["tried"] == 2 and short["info"]["placed"] == 2
        assert_same(GC.gapped_full(s["rows"], s["lens"], spl, *F.targets(s), **s["variants"][i]), short, name, i)
        keep = [r for r in range(len(s["reads"])) if s["reads"][r] is not None]
        for k in ("target", "pos", "end", "edits", "state"):                     # a read's result does not depend on the other reads
            assert (short[k][keep] == want[k][keep]).all(), k
    else:
        assert_same(GC.gapped_full(c["rows"], c["lens"], pl, *F.targets(c), **c["variants"][i]), want, name, i)
    info = want["info"]
    assert (info["tried"], info["placed"], info["unique"], info["with_indel"], info["edits"]) == OUTCOMES[name][i], info
    GI.assert_invariants(c, pl, want, v)
    print(name, i, info)


def test_every_family_is_listed():
    assert sorted(OUTCOMES) == sorted(F.CASES) == sorted(F.SEEDS) and all(len(OUTCOMES[n]) == len(F.case(n)["variants"]) for n in F.CASES)


def _best(w, r):
    return int(w["edits"][r]), int(bool(w["state"][r] & GC.MINUS)), int(w["target"][r]), int(w["pos"][r])


def _has_rival(w, r, E):
    """a placement of read r at d + 1 that is another locus: another strand or target, or further than E from the best"""
    d, strand, t, p = _best(w, r)
    return any(x[0] == d + 1 and ((x[1], x[2]) != (strand, t) or abs(x[3] - p) > E) for x in w["found"][r])


def _E(name, i):
    return dict(GC.DEFAULT, **F.case(name)["variants"][i])["max_edits"]


def test_two_letter_has_many_candidates_a_read():
    for i in range(2):
        info = F.checked("two_letter", i)["info"]
        assert info["candidates"] >= 10 * info["tried"], info


@pytest.mark.parametrize("name", ["tandem", "duplicates"])
def test_ties_and_near_ties(name):
    w = F.checked(name)
    st = w["state"]
    assert ((st & (GC.PLACED | GC.UNIQUE)) == GC.PLACED).any()                               # placed and not UNIQUE: loci at equal d
    near = [r for r in range(len(st)) if st[r] & GC.UNIQUE and _has_rival(w, r, _E(name, 0))]
    assert near, "no UNIQUE read with a rival at d + 1"
    print(name, "UNIQUE with a rival at d + 1:", near)


def test_tandem_pure_repeats_on_both_sides_of_the_rule():
    """a read of PURE_LEN repeat bases in a target of PURE_LEN + x: at d = 0 from column 0 to the last multiple of the period <= x.  UNIQUE iff
    that is <= E: for x = E, not for x = E + 1, with period 1 and with period 2 (E = 3).  The repeat of TA reads the same on both strands: the
    same loci at d = 0 on either, reported +, not UNIQUE although x = E"""
    c, w = F.case("tandem"), F.checked("tandem")
    E, R, n_pure = _E("tandem", 0), len(w["state"]), len(F.PURE)
    assert E == 3 and [x for _, x in F.PURE] == [E, E + 1, E, E + 1, E] and [len(u) for u, _ in F.PURE] == [1, 1, 2, 2, 2]
    for n, (unit, x) in enumerate(F.PURE):
        r, t = R - 1 - n_pure + n, len(F.TANDEM_PERIODS) + n
        both = n == 4
        assert int(c["tlen"][t]) == F.PURE_LEN + x and int(c["lens"][2 * r + 1]) == F.PURE_LEN
        assert _best(w, r) == (0, 0, t, 0) and int(w["end"][r]) == F.PURE_LEN
        at0 = [fx for fx in w["found"][r] if fx[0] == 0]
        assert sorted({fx[3] for fx in at0}) == list(range(0, x + 1, len(unit))) and {fx[2] for fx in at0} == {t}
        assert {fx[1] for fx in at0} == ({0, 1} if both else {0}) and (not both or {fx[3] for fx in at0 if fx[1] == 1} == {0, 2})
        assert bool(w["state"][r] & GC.UNIQUE) == (x == E and not both), (unit, x)
    assert not F.placed("tandem")["state"][R - 1 - n_pure:].any()                             # the Hamming pass left them alone


def test_duplicates_equal_d_on_both_strands_is_reported_plus():
    w = F.checked("duplicates")
    both = [r for r in range(len(w["state"])) if w["state"][r] & GC.PLACED and {x[1] for x in w["found"][r] if x[0] == w["edits"][r]} == {0, 1}]
    assert len(both) >= 10 and all(not (w["state"][r] & (GC.MINUS | GC.UNIQUE)) for r in both)
    # ... although the minus locus lies on the lower target
    assert any(min(x[2] for x in w["found"][r] if x[0] == w["edits"][r] and x[1] == 1) < int(w["target"][r]) for r in both)
    # equal d on two targets through different scripts: a substitution on one, an inserted base on the other
    cg = GC.cigar_strings(w)
    r = 21
    assert w["state"][r] == GC.PLACED and cg[r] == "100M" and sorted({x[2] for x in w["found"][r] if x[0] == 1}) == [1, 2]


def test_long_reads_made_reads():
    c, w, pl = F.case("long_reads"), F.checked("long_reads"), F.placed("long_reads")
    v = dict(GC.DEFAULT, **c["variants"][0])
    k, index = v["k"], P._index(c["seqs"], v["k"])
    subs, broken, twin = F.LONG_MADE
    assert w["info"]["seeds"] == 2 * sum(int(L) // k for L in c["lens"][1::2]) and not pl["state"].any()
    usable = {}
    for r in F.LONG_MADE:
        assert int(c["lens"][2 * r + 1]) == GC.MAX_READ and GC.MAX_READ // k == 128                # 128 seeds per strand: two chunks of 64
        vals = P.kmer_values(P.codes_of(c["rows"][2 * r + 1], 0, GC.MAX_READ), k)[::k]
        usable[r] = [1 <= len(index.get(int(x), ())) <= v["max_occ"] for x in vals]
        assert len(vals) == 128
    cg = GC.cigar_strings(w)
    # three substitutions in chunk 0: placed, and no seed of chunk 1 counts at the true locus (each a duplicate through a usable seed of chunk 0)
    assert w["state"][subs] == GC.PLACED | GC.UNIQUE and cg[subs] == "1024M" and w["edits"][subs] == 3 and sum(usable[subs][:64]) >= 32 and all(usable[subs][64:])
    at = [x for x in w["found"][subs] if x[1:4] == _best(w, subs)[1:]]
    assert at and all(x[5] < 64 for x in at)
    # every seed of chunk 0 broken: not placed, although chunk 1 gives a candidate whose right part is exact
    assert w["state"][broken] == 0 and sum(usable[broken][64:]) >= 60
    # every seed of chunk 0 over max_occ: placed through chunk 1 alone
    assert not any(usable[twin][:64]) and all(len(index[int(x)]) > v["max_occ"] for x in P.kmer_values(P.codes_of(c["rows"][2 * twin + 1], 0, 512), k)[::k])
    assert w["state"][twin] & GC.PLACED and cg[twin] == "799M1D225M" and all(x[5] >= 64 for x in w["found"][twin]) and w["edits"][twin] <= v["max_edits"]


def test_every_family_places_on_both_strands_and_leaves_a_read():
    for name in FAMILIES:
        tried = [r for r in range(len(F.case(name)["lens"]) // 2) if GC.takes_part(F.placed(name), F.case(name)["lens"], r, dict(GC.DEFAULT, **F.case(name)["variants"][0])["k"])]
        for i in range(len(F.case(name)["variants"])):
            st = F.checked(name, i)["state"]
            on = (st & GC.PLACED) > 0
            assert (on & ((st & GC.MINUS) > 0)).any() and (on & ((st & GC.MINUS) == 0)).any(), (name, i)
            assert not on[tried].all(), (name, i)


def test_edits_and_scripts_over_all_families():
    edits, first, last = set(), set(), set()
    for name, i in F.every():
        w = F.checked(name, i)
        edits |= set(w["edits"][(w["state"] & GC.PLACED) > 0].tolist())
        for s in GC.cigar_strings(w):
            if s:
                first.add(s[s.index(next(ch for ch in s if ch in "MID"))])
                last.add(s[-1])
    assert edits >= set(range(1, 7)) and 15 in edits and 0 in edits, sorted(edits)
    assert "I" in first and "I" in last                                                      # (a script neither begins nor ends with D: the target's end is free)
    assert "D" not in first and "D" not in last
    # the best (d, strand, t, p, e) reached through more than one (j, q): the smallest gives the script
    for name in FAMILIES:
        w = F.checked(name)
        assert any(sum(x[:5] == min(f)[:5] for x in f) > 1 for f in w["found"] if f), name
    # the edges of `edges`: targets of k, k + 1, k + 3, k + 15 columns, both parts of a candidate empty, a read of insertions alone beside its seed
    c, cg = F.case("edges"), GC.cigar_strings(F.checked("edges"))
    assert c["tlen"].tolist() == [300, 8, 9, 11, 23] and cg[:6] == ["8M1I", "8I8M", "9M", "8M3I", "8I9M1I", "8M1D2M"] and cg[8] == "8M"
    assert "8M3D8M" in cg and "8M3I8M" in cg and "12M3I9M" in cg                            # a run of E = 3 behind a seed and before one
    w = F.checked("edges")
    assert max(len(w["cigar"][w["cigar_off"][r]:w["cigar_off"][r + 1]]) for r in range(len(cg)) if w["edits"][r] == 15) >= 15   # E = 15 in many runs
    over = [F.checked("edges", i)["info"]["seeds_over_max_occ"] for i in range(4)]
    assert over[0] == over[2] < over[1] == over[3]                                           # the 8-mer planted twice: usable at max_occ 2 alone
    assert F.checked("edges", 2)["info"]["placed"] > F.checked("edges", 1)["info"]["placed"]


def test_the_pool():
    g, pool = F._pool_reads()
    assert len(pool) == F.POOL >= 200 and F.POOL % 2 == 1 and math.gcd(F.POOL, 7) == 1 and (7 * 16384) % F.POOL != 0 and len({p.tobytes() for p in pool}) == F.POOL
    assert min(len(p) for p in pool) >= 30 and max(len(p) for p in pool) <= 150
    w, pl = F.checked("pool"), F.placed("pool")
    on = (w["state"] & GC.PLACED) > 0
    assert 3 <= pl["info"]["placed"] <= 10 and 20 <= w["info"]["tried"] - w["info"]["placed"] <= 80 and w["info"]["insertions"] > 20 and w["info"]["deletions"] > 20
    assert any(on[r - 1] and not on[r] and on[r + 1] for r in range(1, len(on) - 1))
    assert len({int(c) for c in F.case("pool")["lens"][1::2]}) > 50
