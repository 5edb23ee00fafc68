"""Seeded cases of the containment stage (include/alga_amd.h: alga_drop_contained_device), each made for one outcome.  Target i begins at base
offset 3 i mod 16 of the packed array.  A case is a dict: seqs (code arrays), twords / tbegin / tlen, variants (parameter dicts), and expect:
per variant {target: None (kept) or (host, pos, orient, mm, hits)} for the targets the case is about -- what tests/test_contain_cpu.py asserts of
the checker's output and tests/test_gpu_contain.py, through the checker, of the device's."""
import functools

import numpy as np

import contain_checker as CC
import place_checker as P


def _rng(seed):
    return np.random.default_rng(seed)


def _seq(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def _sub(c, positions):
    c = np.array(c, dtype=np.uint8, copy=True)
    for p in positions:
        c[p] = (c[p] + 1) & 3
    return c


def _make(targets, variants, expect, **extra):
    targets = [np.asarray(t, np.uint8) for t in targets]
    twords, tbegin, tlen = P.ragged(targets, [3 * i % 16 for i in range(len(targets))])
    assert len(expect) == len(variants)
    return dict(extra, seqs=targets, twords=twords, tbegin=tbegin, tlen=tlen, variants=variants, expect=expect)


def _word_edges():
    """n mod 16 in 0, 1, 15; p = 0, p = len[h] - n (flush right: the host's last word is followed by the padding), p mod 16 = 1 and 15"""
    rng = _rng(401)
    t, exp = [], {}
    for n in (64, 65, 79):
        for kind in range(4):
            L = 200 + 7 * kind + n % 16
            p = (0, L - n, 33, 47)[kind]
            h = _seq(rng, L)
            exp[len(t)] = None
            exp[len(t) + 1] = (len(t), p, 0, 0, 1)
            t += [h, h[p:p + n]]
    return _make(t, [dict()], [exp])


PASS_N = (1023, 1024, 1025, 2049)


def _pass_edges():
    """n = 1023, 1024, 1025, 2049 bases: less than one cooperative pass of 64 words, exactly one, two, three.  The only mismatch lies in the
    last word of the query (behind every seed): contained at the default, not at max_permille 0"""
    rng = _rng(402)
    t, e0, e1 = [], {}, {}
    for i, n in enumerate(PASS_N):
        h = _seq(rng, n + 40 + i)
        p = 19 + i
        e0[len(t) + 1] = (len(t), p, 0, 1, 1)
        e1[len(t) + 1] = None
        t += [h, _sub(h[p:p + n], [n - 1])]
    return _make(t, [dict(), dict(max_permille=0)], [e0, e1])


def _permille():
    """M(99) = 0 and M(100) = 1 at 10 per mille: n = 99 with one mismatch is kept, n = 100 with one is contained, n = 100 with two is kept; an
    exact n = 99 is contained whatever the bound"""
    rng = _rng(403)
    h = [_seq(rng, 300 + i) for i in range(4)]
    t = h + [_sub(h[0][50:149], [90]), _sub(h[1][60:160], [95]), _sub(h[2][70:170], [90, 97]), h[3][80:179]]
    e0 = {4: None, 5: (1, 60, 0, 1, 1), 6: None, 7: (3, 80, 0, 0, 1)}
    e1 = {4: None, 5: None, 6: None, 7: (3, 80, 0, 0, 1)}
    return _make(t, [dict(), dict(max_permille=0)], [e0, e1])


def _first_last_base():
    """n = 150 (M = 1; a partial last word): the only mismatch in base 0, or in base n - 1, is counted (max_permille 0 keeps the target); the
    bases just outside the interval differ from the padding of the query row and are not compared (the exact window is contained)"""
    rng = _rng(404)
    h = [_seq(rng, 400 + i) for i in range(3)]
    for x in h:                                              # the bases around the interval are not A: the query row has zeros there
        x[99], x[250] = 2, 1
    t = h + [_sub(h[0][100:250], [0]), _sub(h[1][100:250], [149]), h[2][100:250]]
    e0 = {3: (0, 100, 0, 1, 1), 4: (1, 100, 0, 1, 1), 5: (2, 100, 0, 0, 1)}
    e1 = {3: None, 4: None, 5: (2, 100, 0, 0, 1)}
    return _make(t, [dict(), dict(max_permille=0)], [e0, e1])


def _minus():
    """the reverse complement of a window is contained with orientation 1; a palindromic target alone has no container (h != c)"""
    rng = _rng(405)
    h = _seq(rng, 500)
    x = _seq(rng, 60)
    pal = np.concatenate([x, P.revcomp(x)])
    assert (pal == P.revcomp(pal)).all()
    return _make([h, P.revcomp(h[123:323]), pal], [dict()], [{0: None, 1: (0, 123, 1, 0, 1), 2: None}])


def _duplicates():
    """three equal targets and one equal to their reverse complement behind an unrelated one: the smallest id is kept, the hosts run by (mm, h)"""
    rng = _rng(406)
    a = _seq(rng, 333)
    return _make([_seq(rng, 200), a, P.revcomp(a), a, a], [dict()], [{0: None, 1: None, 2: (1, 0, 1, 0, 1), 3: (1, 0, 0, 0, 2), 4: (1, 0, 0, 0, 3)}])


CHAIN_DEPTHS = tuple(range(1, 10)) + (33,)
CHAIN_CORE = 110


def _nest(rng, depth):
    """member 0 is the outermost; member i + 1 is a window of member i with ONE substitution, in either orientation.  The substitutions lie at
    distinct bases of the innermost member, so a member has i mismatches against its ancestor i levels up: its best container is its parent
    (mm 1), and the innermost is far outside M of the root"""
    cur = _seq(rng, CHAIN_CORE)
    off, orient = 0, 0                                       # where the innermost member lies in `cur`
    out = [cur]
    for lvl in range(depth):
        q = 5 + 3 * lvl
        child = _sub(cur, [off + q if orient == 0 else off + CHAIN_CORE - 1 - q])
        left, right = 3 + lvl % 5, 2 + lvl % 3
        if rng.integers(0, 2):
            child = P.revcomp(child)
            off, orient = len(cur) - off - CHAIN_CORE, orient ^ 1
        cur = np.concatenate([_seq(rng, left), child, _seq(rng, right)])
        off += left
        out.append(cur)
    return out[::-1]


def _chain():
    """nests of depth 1 .. 9 and one of 33, mixed orientations, ids shuffled: root, root_pos and root_orient against the walk"""
    rng = _rng(407)
    members = [(d, i, s) for d in CHAIN_DEPTHS for i, s in enumerate(_nest(rng, d))]
    order = rng.permutation(len(members))
    t = [members[j][2] for j in order]
    where = {(members[j][0], members[j][1]): c for c, j in enumerate(order)}
    return _make(t, [dict()], [{where[(d, 0)]: None for d in CHAIN_DEPTHS}], where=where)


def _seed63():
    """n = 6400, k = 21: 64 seeds over the first 1344 bases, M = 64.  63 mismatches, one in each of seeds 0 .. 62: found through seed 63 only.
    With a 64th in seed 63 the Hamming bound still holds and no seed finds it: not a container"""
    rng = _rng(408)
    h, h2 = _seq(rng, 6500), _seq(rng, 6480)                  # a host each: the second query would else lie in the first
    subs = [21 * j + 10 for j in range(63)]
    return _make([h, _sub(h[37:6437], subs), h2, _sub(h2[41:6441], subs + [21 * 63 + 4])], [dict()], [{0: None, 1: (0, 37, 0, 63, 1), 2: None, 3: None}])


def _one_hit():
    """a perfect containment that all 64 seeds find counts once"""
    rng = _rng(409)
    h = _seq(rng, 1700)
    return _make([h[150:1550], h], [dict()], [{0: (1, 150, 0, 0, 1), 1: None}])


def _repeats():
    """a 40-base AT query inside a 600-base AT host at k = 8: 281 placements in each orientation; at max_occ 4 every seed is over"""
    at = np.tile(np.array([0, 3], np.uint8), 300)
    return _make([at[:40], at], [dict(k=8, max_occ=1000), dict(k=8, max_occ=4)], [{0: (1, 0, 0, 0, 255), 1: None}, {0: None, 1: None}])


def _two_hosts():
    """the best container by mm, then h, then p, then s"""
    rng = _rng(410)
    q = [_seq(rng, 120) for _ in range(3)]
    x = _seq(rng, 60)
    pal = np.concatenate([x, P.revcomp(x)])
    wrap = lambda s, a, b: np.concatenate([_seq(rng, a), s, _seq(rng, b)])
    t = [wrap(_sub(q[0], [100]), 30, 40), wrap(q[0], 50, 20),                # 0, 1: mm 1 in the smaller id, mm 0 in the larger
         wrap(q[1], 10, 90), wrap(q[1], 70, 30),                             # 2, 3: both exact
         np.concatenate([_seq(rng, 25), q[2], _seq(rng, 33), q[2], _seq(rng, 8)]),   # 4: twice in one host
         wrap(pal, 44, 41),                                                  # 5: a palindrome, in both orientations at one p
         q[0], q[1], q[2], pal]
    return _make(t, [dict()], [{6: (1, 50, 0, 0, 2), 7: (2, 10, 0, 0, 2), 8: (4, 25, 0, 0, 2), 9: (5, 44, 0, 0, 2)}])


def _short():
    """n < k has no container and is kept; n = k has one seed; a target of length 0 is neither kept nor contained"""
    rng = _rng(411)
    h = _seq(rng, 300)
    return _make([h, h[40:60], h[100:121], np.zeros(0, np.uint8), _seq(rng, 1)], [dict()], [{0: None, 1: None, 2: (0, 100, 0, 0, 1), 4: None}])


def _t0():
    return _make([], [dict()], [{}])


def _all_empty():
    return _make([np.zeros(0, np.uint8)] * 3, [dict()], [{}])


def _one():
    return _make([_seq(_rng(412), 333)], [dict()], [{0: None}])


def _word_seams():
    """k_ct_build at its seams: kept targets of 1, 15, 16, 17, 31, 32 and 33 bases around a host of 4200 whose window of 300 is dropped, an empty
    target between them; 4345 kept columns (no multiple of 16: the last word is partial, the two behind it are padding; 274 words: with
    contain_max_blocks 1 every lane takes two).  An empty target is not kept: the kept set has no empty item"""
    rng = _rng(414)
    h = _seq(rng, 4200)
    t = [_seq(rng, n) for n in (1, 15, 16)] + [_seq(rng, 0), _seq(rng, 17), h, h[1000:1300]] + [_seq(rng, n) for n in (31, 32, 33)]
    return _make(t, [dict()], [{**{i: None for i in (0, 1, 2, 4, 5, 7, 8, 9)}, 6: (5, 1000, 0, 0, 1)}])


CASES = {"word_seams": _word_seams, "word_edges": _word_edges, "pass_edges": _pass_edges, "permille": _permille, "first_last_base": _first_last_base, "minus": _minus, "duplicates": _duplicates,
         "chain": _chain, "seed63": _seed63, "one_hit": _one_hit, "repeats": _repeats, "two_hosts": _two_hosts, "short": _short, "t0": _t0, "all_empty": _all_empty,
         "one": _one}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def every():
    return [(n, i) for n in sorted(CASES) for i in range(len(case(n)["variants"]))]


def targets(c):
    return c["twords"], c["tbegin"], c["tlen"]


@functools.lru_cache(maxsize=None)
def checked(name, i=0):
    c = case(name)
    return CC.contain_index(c["seqs"], **c["variants"][i])


@functools.lru_cache(maxsize=None)
def many_queries(n):
    """n targets: every 16th is a window of 40 bases of the target before it, in either orientation, the others are unrelated and 50 .. 59 bases
    long.  Not in CASES: the GPU test sizes n by the device, so that a wave of k_ct_contain takes a second (c, s)"""
    rng = _rng(413)
    t = []
    while len(t) < n:
        i = len(t)
        if i % 16 == 15:
            w = t[-1][5:45]
            t.append(P.revcomp(w) if (i // 16) % 2 else w)
        else:
            t.append(_seq(rng, 50 + i % 10))
    return _make(t, [dict()], [{}])


def next_round(kept):
    """the case whose targets are the kept contigs"""
    return _make(CC.sequences(kept), [dict()], [{}])
