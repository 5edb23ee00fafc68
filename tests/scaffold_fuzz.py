"""Seeded families for the scaffold stage (tests/scaffold_checker.py is the definition), built on tests/scaffold_cases.py: random targets, reads
of 25 bases cut from them at planted reaches, so the links are known.  Each family is a function of a seed and returns the case dict of
scaffold_cases._make with `variants`, the placement written down in the checker's form (`written`: scaffold_cases.chunks() does the same; the
CPU file runs the Python placement over every case of at most 600 targets and the GPU file compares the device's placement first) and `truth`,
what the family planted.  Every size is the smallest at which the thing the family is for can go wrong:

  whole_chains    one chain through all T targets, T on and around the powers of two the jump rounds are derived from; 513 members in one record
  rings           rings of 2 .. 257 contigs, the smallest contig anywhere and entered through either end; four rings, chains and singletons together
  bundle_edges    bundles of 1 .. 1000 links whose starts in the sorted link array fall on many lanes, cross blocks, follow a long bundle in one wave
  wide_span       4 200 links of nearly 2^20 between two ends: the sum of the spans is above 2^32
  rivals          ends with up to 12 supported bundles, ties of three at the top, pairs exactly on and one link below every percentage
  many_targets    40 000 targets: a 50-bit sort key, joins between target 0 and the last, keys that differ in one high bit or in the lowest
  many_scaffolds  about 900 short chains in 3 000 targets: a FASTA of many small records

case(key) -> the case, checked(key, i) -> scaffold_dicts for variant i, both computed once.  KEYS lists the cases per family."""
import functools

import numpy as np

import place_checker as P
import scaffold_cases as QC
import scaffold_checker as SC

_rng, _seq = QC._rng, QC._seq
READ, L, R = QC.READ, QC.L, QC.R


def written(targets, links, extra=0):
    """the placement of the reads of `links` (and `extra` unpaired reads that lie at the start of target 0) as the placement checker returns it"""
    ends = [(x, d) for x1, d1, x2, d2 in links for x, d in ((x1, d1), (x2, d2))]
    tlen = np.array([len(t) for t in targets], dtype=np.int64)
    return dict(target=np.array([x >> 1 for x, _ in ends] + [0] * extra, np.int32),
                pos=np.array([tlen[x >> 1] - d if x & 1 else d - READ for x, d in ends] + [0] * extra, np.int32),
                state=np.array([P.PLACED | P.UNIQUE | (0 if x & 1 else P.MINUS) for x, _ in ends] + [P.PLACED | P.UNIQUE] * extra, np.uint8),
                col_off=np.concatenate([[0], np.cumsum(tlen)]).astype(np.uint32), info=dict(pairs_split=len(links)))


def _case(targets, links, truth, variants, extra=(), **kw):
    c = QC._make(targets, links, variants=variants, extra=extra, **kw)
    return dict(c, written=written(targets, links, len(extra)), truth=truth)


def _shuffled(rng, links):
    return [links[i] for i in rng.permutation(len(links))]


def from_smaller_terminal(chain):
    return chain if chain[0][0] <= chain[-1][0] else [(c, o ^ 1) for c, o in chain[::-1]]


# ---- whole_chains ----------------------------------------------------------------------------------------------------------------------------
CHAIN_T = (1, 2, 3, 4, 5, 127, 128, 129, 512, 513)


def whole_chains(seed, T, smaller_first):
    """truth: path, the one scaffold as [(contig, orient)] from its smaller terminal, and planted, the chain as the links were made.  smaller_first: the chain is planted beginning at that terminal,
    else ending at it (the device's two directions swap their roles)"""
    rng = _rng(seed)
    ids = [int(c) for c in rng.permutation(T)]
    if T > 1 and (ids[0] < ids[-1]) != smaller_first:
        ids[0], ids[-1] = ids[-1], ids[0]
    chain = [(c, int(rng.integers(0, 2))) for c in ids]
    if T == 1:
        chain = [(0, 0)]
    tg = [_seq(rng, 30 + int(rng.integers(0, 50))) for _ in range(T)]
    extra = [tg[0][:READ]] * 2 if T == 1 else ()                        # (a read set must not be empty for the links kernel to run at all)
    return _case(tg, _shuffled(rng, QC.chain_links(rng, tg, chain, 5)), dict(path=from_smaller_terminal(chain), planted=chain), (dict(insert=120),), extra=extra,
                 shifts=[7 * i % 16 for i in range(T)], gaps=[i % 3 != 1 for i in range(T)])


# ---- rings -----------------------------------------------------------------------------------------------------------------------------------
RING_M = (2, 3, 4, 5, 64, 65, 257)


def ring_links(rng, targets, ring, counts):
    links = []
    for k, ((c, o), (d, q)) in enumerate(zip(ring, ring[1:] + ring[:1])):
        links += QC.bundle(rng, targets, 2 * c + (o ^ 1), 2 * d + q, counts[k % len(counts)])
    return links


def rings(seed, m):
    """one ring of m contigs among m + 3 targets (one of them empty).  truth: rings = [[(contig, orient)]] in planted order, chains = []"""
    rng = _rng(seed)
    T = m + 3
    tg = [_seq(rng, 30 + int(rng.integers(0, 50))) for _ in range(T)]
    ids = [int(c) for c in rng.permutation(T)]
    tg[ids[m]] = _seq(rng, 0)
    ring = [(c, int(rng.integers(0, 2))) for c in ids[:m]]
    links = ring_links(rng, tg, ring, (5, 7, 6, 9, 8))
    return _case(tg, _shuffled(rng, links), dict(rings=[ring], chains=[]), (dict(insert=120), dict(insert=120, min_links=6)), shifts=[5 * i % 16 for i in range(T)])


MIXED_RINGS, MIXED_CHAINS = (2, 3, 5, 9), (4, 2, 7)


def mixed(seed):
    """four rings, three chains and nine singletons (three of them empty) side by side in shuffled ids"""
    rng = _rng(seed)
    T = sum(MIXED_RINGS) + sum(MIXED_CHAINS) + 9
    tg = [_seq(rng, 30 + int(rng.integers(0, 50))) for _ in range(T)]
    ids = [int(c) for c in rng.permutation(T)]
    for c in ids[-3:]:
        tg[c] = _seq(rng, 0)
    at, rr, cc, links = 0, [], [], []
    for m in MIXED_RINGS:
        rr.append([(c, int(rng.integers(0, 2))) for c in ids[at:at + m]])
        links += ring_links(rng, tg, rr[-1], (6, 5, 8))
        at += m
    for m in MIXED_CHAINS:
        cc.append([(c, int(rng.integers(0, 2))) for c in ids[at:at + m]])
        links += QC.chain_links(rng, tg, cc[-1], 5)
        at += m
    return _case(tg, _shuffled(rng, links), dict(rings=rr, chains=[from_smaller_terminal(x) for x in cc]), (dict(insert=120),), shifts=[11 * i % 16 for i in range(T)])


def opened(ring):
    """a planted ring as the path the definition leaves: the join at end 2c of its smallest contig c dropped, laid out from c
    -> the path, the dropped key (a, b)"""
    k = min(range(len(ring)), key=lambda i: ring[i][0])
    c, o = ring[k]
    if o == 0:                                                          # end 2c is where the ring enters c: the path runs on from c as planted
        path = ring[k:] + ring[:k]
        into = ring[k - 1]
        other = 2 * into[0] + (into[1] ^ 1)
    else:                                                               # end 2c is where the ring leaves c: the path runs backwards
        path = [(d, q ^ 1) for d, q in (ring[:k + 1][::-1] + ring[k + 1:][::-1])]
        into = ring[(k + 1) % len(ring)]
        other = 2 * into[0] + into[1]
    return path, (min(2 * c, other), max(2 * c, other))


# ---- bundle_edges ----------------------------------------------------------------------------------------------------------------------------
EDGE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
EDGE_MORE = (1, 1, 1, 2, 2, 63, 64, 65, 127, 129)                       # what the further bundles are drawn from
EDGE_BUNDLES, EDGE_TARGETS = 56, 12


def bundle_edges(seed):
    """12 targets, so two dozen ends; 56 bundles between them: every size of EDGE_SIZES once, the rest drawn from EDGE_MORE.  The keys are drawn
    and the sizes dealt to them in sorted order, so the seed decides where every bundle starts in the sorted link array (the CPU file asserts
    what that has to give).  truth: [(a, b, links)] ascending"""
    rng = _rng(seed)
    tg = [_seq(rng, 200) for _ in range(EDGE_TARGETS)]
    pairs = [(a, b) for a in range(2 * EDGE_TARGETS) for b in range(a + 1, 2 * EDGE_TARGETS) if a >> 1 != b >> 1]
    keys = sorted(pairs[i] for i in rng.choice(len(pairs), EDGE_BUNDLES, replace=False))
    sizes = list(EDGE_SIZES) + [EDGE_MORE[int(i)] for i in rng.integers(0, len(EDGE_MORE), EDGE_BUNDLES - len(EDGE_SIZES))]
    sizes = [sizes[i] for i in rng.permutation(EDGE_BUNDLES)]
    links = []
    for (a, b), n in zip(keys, sizes):
        links += QC.bundle(rng, tg, a, b, n)
    return _case(tg, _shuffled(rng, links), [(a, b, n) for (a, b), n in zip(keys, sizes)],
                 tuple(dict(insert=300, min_links=n) for n in (1, 64, 65, 1001)), shifts=[3 * i % 16 for i in range(EDGE_TARGETS)])


# ---- wide_span -------------------------------------------------------------------------------------------------------------------------------
WIDE_LINKS, WIDE_CUT = 4200, (1 << 20) - 1000


def wide_span(seed):
    """truth: the spans of the links"""
    rng = _rng(seed)
    tg = [_seq(rng, 600000), _seq(rng, 590000)]
    links, spans = [], []
    for i in range(WIDE_LINKS):
        s = (1 << 20) - int(rng.integers(0, 2001))
        d1 = int(rng.integers(460000, 588001))
        spans.append(s)
        links.append((2 * 0 + R, d1, 2 * 1 + L, s - d1) if i & 1 else (2 * 1 + L, s - d1, 2 * 0 + R, d1))
    return _case(tg, links, spans, (dict(insert=1 << 20, max_insert=1 << 20), dict(insert=1 << 20, max_insert=WIDE_CUT)), shifts=[9, 2])


# ---- rivals ----------------------------------------------------------------------------------------------------------------------------------
RIVAL_T, RIVAL_RANDOM_T, RIVAL_RANDOM = 200, 150, 330
# the planted hubs: the link counts of the bundles at one end, each to an end nothing else touches
RIVAL_HUBS = ((7, 7, 7, 3, 2), (9, 9, 9), (6, 6), (11, 11, 4), (12, 6), (12, 5), (10, 5), (10, 4), (6, 3), (6, 2), (5, 5, 5, 5), (6, 5), (100, 51), (100, 50), (100, 1),
              (100, 100, 99), tuple(range(1, 13)), (12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1))
RIVAL_VARIANTS = tuple(dict(insert=300, min_links=n, max_second_percent=p) for n in (1, 3, 5) for p in (1, 50, 51, 100))


def rivals(seed):
    """truth: [(hub end, its counts)]"""
    rng = _rng(seed)
    tg = [_seq(rng, 140 + int(rng.integers(0, 61))) for _ in range(RIVAL_T)]
    links, seen = [], set()
    while len(seen) < RIVAL_RANDOM:
        a, b = (int(x) for x in rng.integers(0, 2 * RIVAL_RANDOM_T, 2))
        if a >> 1 == b >> 1 or (min(a, b), max(a, b)) in seen:
            continue
        seen.add((min(a, b), max(a, b)))
        links += QC.bundle(rng, tg, a, b, int(rng.integers(1, 13)))
    free = [int(x) for x in rng.permutation(np.arange(2 * RIVAL_RANDOM_T, 2 * RIVAL_T))]
    hubs = []
    for counts in RIVAL_HUBS:
        hub = free.pop()
        hubs.append((hub, counts))
        for n in counts:
            leaf = next(x for x in free if x >> 1 != hub >> 1)
            free.remove(leaf)
            links += QC.bundle(rng, tg, hub, leaf, n)
    return _case(tg, _shuffled(rng, links), hubs, RIVAL_VARIANTS, shifts=[13 * i % 16 for i in range(RIVAL_T)])


# ---- many_targets ----------------------------------------------------------------------------------------------------------------------------
MANY_T, MANY_HIGH = 40000, 32768


def many_targets(seed):
    """every target t with t % 7 == 3 is empty.  truth: dict(chains, rings, far: the (a, b) between the first targets and the last, high: pairs of keys
    that differ in one bit above 2^15, low: pairs of keys that differ in the lowest bit)"""
    rng = _rng(seed)
    T = MANY_T
    tg = [_seq(rng, 0 if t % 7 == 3 else 30 + int(rng.integers(0, 31))) for t in range(T)]
    full = lambda t: t % 7 != 3
    pool = [int(t) for t in rng.permutation(np.arange(MANY_HIGH + 1, T - 2)) if full(int(t))]
    take = lambda n: [(pool.pop(), int(rng.integers(0, 2))) for _ in range(n)]
    chains, rr, links = [], [], []
    for _ in range(150):
        chains.append(take(int(rng.integers(2, 9))))
        links += QC.chain_links(rng, tg, chains[-1], 3)
    for m in (3, 4, 6):
        rr.append(take(m))
        links += ring_links(rng, tg, rr[-1], (3, 4))
    low = [int(t) for t in rng.permutation(np.arange(2, 16000)) if full(int(t))]
    rr.append([(low.pop(), 0), take(1)[0], (low.pop(), 1), take(1)[0], take(1)[0]])      # a ring through low and high ids
    links += ring_links(rng, tg, rr[-1], (4, 3))
    far = [(2 * 0 + R, 2 * (T - 1) + L), (2 * 0 + L, 2 * (T - 2) + R), (2 * 1 + R, 2 * (T - 1) + R)]      # the chain T-2, 0, T-1, 1
    for a, b in far:
        links += QC.bundle(rng, tg, a, b, 3)
    used = {0, 1, T - 2, T - 1} | {c for x in chains + rr for c, _ in x}
    high, lowbit = [], []
    for j in range(40):                                                 # (a, b) beside (a, b ^ bit), then beside (a ^ bit, b): bit 2^15 or 2^16
        while True:
            bit = 1 << int(rng.integers(15, 17))
            a = 2 * low.pop() + int(rng.integers(0, 2))
            if j % 2 == 0:
                b = (2 * low.pop() + int(rng.integers(0, 2))) | bit
                other = (a, b ^ bit)
            else:
                b = 2 * pool.pop() + int(rng.integers(0, 2))
                other = (a ^ bit, b)
            new = {a >> 1, b >> 1, other[0] >> 1, other[1] >> 1}
            if a < b and other[0] < other[1] and b < 2 * T and len(new) == 3 and all(full(t) for t in new) and not new & used:
                break
        used |= new
        high.append(((a, b), other))
        links += QC.bundle(rng, tg, a, b, 4) + QC.bundle(rng, tg, *other, 2)
    for _ in range(40):                                                 # one end joined to both ends of another target: 4 links against 1
        a, t = 2 * low.pop() + int(rng.integers(0, 2)), low.pop()
        k = ((a, 2 * t), (a, 2 * t + 1)) if a < 2 * t else ((2 * t, a), (2 * t + 1, a))
        lowbit.append(k)
        links += QC.bundle(rng, tg, *k[0], 4) + QC.bundle(rng, tg, *k[1], 1)
    truth = dict(chains=[from_smaller_terminal(x) for x in chains], rings=rr, far=far, high=high, low=lowbit)
    return _case(tg, _shuffled(rng, links), truth, (dict(insert=60, min_links=2), dict(insert=60, min_links=1, max_second_percent=100)),
                 shifts=[5 * i % 16 for i in range(T)], gaps=[i % 64 == 0 for i in range(T)])


# ---- many_scaffolds --------------------------------------------------------------------------------------------------------------------------
SCAF_T = 3000


def many_scaffolds(seed):
    """truth: the chains as [(contig, orient)] from their smaller terminal, singletons among them"""
    rng = _rng(seed)
    tg = [_seq(rng, 40 + int(rng.integers(0, 51))) for _ in range(SCAF_T)]
    ids = [int(c) for c in rng.permutation(SCAF_T)]
    chains, links = [], []
    while ids:
        m = min(len(ids), int(rng.integers(1, 7)))
        chain = [(ids.pop(), int(rng.integers(0, 2))) for _ in range(m)]
        if m == 1:
            chain = [(chain[0][0], 0)]
        chains.append(from_smaller_terminal(chain))
        links += QC.chain_links(rng, tg, chain, 2, hi=45)
    return _case(tg, _shuffled(rng, links), sorted(chains), (dict(insert=80, min_links=2), dict(insert=62, min_links=2, min_gap=3)),
                 shifts=[i % 16 for i in range(SCAF_T)], gaps=[i % 97 == 0 for i in range(SCAF_T)])


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
SEEDS = dict(whole_chains=1100, rings=1200, mixed=1290, bundle_edges=1309, wide_span=1400, rivals=1500, many_targets=1600, many_scaffolds=1700)
CASES = {}
for _j, _t in enumerate(CHAIN_T):
    CASES["whole_chains/%d/first" % _t] = functools.partial(whole_chains, SEEDS["whole_chains"] + 2 * _j, _t, True)
    CASES["whole_chains/%d/last" % _t] = functools.partial(whole_chains, SEEDS["whole_chains"] + 2 * _j + 1, _t, False)
for _j, _m in enumerate(RING_M):
    CASES["rings/%d" % _m] = functools.partial(rings, SEEDS["rings"] + _j, _m)
CASES["rings/mixed"] = functools.partial(mixed, SEEDS["mixed"])
for _n, _f in (("bundle_edges", bundle_edges), ("wide_span", wide_span), ("rivals", rivals), ("many_targets", many_targets), ("many_scaffolds", many_scaffolds)):
    CASES[_n] = functools.partial(_f, SEEDS[_n])
FAMILIES = ("whole_chains", "rings", "bundle_edges", "wide_span", "rivals", "many_targets", "many_scaffolds")
KEYS = {f: [k for k in CASES if k.split("/")[0] == f] for f in FAMILIES}
# scaffold_walk is run where it finishes in a few seconds; the three left to scaffold_dicts alone cost it minutes: it looks at every link for
# every bundle and at every supported bundle for every end (wide_span: 1.2 Mb of FASTA compared twice; many_targets: 40 000 walks; many_scaffolds:
# 2 100 bundles times 4 300 links)
WALKED = ("whole_chains", "rings", "bundle_edges", "rivals")
PLACE_MAX_T = 600                                                       # the Python placement is run up to this many targets


@functools.lru_cache(maxsize=None)
def case(key):
    return CASES[key]()


@functools.lru_cache(maxsize=None)
def checked(key, i=0):
    c = case(key)
    return SC.scaffold_dicts(*QC.scaffold_args(c, c["written"]), **c["variants"][i])


@functools.lru_cache(maxsize=None)
def fasta(key, i=0):
    return SC.fasta(checked(key, i), case(key)["seqs"])


def n_variants(key):
    """(written down, so that listing the cases builds none of them; the CPU file compares it with the cases)"""
    return 1 if key == "rings/mixed" else dict(whole_chains=1, rings=2, bundle_edges=4, wide_span=2, rivals=len(RIVAL_VARIANTS), many_targets=2, many_scaffolds=2)[key.split("/")[0]]


def every(families=FAMILIES):
    """(key, variant index) of all cases of the families"""
    return [(k, i) for f in families for k in KEYS[f] for i in range(n_variants(k))]
