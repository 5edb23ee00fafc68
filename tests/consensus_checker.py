"""Consensus sequences of the unitigs in plain Python / numpy: the DEFINITION the device code (alga_unitig_consensus_device) has to equal
byte for byte, stated twice.

consensus_literal   the reference's Contig::correctSnipsInContig (src/DataStructures/Contig.cpp:33-93) restated line for line: the list of
                    correctors with its swap-and-pop, the sentinel read, the `freqs` trimming (THR is a parameter here).
consensus_pileup    the same result from the definition in include/alga_amd.h: count every base of every path entry into its column, take
                    the smallest base with the largest count, cut the ends back to the first / last column with more than min_votes votes.

Both work on the result of tests/unitig_checker.py (or the device's, via Unitigs.to_host()): pair k, its path entries (node, position)."""
import numpy as np


def consensus_literal(contained, thr=3):
    """contained: list of (codes of the read, offset to the PREVIOUS read) as Contig::containedReads holds them (the first offset is not
    read).  -> (untrimmed codes as a list, freqs, p, q): the contig is s[p : q + 1]."""
    contained = [(list(map(int, r)), int(o)) for r, o in contained]
    s = []
    correctors = [[contained[0][0], 0]]                                        # correctors.emplace_back(containedReads[0].first, 0)
    contained.append(([], len(contained[-1][0])))                             # the sentinel: any read, offset = size of the last one
    freqs = []
    for i in range(1, len(contained)):
        offset = contained[i][1]
        while offset > 0:
            offset -= 1
            most = [0, 0, 0, 0]
            k = len(correctors) - 1
            while k >= 0:                                                     # for (int k = correctors.size() - 1; k >= 0; k--)
                r, ind = correctors[k]
                if ind >= len(r):
                    correctors[k], correctors[-1] = correctors[-1], correctors[k]
                    correctors.pop()
                    k -= 1
                    continue
                correctors[k][1] += 1
                most[r[ind]] += 1
                k -= 1
            best = max(most)
            freqs.append(best)                                                # *max_element
            s.append(most.index(best))                                        # it - mostFrequent.begin(): the first of the largest
        if i < len(contained) - 1:
            correctors.append([contained[i][0], 0])
    contained.pop()
    p, q = 0, len(freqs) - 1
    while p <= q and freqs[p] <= thr:
        p += 1
    while p <= q and freqs[q] <= thr:
        q -= 1
    return s, freqs, p, q


def pack_ragged(flat_codes):
    """codes per column (laid out at 16 * word_off[k] + j, zeros elsewhere) -> packed words"""
    flat = np.asarray(flat_codes, dtype=np.uint64).reshape(-1, 16)
    return (flat << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)


def _unpack_columns(words):
    w = np.asarray(words, dtype=np.uint32)
    return ((w[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & np.uint32(3)).reshape(-1).astype(np.int64)


def _result(P, words, trim, length, changed, votes, ulen):
    return dict(n_pairs=P, words=words, trim_left=np.asarray(trim, dtype=np.int32), len=np.asarray(length, dtype=np.int32),
               changed=np.asarray(changed, dtype=np.int32), votes=votes,
               info=dict(pairs=P, pairs_kept=int((np.asarray(length) > 0).sum()), columns=int(np.asarray(ulen, dtype=np.int64).sum()),
                         trimmed_bases=int(np.asarray(length, dtype=np.int64).sum()), changed=int(np.asarray(changed, dtype=np.int64).sum())))


def consensus_pileup(words, lens, u, min_votes=3):
    """The definition, vectorised.  u: a unitig result (dict).  -> dict(words uint32 [total words] in u's ragged layout, trim_left / len /
    changed int32 [n_pairs], votes uint8 [16 * total words] saturated at 255, info)."""
    if min_votes < 0:
        raise ValueError("min_votes must not be negative")
    words = np.ascontiguousarray(words, dtype=np.uint32)
    lens64 = np.asarray(lens, dtype=np.int64)
    if len(lens64) % 2:
        raise ValueError("the node count must be even")
    P = int(u["n_pairs"])
    wo = np.asarray(u["word_off"]).astype(np.int64)
    po = np.asarray(u["path_off"]).astype(np.int64)
    pn = np.asarray(u["path_node"]).astype(np.int64)
    pp = np.asarray(u["path_pos"]).astype(np.int64)
    ulen = np.asarray(u["len"]).astype(np.int64)
    if len(pn) and (pn.max() >= len(lens64) or pn.min() < 0):
        raise ValueError("a path node is outside [0, n)")
    total = int(wo[-1]) * 16 if P else 0
    cnt = np.zeros(total * 4, dtype=np.int64)
    if len(pn):
        pair_of_entry = np.repeat(np.arange(P), np.diff(po))
        el = lens64[pn]
        for s0 in range(0, len(pn), 1 << 16):                                  # in slabs: bounded memory on the large cases
            sl = slice(s0, min(len(pn), s0 + (1 << 16)))
            ent = np.repeat(np.arange(sl.start, sl.stop), el[sl])
            start = np.cumsum(el[sl]) - el[sl]
            q = np.arange(len(ent)) - np.repeat(start, el[sl])
            code = ((words[pn[ent], q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & np.uint32(3)).astype(np.int64)
            col = wo[pair_of_entry[ent]] * 16 + pp[ent] + q
            cnt += np.bincount(col * 4 + code, minlength=total * 4)
    cnt = cnt.reshape(-1, 4)
    base = cnt.argmax(axis=1)                                                  # the first of the largest = the smallest code
    best = cnt.max(axis=1) if total else np.zeros(0, dtype=np.int64)
    packed = pack_ragged(base) if total else np.zeros(0, dtype=np.uint32)
    spelled = _unpack_columns(u["words"]) if total else np.zeros(0, dtype=np.int64)
    trim, length, changed = [], [], []
    for k in range(P):
        a = int(wo[k]) * 16
        L = int(ulen[k])
        assert (cnt[a:a + L].sum(axis=1) > 0).all(), "a column no read covers"
        ok = np.nonzero(best[a:a + L] > min_votes)[0]
        trim.append(int(ok[0]) if len(ok) else 0)
        length.append(int(ok[-1] - ok[0] + 1) if len(ok) else 0)
        changed.append(int((base[a:a + L] != spelled[a:a + L]).sum()))
    return _result(P, packed, trim, length, changed, np.minimum(best, 255).astype(np.uint8), ulen)


def contained_reads(words, lens, u, k):
    """Pair k as Contig::containedReads: (codes, offset to the previous read) per path entry"""
    rows = np.ascontiguousarray(words, dtype=np.uint32)
    po = np.asarray(u["path_off"]).astype(np.int64)
    out, prev = [], 0
    for i in range(int(po[k]), int(po[k + 1])):
        v, p = int(u["path_node"][i]), int(u["path_pos"][i])
        q = np.arange(int(lens[v]))
        out.append((((rows[v, q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & 3).astype(np.uint8), p - prev))
        prev = p
    return out


def consensus_by_the_literal_form(words, lens, u, min_votes=3):
    """consensus_literal on every pair, in the shape consensus_pileup returns (small inputs: a Python loop per column and read)"""
    P = int(u["n_pairs"])
    wo = np.asarray(u["word_off"]).astype(np.int64)
    total = int(wo[-1]) * 16 if P else 0
    flat = np.zeros(total, dtype=np.int64)
    votes = np.zeros(total, dtype=np.int64)
    spelled = _unpack_columns(u["words"]) if total else np.zeros(0, dtype=np.int64)
    trim, length, changed = [], [], []
    for k in range(P):
        s, freqs, p, q = consensus_literal(contained_reads(words, lens, u, k), min_votes)
        L = int(u["len"][k])
        assert len(s) == L
        a = int(wo[k]) * 16
        flat[a:a + L] = s
        votes[a:a + L] = freqs
        trim.append(p if q >= p else 0)
        length.append(q - p + 1 if q >= p else 0)
        changed.append(int((flat[a:a + L] != spelled[a:a + L]).sum()))
    packed = pack_ragged(flat) if total else np.zeros(0, dtype=np.uint32)
    return _result(P, packed, trim, length, changed, np.minimum(votes, 255).astype(np.uint8), u["len"])


def window(u, cons, k):
    """ACGT string of pair k's trimmed consensus"""
    wo = np.asarray(u["word_off"]).astype(np.int64)
    w = np.asarray(cons["words"])[wo[k]: wo[k + 1]]
    q = int(cons["trim_left"][k]) + np.arange(int(cons["len"][k]))
    return "".join("ACGT"[c] for c in ((w[q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & 3))


def fasta_bytes(u, cons, min_length=200):
    """The text of alga_write_consensus_fasta_device and its record count"""
    out, n = [], 0
    for k in range(int(u["n_pairs"])):
        L = int(cons["len"][k])
        if L > 0 and L >= min_length:
            out.append(">unitig_%d_length=%d\n%s\n" % (k, L, window(u, cons, k)))
            n += 1
    return "".join(out).encode(), n


def consensus_rows(u, cons):
    """A copy of the unitig result whose rows are the untrimmed consensus (what tests/gfa_writer.py takes via unitig_checker.padded_rows)"""
    v = dict(u)
    v["words"] = np.asarray(cons["words"], dtype=np.uint32)
    return v


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))

