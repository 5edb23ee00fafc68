"""The definition of the grow stage (include/alga_amd.h: alga_grow_placed_device), twice, in Python.

grow_index() finds the overhang placements through a dictionary of the indexed k-mers of the end sequences and the seeds of the nodes, adds the
votes to the count array one by one and walks the columns of an end.  grow_bruteforce() walks every (node, e, h) literally, looks at the seeds
afterwards, counts the votes of an end from the list of its voters and takes the decision from whole arrays.  They share the refusals and the
packing of bases, nothing else; neither sorts placements, and neither shares anything with the device's method: no column space of the
ends, no keys, no directory.
Both take a placement as tests/place_checker.py returns it (state, col_off) and the bases of the placed targets as code arrays (the targets,
or the polished sequences)."""
import collections

import numpy as np

import place_checker as P
import scaffold_checker as SC

OVERHANGS, VOTES, MINUS = 1, 2, 4
ARRAYS = ("end", "over", "mm", "hits", "state", "count", "e_stop", "e_voters", "left", "right", "len", "col_off", "begin", "words")
COUNTERS = ("candidates", "overhanging", "voting", "multi", "hits_saturated", "seeds", "seeds_over_max_occ", "index_positions", "ends_with_voters", "ends_grown",
            "bases_added", "longest_growth", "stops_cover", "stops_percent", "stops_max", "columns_before", "columns_after", "n50_before", "n50_after")
DEFAULT = dict(k=21, max_mismatches=2, max_occ=256, min_anchor=63, min_cover=3, min_percent=80, max_grow=64)


def check(rows, lens, pl, seqs, k, max_mismatches, max_occ, min_anchor, min_cover, min_percent, max_grow):
    """the refusals"""
    if not 8 <= k <= 31 or not 0 <= max_mismatches <= 254 or not 1 <= max_occ <= 65535 or not k <= min_anchor <= 1 << 20 or not 1 <= min_cover <= 2 ** 31 - 1 or \
            not 51 <= min_percent <= 100 or not 1 <= max_grow <= 4096:
        raise ValueError("parameter out of range")
    n = len(lens)
    if n % 2 or n // 2 != len(pl["state"]):
        raise ValueError("not the node set that was placed")
    stride = rows.shape[1] if n else 0
    for r in range(n // 2):
        L = int(lens[2 * r])
        if L != lens[2 * r + 1] or L > 16 * stride:
            raise ValueError("twin lengths")
        if L > 0 and (P.pack(P.revcomp(P.codes_of(rows[2 * r + 1], 0, L)), stride)[:P.blocks_of(L)] != rows[2 * r][:P.blocks_of(L)]).any():
            raise ValueError("row 2r is not the reverse complement of row 2r + 1")
    if len(pl["col_off"]) != len(seqs) + 1 or int(pl["col_off"][-1]) != sum(len(s) for s in seqs):
        raise ValueError("n_columns is not col_off[n_targets]")
    if 2 * len(seqs) * max_grow > 1 << 30:
        raise OverflowError("2 T max_grow > 2^30")


def column_words(seqs):
    """the sequences one behind the other in column space: column g in word g >> 4 at bits 2 * (g & 15), two words of padding"""
    c = np.concatenate([np.asarray(s, np.uint32) for s in seqs] + [np.zeros(0, np.uint32)])
    words = np.zeros((len(c) + 15) // 16 + 2, dtype=np.uint32)
    i = np.arange(len(c), dtype=np.int64)
    np.bitwise_or.at(words, i >> 4, c << ((i & 15) << 1).astype(np.uint32))
    return words


def grow_index(rows, lens, pl, seqs, **params):
    """the definition with a dictionary index: the placements are the occurrences of the usable seeds"""
    p = dict(DEFAULT, **params)
    check(rows, lens, pl, seqs, **p)
    k, max_mm, max_occ, min_anchor, min_cover, min_percent, max_grow = (p[x] for x in ("k", "max_mismatches", "max_occ", "min_anchor", "min_cover", "min_percent", "max_grow"))
    R, T = len(lens) // 2, len(seqs)
    seqs = [np.asarray(s, np.uint8) for s in seqs]
    Lmax = max([int(x) for x in lens if x > 0] + [0])
    ends = []
    for s in seqs:
        W = max(0, min(len(s), Lmax - 1))
        ends += [P.revcomp(s[:W]), s[len(s) - W:]]
    index = collections.defaultdict(list)
    for e, E in enumerate(ends):
        for q, x in enumerate(P.kmer_values(E, k)):
            index[int(x)].append((e, q))
    info = dict.fromkeys(COUNTERS, 0)
    info["index_positions"] = sum(len(v) for v in index.values())
    out = dict(end=np.full(R, -1, np.int32), over=np.zeros(R, np.int32), mm=np.zeros(R, np.uint8), hits=np.zeros(R, np.uint8), state=np.zeros(R, np.uint8),
               count=np.zeros(2 * T * max_grow * 4, np.uint32), e_stop=np.zeros(2 * T, np.uint8), e_voters=np.zeros(2 * T, np.uint32))
    for r in range(R):
        L = int(lens[2 * r + 1])
        if int(pl["state"][r]) & P.PLACED or L < min_anchor + 1:
            continue
        info["candidates"] += 1
        found = set()
        codes = {}
        for strand, v in ((0, 2 * r + 1), (1, 2 * r)):
            c = codes[strand] = P.codes_of(rows[v], 0, L)
            for j, x in enumerate(P.kmer_values(c, k)[::k]):
                if (j + 1) * k > L - 1:                                   # a seed of no anchored part: a <= L - 1
                    break
                info["seeds"] += 1
                at = index.get(int(x), ())
                info["seeds_over_max_occ"] += len(at) > max_occ
                if not 1 <= len(at) <= max_occ:
                    continue
                for e, q in at:
                    W = len(ends[e])
                    a = W - q + j * k                                      # v[jk] lies on E[q], v[a] behind the end
                    h = L - a
                    if h < 1 or a < min_anchor or a > W:
                        continue
                    mm = int((c[:a] != ends[e][W - a:]).sum())
                    if mm <= max_mm:
                        found.add((mm, e, h, strand))
        if not found:
            continue
        best = min(found)
        hits = sum(1 for x in found if x[0] == best[0])
        mm, e, h, strand = best
        out["end"][r], out["over"][r], out["mm"][r], out["hits"][r] = e, h, mm, min(hits, 255)
        out["state"][r] = OVERHANGS | (VOTES if hits == 1 else 0) | (MINUS if strand else 0)
        info["overhanging"] += 1
        info["hits_saturated"] += hits > 255
        if hits == 1:
            info["voting"] += 1
            out["e_voters"][e] += 1
            c = codes[strand]
            for i in range(min(h, max_grow)):
                out["count"][(e * max_grow + i) * 4 + int(c[L - h + i])] += 1
    info["multi"] = info["overhanging"] - info["voting"]
    # the decision, column by column
    grown = []
    for e in range(2 * T):
        g, stop = [], 2
        for i in range(max_grow):
            cnt = [int(x) for x in out["count"][(e * max_grow + i) * 4:(e * max_grow + i) * 4 + 4]]
            cover, w = sum(cnt), cnt.index(max(cnt))
            if cover < min_cover:
                stop = 0
                break
            if 100 * cnt[w] < min_percent * cover:
                stop = 1
                break
            g.append(w)
        grown.append(np.array(g, np.uint8))
        out["e_stop"][e] = stop
        info[("stops_cover", "stops_percent", "stops_max")[stop]] += 1
        info["ends_with_voters"] += out["e_voters"][e] > 0
        info["ends_grown"] += len(g) > 0
        info["bases_added"] += len(g)
        info["longest_growth"] = max(info["longest_growth"], len(g))
    new = [np.concatenate([P.revcomp(grown[2 * t]), seqs[t], grown[2 * t + 1]]).astype(np.uint8) for t in range(T)]
    out["left"] = np.array([len(grown[2 * t]) for t in range(T)], np.uint32)
    out["right"] = np.array([len(grown[2 * t + 1]) for t in range(T)], np.uint32)
    out["len"] = np.array([len(s) for s in new], np.int32)
    out["col_off"] = np.concatenate([[0], np.cumsum(out["len"].astype(np.int64))]).astype(np.uint32)
    out["begin"] = out["col_off"][:-1].astype(np.uint64)
    out["words"] = column_words(new)
    info["columns_before"], info["columns_after"] = sum(len(s) for s in seqs), sum(len(s) for s in new)
    if info["columns_after"] > 2 ** 32 - 2:
        raise OverflowError("more than 2^32 - 2 new columns")
    info["n50_before"], info["n50_after"] = SC.n50([len(s) for s in seqs]), SC.n50([len(s) for s in new])
    out["info"] = {k_: int(v) for k_, v in info.items()}
    return out


def grow_bruteforce(rows, lens, pl, seqs, **params):
    """the definition walked literally: every (node, e, h), the Hamming distance first, then whether a usable seed matches there; the votes
    of an end from the list of its voters"""
    p = dict(DEFAULT, **params)
    check(rows, lens, pl, seqs, **p)
    k, max_grow = p["k"], p["max_grow"]
    R, T = len(lens) // 2, len(seqs)
    longest = 0
    for x in lens:
        longest = max(longest, int(x))
    E = []                                                                 # E[e]: the end sequence with the contig end at the right
    for t in range(T):
        s = np.asarray(seqs[t], np.uint8)
        W = min(len(s), longest - 1) if longest >= 1 else 0
        E.append((3 - s[:W])[::-1])
        E.append(s[len(s) - W:] if W else s[:0])
    occ = collections.Counter()
    for x in E:
        occ.update(int(v) for v in P.kmer_values(x, k))
    res = dict(end=[], over=[], mm=[], hits=[], state=[])
    voters = [[] for _ in range(2 * T)]                                    # per end: (the overhanging bases of a voter)
    n_cand = n_seeds = n_over = n_sat = 0
    for r in range(R):
        L = int(lens[2 * r + 1])
        best, n_best = None, 0
        if not int(pl["state"][r]) & P.PLACED and L >= p["min_anchor"] + 1:
            n_cand += 1
            for strand in (0, 1):
                c = P.codes_of(rows[2 * r + 1 - strand], 0, L)
                seeds = [int(x) for x in P.kmer_values(c[:L - 1], k)[::k]]  # the seeds that fit the longest anchored part
                n_seeds += len(seeds)
                n_over += sum(occ[x] > p["max_occ"] for x in seeds)
                usable = [1 <= occ[x] <= p["max_occ"] for x in seeds]
                for e in range(2 * T):
                    W = len(E[e])
                    for h in range(1, L - p["min_anchor"] + 1):
                        a = L - h
                        if a > W:
                            continue
                        diff = c[:a] != E[e][W - a:]
                        mm = int(diff.sum())
                        if mm > p["max_mismatches"]:
                            continue
                        if not any(usable[j] and not diff[j * k:j * k + k].any() for j in range(a // k)):
                            continue
                        key = (mm, e, h, strand)
                        if best is None or mm < best[0]:
                            best, n_best = key, 1
                        else:
                            n_best += mm == best[0]
                            best = key if key < best else best
        if best is None:
            for key, v in (("end", -1), ("over", 0), ("mm", 0), ("hits", 0), ("state", 0)):
                res[key].append(v)
            continue
        mm, e, h, strand = best
        n_sat += n_best > 255
        res["end"].append(e); res["over"].append(h); res["mm"].append(mm); res["hits"].append(min(n_best, 255))
        res["state"].append(OVERHANGS | (VOTES if n_best == 1 else 0) | (MINUS if strand else 0))
        if n_best == 1:
            voters[e].append(P.codes_of(rows[2 * r + 1 - strand], L - h, h)[:max_grow])
    out = dict(end=np.array(res["end"], np.int32).reshape(R), over=np.array(res["over"], np.int32).reshape(R), mm=np.array(res["mm"], np.uint8).reshape(R),
               hits=np.array(res["hits"], np.uint8).reshape(R), state=np.array(res["state"], np.uint8).reshape(R))
    count = np.zeros((2 * T, max_grow, 4), np.uint32)
    for e in range(2 * T):
        for b in range(4):
            for tail in voters[e]:
                count[e, :len(tail), b] += tail == b
    cover = count.sum(axis=2, dtype=np.int64)
    top = count.max(axis=2).astype(np.int64)
    ok_cover = cover >= p["min_cover"]
    ok = ok_cover & (100 * top >= p["min_percent"] * cover)
    x = np.array([int(np.argmin(np.append(ok[e], False))) for e in range(2 * T)], np.int64).reshape(2 * T)
    stop = np.array([2 if x[e] == max_grow else (0 if not ok_cover[e, x[e]] else 1) for e in range(2 * T)], np.uint8).reshape(2 * T)
    win = count.argmax(axis=2).astype(np.uint8)                            # the first of equal counts; a passing column has one winner
    left, right = x[0::2], x[1::2]
    tlen = np.array([len(s) for s in seqs], np.int64).reshape(T)
    new_len = tlen + left + right
    col_off = np.concatenate([[0], np.cumsum(new_len)])
    if int(col_off[-1]) > 2 ** 32 - 2:
        raise OverflowError("more than 2^32 - 2 new columns")
    flat = np.zeros(int(col_off[-1]), np.uint8)
    for t in range(T):
        o = int(col_off[t])
        for i in range(int(left[t])):
            flat[o + int(left[t]) - 1 - i] = 3 - win[2 * t, i]
        flat[o + int(left[t]):o + int(left[t]) + int(tlen[t])] = seqs[t]
        flat[o + int(left[t]) + int(tlen[t]):int(col_off[t + 1])] = win[2 * t + 1, :int(right[t])]
    n_voting = sum(len(v) for v in voters)
    n_hang = int((out["state"] & OVERHANGS > 0).sum())
    out.update(count=count.reshape(-1), e_stop=stop, e_voters=np.array([len(v) for v in voters], np.uint32).reshape(2 * T), left=left.astype(np.uint32),
               right=right.astype(np.uint32), len=new_len.astype(np.int32), col_off=col_off.astype(np.uint32), begin=col_off[:-1].astype(np.uint64),
               words=column_words([flat]))
    out["info"] = dict(candidates=n_cand, overhanging=n_hang, voting=n_voting, multi=n_hang - n_voting, hits_saturated=int(n_sat), seeds=n_seeds,
                       seeds_over_max_occ=int(n_over), index_positions=int(sum(occ.values())), ends_with_voters=sum(1 for v in voters if v), ends_grown=int((x > 0).sum()),
                       bases_added=int(x.sum()), longest_growth=int(x.max()) if len(x) else 0, stops_cover=int((stop == 0).sum()), stops_percent=int((stop == 1).sum()),
                       stops_max=int((stop == 2).sum()), columns_before=int(tlen.sum()), columns_after=int(new_len.sum()), n50_before=SC.n50(tlen), n50_after=SC.n50(new_len))
    return out


def sequences(res):
    """the grown targets as code arrays"""
    return [P.codes_of(res["words"], int(res["col_off"][t]), int(res["len"][t])) for t in range(len(res["len"]))]


def fasta(res):
    """the grown FASTA as bytes: one record per target with a length"""
    out = []
    for t, s in enumerate(sequences(res)):
        if len(s):
            out.append(">contig_id=%d_length=%d_left=%d_right=%d\n%s\n" % (t, len(s), res["left"][t], res["right"][t], "".join("ACGT"[x] for x in s)))
    return "".join(out).encode()


def grow_tsv(res):
    """one line per target: contig left right voters_left voters_right stop_left stop_right"""
    return "".join("%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (t, res["left"][t], res["right"][t], res["e_voters"][2 * t], res["e_voters"][2 * t + 1], res["e_stop"][2 * t],
                                                   res["e_stop"][2 * t + 1]) for t in range(len(res["len"]))).encode()
