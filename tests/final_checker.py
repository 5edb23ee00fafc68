"""The final contig set in plain Python / numpy: the DEFINITION the device code (alga_final_contigs_device, alga_contig_trim_device,
alga_write_final_fasta_device) has to equal array for array and byte for byte.  Written from the definition in include/alga_amd.h.

verdicts_sequential   OutputWriterNew::filterContigs restated: the pairs longest first (ties: the smaller pair number), a mark per read
                      index, the share of new reads in IEEE double.
verdicts_rounds       the same result by the schedule the device uses: marks for the end entries alone, a pair decided in the round in which each
                      of its end reads is marked by an accepted pair of smaller rank or has no undecided pair of smaller rank.
trim_left             src/main.cpp:636-697 through the oracle's creator on the sequences as they are, or (capped=True) in the cap form: the
                      first 501 and the last 501 nt of every sequence longer than 1002 nt.
final_contigs         the whole call; fasta_bytes: the text of the FASTA.

u / cons: a unitig or contig result and its consensus as dicts (tests/unitig_checker.py, contig_checker.py, consensus_checker.py, or the device's
via to_host())."""
import numpy as np

import oracle_lib as O

SHORT, REJECTED, ACCEPTED, TRIMMED_AWAY = 0, 1, 2, 3
CAP_HALF = 501


def _check_args(min_length, percent, trim_threshold=0):
    if min_length < 0:
        raise ValueError("min_length must not be negative")
    if not 0 <= percent <= 100:
        raise ValueError("new_reads_percent must be in [0, 100]")
    if trim_threshold != 0 and not 1 <= trim_threshold <= 501:
        raise ValueError("trim_threshold must be 0 or in [1, 501]")


def rank_order(cons_len):
    """pairs by (length descending, pair ascending)"""
    L = np.asarray(cons_len, dtype=np.int64)
    return sorted(range(len(L)), key=lambda k: (-int(L[k]), k))


def rejects(new, all_, percent):
    """OutputWriterNew::filterContig: double ratio = (double) new / all; 100 * ratio < percentage"""
    ratio = float(new) / float(all_)
    return 100.0 * ratio < float(percent)


def _reads_of(u, k):
    po = np.asarray(u["path_off"]).astype(np.int64)
    return [int(v) >> 1 for v in np.asarray(u["path_node"])[po[k]: po[k + 1]]]


def _numbered(P, by_rank, verdict, new_reads):
    rank = np.zeros(P, dtype=np.int32)
    ident = np.full(P, -1, dtype=np.int32)
    order = []
    for r, k in enumerate(by_rank):
        rank[k] = r
        if verdict[k] == ACCEPTED:
            ident[k] = len(order)
            order.append(k)
    return dict(verdict=np.asarray(verdict, dtype=np.uint8), rank=rank, id=ident, new_reads=np.asarray(new_reads, dtype=np.int32),
                order=np.asarray(order, dtype=np.int32))


def verdicts_sequential(u, cons_len, min_length, percent):
    _check_args(min_length, percent)
    P = int(u["n_pairs"])
    by_rank = rank_order(cons_len)
    marked = set()
    verdict, new_reads = [SHORT] * P, [-1] * P
    for k in by_rank:
        L = int(cons_len[k])
        if L < min_length or L == 0:
            continue
        reads = _reads_of(u, k)
        new = sum(1 for r in reads if r not in marked)
        new_reads[k] = new
        if rejects(new, len(reads), percent):
            verdict[k] = REJECTED
        else:
            verdict[k] = ACCEPTED
            marked.update(reads)
    return _numbered(P, by_rank, verdict, new_reads)


def verdicts_rounds(u, cons_len, min_length, percent):
    """-> (the result of verdicts_sequential, rounds)"""
    _check_args(min_length, percent)
    P = int(u["n_pairs"])
    by_rank = rank_order(cons_len)
    rank = {k: r for r, k in enumerate(by_rank)}
    INF = 1 << 62
    first_acc = {}
    verdict = [SHORT] * P
    ends, alls = {}, {}
    undecided = []
    for k in by_rank:
        L = int(cons_len[k])
        if L < min_length or L == 0:
            continue
        reads = _reads_of(u, k)
        alls[k] = len(reads)
        ends[k] = reads[:1] if len(reads) == 1 else [reads[0], reads[-1]]
        if not rejects(len(reads) - len(ends[k]), len(reads), percent):       # accepted whatever came before
            verdict[k] = ACCEPTED
            for r in ends[k]:
                first_acc[r] = min(first_acc.get(r, INF), rank[k])
        else:
            undecided.append(k)
    rounds = 0
    while undecided:
        rounds += 1
        min_und = {}
        for k in undecided:
            for r in ends[k]:
                min_und[r] = min(min_und.get(r, INF), rank[k])
        snapshot = dict(first_acc)                                             # (a round reads the marks of its start: the slowest schedule)
        again = []
        for k in undecided:
            rho = rank[k]
            if all(snapshot.get(r, INF) < rho or min_und[r] >= rho for r in ends[k]):
                new = alls[k] - sum(1 for r in ends[k] if snapshot.get(r, INF) < rho)
                if rejects(new, alls[k], percent):
                    verdict[k] = REJECTED
                else:
                    verdict[k] = ACCEPTED
                    for r in ends[k]:
                        first_acc[r] = min(first_acc.get(r, INF), rho)
            else:
                again.append(k)
        assert len(again) < len(undecided), "the undecided pair of the smallest rank is decidable"
        undecided = again
    new_reads = [-1] * P
    for k in alls:
        new_reads[k] = alls[k] - sum(1 for r in ends[k] if first_acc.get(r, INF) < rank[k])
    return _numbered(P, by_rank, verdict, new_reads), rounds


def codes_of(words, begin, length):
    """bases begin .. begin + length of a packed word array as codes (uint8)"""
    q = int(begin) + np.arange(int(length), dtype=np.int64)
    return ((np.asarray(words, dtype=np.uint32)[q >> 4] >> (2 * (q & 15)).astype(np.uint32)) & np.uint32(3)).astype(np.uint8)


def cap(seq):
    return seq if len(seq) <= 2 * CAP_HALF else np.concatenate([seq[:CAP_HALF], seq[-CAP_HALF:]])


def pack_rows(seqs):
    n = len(seqs)
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    W = max(1, (int(lens.max()) + 15) // 16) if n else 1
    codes = np.zeros((n, 16 * W), dtype=np.uint64)
    for i, s in enumerate(seqs):
        codes[i, : len(s)] = s
    words = (codes.reshape(n, W, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=2).astype(np.uint32)
    return words, lens


def trim_left(seqs, threshold=25, capped=False):
    """seqs: list of code arrays.  Nodes 0 .. n-1 the sequences, n .. 2n-1 their reverse complements, one build at min_overlap = rsoe_min_overlap =
    threshold; trim_left[d] = the largest len[i] - offset over the edges i -> d with i, d < n.  -> (int32 [n], edges of the build)"""
    n = len(seqs)
    if n == 0:
        return np.zeros(0, dtype=np.int32), 0
    seqs = [np.asarray(s, dtype=np.uint8) for s in seqs]
    if capped:
        seqs = [cap(s) for s in seqs]
    words, lens = pack_rows(seqs + [(3 - s)[::-1] for s in seqs])
    e, _, _ = O.prefsuf(words, lens, threshold, threshold)
    trim = np.zeros(n, dtype=np.int32)
    for a, d, off in e.tolist():
        if a < n and d < n:
            trim[d] = max(int(trim[d]), int(lens[a]) - off)
    return trim, len(e)


def final_contigs(u, cons, min_length, percent, trim_threshold, capped=False):
    """The definition of alga_final_contigs_device -> dict in the dtypes of FinalContigs.to_host()"""
    _check_args(min_length, percent, trim_threshold)
    P = int(u["n_pairs"])
    clen = np.asarray(cons["len"], dtype=np.int32)
    ctrim = np.asarray(cons["trim_left"], dtype=np.int32)
    wo = np.asarray(u["word_off"]).astype(np.int64)
    r = verdicts_sequential(u, clen, min_length, percent)
    verdict = r["verdict"].copy()
    acc = verdict == ACCEPTED
    begin = np.where(acc, ctrim, 0).astype(np.int32)
    length = np.where(acc, clen, 0).astype(np.int32)
    tl = np.zeros(P, dtype=np.int32)
    edges = 0
    if trim_threshold > 0 and len(r["order"]):
        seqs = [codes_of(cons["words"], 16 * wo[k] + ctrim[k], clen[k]) for k in r["order"].tolist()]
        t, edges = trim_left(seqs, trim_threshold, capped)
        for j, k in enumerate(r["order"].tolist()):
            tl[k] = t[j]
            if t[j] + 10 < clen[k]:                                            # src/main.cpp:705 with trimRight = 0
                begin[k] += t[j]
                length[k] -= t[j]
            else:
                verdict[k], begin[k], length[k] = TRIMMED_AWAY, 0, 0
    count = lambda v: int((verdict == v).sum())
    return dict(n_pairs=P, verdict=verdict, rank=r["rank"], id=r["id"], new_reads=r["new_reads"], trim_left=tl, begin=begin, len=length, order=r["order"],
                n_accepted=len(r["order"]), n_written=count(ACCEPTED),
                info=dict(pairs=P, n_short=count(SHORT), rejected=count(REJECTED), accepted=count(ACCEPTED), trimmed_away=count(TRIMMED_AWAY), trim_edges=edges))


def window(u, cons, fin, k):
    """ACGT string of pair k's written window"""
    wo = np.asarray(u["word_off"]).astype(np.int64)
    return "".join("ACGT"[c] for c in codes_of(cons["words"], 16 * wo[k] + int(fin["begin"][k]), fin["len"][k]))


def fasta_bytes(u, cons, fin):
    """The text of alga_write_final_fasta_device and its record count"""
    out = []
    for j, k in enumerate(np.asarray(fin["order"]).tolist()):
        if fin["verdict"][k] == ACCEPTED:
            out.append(">contig_id=%d_length=%d\n%s\n" % (j, int(fin["len"][k]), window(u, cons, fin, k)))
    return "".join(out).encode(), len(out)
