"""Hand-built contig graphs for the extension by paired connections (tests/test_extend_cpu.py, tests/test_gpu_extend.py): nodes of one
length, chains given by their offsets, mates handed out in adjacent read indices as the ingest interleaves them.  The sequences are
arbitrary rows: only the dovetail check looks at the lengths.

A case is a function -> dict(words, lens, edges, pair_off, mcw, mconn, max_insert, expect) where expect pins what the case is about
(pairs_out, joinable, ...) so that a change of the builder cannot turn an edge case into an easy one unnoticed."""
import numpy as np

LEN = 100
STEP = 10                                                                  # default offset between neighbours of a chain


class Build:
    def __init__(self, seed=1):
        self.edges, self.n_reads, self.po, self.seed = [], 0, {}, seed

    def reads(self, k):
        """k unpaired reads -> their forward nodes"""
        out = [2 * (self.n_reads + i) + 1 for i in range(k)]
        self.n_reads += k
        return out

    def mates(self, k, swap=False):
        """k pairs -> (A, B): forward nodes, A[i] and B[i] are mates (pair_off 1 and 2; swap: 2 and 1)"""
        A, B = [], []
        for _ in range(k):
            r = self.n_reads
            self.n_reads += 2
            for v in (2 * r, 2 * r + 1):
                self.po[v] = 1
            for v in (2 * r + 2, 2 * r + 3):
                self.po[v] = 2
            A.append(2 * r + 1); B.append(2 * r + 3)
        return (B, A) if swap else (A, B)

    def chain(self, nodes, offsets=STEP):
        offs = [offsets] * (len(nodes) - 1) if isinstance(offsets, int) else list(offsets)
        assert len(offs) == len(nodes) - 1
        for a, b, o in zip(nodes, nodes[1:], offs):
            self.edges.append((a, b, o))
        return nodes

    def done(self, mcw=0, mconn=5, max_insert=1000, **expect):
        n = 2 * self.n_reads
        lens = np.full(n, LEN, dtype=np.int32)
        words = np.random.RandomState(self.seed).randint(0, 1 << 32, size=(n, (LEN + 15) // 16), dtype=np.uint64).astype(np.uint32)
        words[:, -1] &= np.uint32((1 << (2 * (LEN & 15))) - 1) if LEN & 15 else np.uint32(0xFFFFFFFF)
        po = np.zeros(n, dtype=np.uint8)
        for v, x in self.po.items():
            po[v] = x
        return dict(words=words, lens=lens, edges=np.array(self.edges, dtype=np.int32).reshape(-1, 3), pair_off=po, mcw=mcw, mconn=mconn,
                    max_insert=max_insert, expect=expect)


def junction(b, n_pairs=5, x_body=3, y_body=3, tail_offsets=STEP, head_offsets=STEP, twin_mates=0, swap=False):
    """X = x.. A.. a,  Y = a B.. y..,  Z = z z a (a second predecessor: `a` is a junction and Y the only contig that starts there).
    A[i] / B[i] are mates; the first twin_mates of the B stand in Y as their reverse nodes.  tail_offsets: the offsets of the edges into the
    A and into a; head_offsets: of the edges into the B and out of the last one."""
    A, B = b.mates(n_pairs, swap=swap)
    a = b.reads(1)[0]
    xs, ys = b.reads(x_body), b.reads(y_body)
    head = [v ^ 1 if i < twin_mates else v for i, v in enumerate(B)]
    X = xs + A + [a]
    Y = [a] + head + ys
    nx, ny = len(X) - 1, len(Y) - 1
    b.chain(X, ([STEP] * max(nx - n_pairs - 1, 0) + [tail_offsets] * (n_pairs + 1))[-nx:])
    b.chain(Y, ([head_offsets] * (n_pairs + 1) + [STEP] * max(ny - n_pairs - 1, 0))[:ny])
    Z = b.chain(b.reads(2) + [a])
    return dict(X=X, Y=Y, Z=Z, A=A, B=B, a=a)


def case_join():
    b = Build()
    junction(b)
    return b.done(pairs_out=2, joinable=2, direct_links=1, links=2, ambiguous=0)


def case_no_pairs():
    b = Build()
    junction(b)
    b.po.clear()
    return b.done(pairs_out=3, joinable=0, direct_links=0)


def case_cnt_4():
    b = Build()
    junction(b, n_pairs=4)
    return b.done(pairs_out=3, joinable=0, direct_links=0)


def case_cnt_5_of_6_needed():
    b = Build()
    junction(b, n_pairs=5)
    return b.done(mconn=6, pairs_out=3, joinable=0)


def case_weight_at():
    """w(X) = w(Y) = 8 * STEP: X = 3 + 5 + 1 nodes, Y = 1 + 5 + 3"""
    b = Build()
    junction(b)
    return b.done(mcw=8 * STEP, pairs_out=2, joinable=2)


def case_weight_x_below():
    b = Build()
    junction(b, x_body=2)                                                  # w(X) = 7 * STEP, w(Y) = 8 * STEP
    return b.done(mcw=8 * STEP, pairs_out=3, joinable=0)


def case_weight_y_below():
    b = Build()
    junction(b, y_body=2)
    return b.done(mcw=8 * STEP, pairs_out=3, joinable=0)


def case_head_window_in():
    """Y = a B1 .. B5 y..: entry i is in the head when p_(i-1) <= max_insert; B5 is entry 5, p_4 = 4 * STEP.  The tail is made narrow by
    small offsets so that only the head decides."""
    b = Build()
    junction(b, tail_offsets=1)
    return b.done(max_insert=4 * STEP, pairs_out=2, joinable=2)


def case_head_window_out():
    b = Build()
    junction(b, tail_offsets=1)
    return b.done(max_insert=4 * STEP - 1, pairs_out=3, joinable=0)


def case_tail_window_in():
    """X = x x x A1 .. A5 a: w - p_i of A1 is 5 * STEP; the head is made wide by small offsets so that only the tail decides"""
    b = Build()
    junction(b, head_offsets=1)
    return b.done(max_insert=5 * STEP, pairs_out=2, joinable=2)


def case_tail_window_out():
    b = Build()
    junction(b, head_offsets=1)
    return b.done(max_insert=5 * STEP - 1, pairs_out=3, joinable=0)


def case_entry0_of_x_not_counted():
    """X = A1 .. A5 a without a body: A1 is entry 0, inside the window and still not counted -> 4"""
    b = Build()
    junction(b, x_body=0)
    return b.done(pairs_out=3, joinable=0, direct_links=0)


def case_a_not_in_head():
    """the junction read itself is paired with a tail read: entry 0 of Y is not in the head -> 4 + 0"""
    b = Build()
    A, B = b.mates(5)
    xs, ys = b.reads(3), b.reads(3)
    a = B[4]
    b.chain(xs + A + [a])
    b.chain([a] + B[:4] + ys)
    b.chain(b.reads(2) + [a])
    return b.done(pairs_out=3, joinable=0, direct_links=0)


def case_y_two_entries():
    """Y = a B1: the head is one read; five tail reads cannot all be its mates, so min_connections = 1 decides"""
    b = Build()
    A, B = b.mates(1)
    a = b.reads(1)[0]
    b.chain(b.reads(3) + A + [a])
    b.chain([a] + B)
    b.chain(b.reads(2) + [a])
    return b.done(mconn=1, pairs_out=2, joinable=2)


def case_pair_off_swapped():
    b = Build()
    junction(b, swap=True)
    return b.done(pairs_out=2, joinable=2)


def case_mate_as_twin():
    """two of the five mates stand in Y as the reverse node of the mate read (the head is compared on read indices)"""
    b = Build()
    junction(b, twin_mates=2)
    return b.done(pairs_out=2, joinable=2)


def case_unpaired_own_index_in_head():
    """four pairs, and the unpaired junction read a: it is the last entry of X (in the tail) and the last entry of the closed chain C = a .. a
    (in C's head).  The reference would compare it with itself and reach 5; here it does not count, X -> C is no link and nothing is joined."""
    b = Build()
    A, B = b.mates(4)
    a = b.reads(1)[0]
    b.chain(b.reads(3) + A + [a])
    b.chain([a] + B + b.reads(2) + [a])
    return b.done(pairs_out=2, joinable=0, direct_links=0)


SLICE = 1024                                                               # head entries a pass of the device's count takes (ALGA_EXTEND_HEAD_SLICE)


def case_sizes(k_head, k_tail, offset=1, mates_last=False):
    """A head of EXACTLY k_head entries and a tail of EXACTLY k_tail entries (the junction read a, always in T, is one of them), pinned by
    expect["head_max"] and by "sizes" / "X" / "Y" (tests/test_extend_cpu.py counts the tail with the checker's tail_entries).
    n = min(k_head, k_tail) pairs, min_connections = n: every one has to be found.  a itself is the first read of the last pair, the other
    first reads end the tail; the mates begin the head (mates_last: they end it, so that they fall into the last slice of a long head).
    offset 1: max_insert = max(k) - 1.  The side with the most entries is cut by the WINDOW: two more reads follow the head (the first has
    p_(i-1) = k_head > max_insert) or lead the tail (w - p_i = k_tail - 1 + STEP).  The side with fewer entries is cut by the contig's END:
    Y = a + head, X = one read + tail -- entry 0 of X is not in T.
    offset 0: a run of offset 0 behind one edge of 7 (no chain weighs 0); both sides are cut by the contig's end.
    Z = one read + a weighs 1, below min_chain_weight = 2, so that X is the only predecessor that qualifies."""
    def make():
        b = Build()
        n_pairs = min(k_head, k_tail)
        A, B = b.mates(n_pairs)
        a = A[-1]
        tail = b.reads(k_tail - n_pairs) + A[:-1]
        fill = b.reads(k_head - n_pairs)
        head = fill + B if mates_last else B + fill
        assert len(head) == k_head and len(tail) + 1 == k_tail
        by_window = offset > 0
        big = max(k_head, k_tail)
        lead = b.reads(2) if by_window and k_tail == big else b.reads(1)
        trail = b.reads(2) if by_window and k_head == big else []
        X = lead + tail + [a]
        Y = [a] + head + trail
        if by_window:
            b.chain(X, [STEP] * len(lead) + [offset] * (len(X) - 1 - len(lead)))
            b.chain(Y, [offset] * k_head + [STEP] * len(trail))
            max_insert = big * offset - 1
        else:
            b.chain(X, [7] + [0] * (len(X) - 2))
            b.chain(Y, [7] + [0] * (len(Y) - 2))
            max_insert = 50
        b.chain(b.reads(1) + [a], [1])                                     # Z, too light to qualify: a's own pair would count for it too
        d = b.done(mcw=2, mconn=n_pairs, max_insert=max_insert, pairs_out=2, joinable=2, direct_links=1, head_max=k_head)
        d.update(sizes=(k_head, k_tail), X=X, Y=Y)
        return d
    return make


def case_ambiguous():
    """two predecessors qualify: none is joined"""
    b = Build()
    A1, B1 = b.mates(5)
    A2, B2 = b.mates(5)
    a = b.reads(1)[0]
    b.chain(b.reads(3) + A1 + [a])
    b.chain(b.reads(3) + A2 + [a])
    b.chain([a] + B1 + B2 + b.reads(3))
    return b.done(pairs_out=3, joinable=0, direct_links=2, links=4, ambiguous=1)


def case_one_of_two():
    """one qualifying predecessor of two: a join; Z ends at a read that is now interior"""
    b = Build()
    junction(b)
    return b.done(pairs_out=2, joinable=2)


def case_three_chains(shift=0):
    """X -> Y -> W through two junctions; w(X) = 8 * STEP + shift moves the second and third chain to every base & 15"""
    def make():
        b = Build()
        A1, B1 = b.mates(5)
        A2, B2 = b.mates(5)
        a, c = b.reads(2)
        X = b.reads(3) + A1 + [a]
        Y = [a] + B1 + b.reads(2) + A2 + [c]
        W = [c] + B2 + b.reads(3)
        b.chain(X, [STEP + shift] + [STEP] * (len(X) - 2))
        b.chain(Y, [STEP + (shift * 7) % 16] + [STEP] * (len(Y) - 2))
        b.chain(W)
        b.chain(b.reads(2) + [a])
        b.chain(b.reads(2) + [c])
        return b.done(pairs_out=3, joinable=4, longest_nodes=len(X) + len(Y) + len(W) - 2)
    return make


def case_cycle():
    """X: a .. c and Y: c .. a with pairs across both junctions: a cycle of joinable links (and its twin), opened at the smallest id"""
    b = Build()
    A1, B1 = b.mates(5)
    A2, B2 = b.mates(5)
    a, c = b.reads(2)
    b.chain([a] + B2 + b.reads(2) + A1 + [c])
    b.chain([c] + B1 + b.reads(2) + A2 + [a])
    b.chain(b.reads(2) + [a])
    b.chain(b.reads(2) + [c])
    return b.done(cycles_cut=1, joinable=2, pairs_out=3)


def case_closed_chain():
    """C: a .. a, its tail paired with its own head, and Z into a: C -> C is a link but never joinable"""
    b = Build()
    A, B = b.mates(5)
    a = b.reads(1)[0]
    b.chain([a] + B + b.reads(3) + A + [a])
    b.chain(b.reads(2) + [a])
    return b.done(joinable=0, pairs_out=2)


CASES = {
    "join": case_join, "no_pairs": case_no_pairs, "cnt_4": case_cnt_4, "cnt_5_of_6_needed": case_cnt_5_of_6_needed, "weight_at": case_weight_at,
    "weight_x_below": case_weight_x_below, "weight_y_below": case_weight_y_below, "head_window_in": case_head_window_in,
    "head_window_out": case_head_window_out, "tail_window_in": case_tail_window_in, "tail_window_out": case_tail_window_out,
    "entry0_of_x_not_counted": case_entry0_of_x_not_counted, "a_not_in_head": case_a_not_in_head, "y_two_entries": case_y_two_entries,
    "pair_off_swapped": case_pair_off_swapped, "mate_as_twin": case_mate_as_twin, "unpaired_own_index_in_head": case_unpaired_own_index_in_head,
    "ambiguous": case_ambiguous, "one_of_two": case_one_of_two, "cycle": case_cycle, "closed_chain": case_closed_chain,
}
for _k in (1, 63, 64, 65, 1100):
    CASES["head_%d" % _k] = case_sizes(_k, 5 if _k >= 5 else 1)
    CASES["tail_%d" % _k] = case_sizes(5 if _k >= 5 else 1, _k)
CASES["head_tail_1100"] = case_sizes(1100, 1100)
CASES["offset_0_run"] = case_sizes(70, 70, offset=0)
# the slice boundary of a long head: the five mates are its last entries -- the last of slice 1; four in slice 1 and one in slice 2; all in slice 2
CASES["head_%d_mates_last" % SLICE] = case_sizes(SLICE, 5, mates_last=True)
CASES["head_%d_mates_last" % (SLICE + 1)] = case_sizes(SLICE + 1, 5, mates_last=True)
CASES["head_1100_mates_last"] = case_sizes(1100, 5, mates_last=True)
SIZE_CASES = sorted(k for k in CASES if k.startswith(("head_", "tail_", "offset_0")) and "window" not in k)
for _s in range(16):
    CASES["three_chains_%02d" % _s] = case_three_chains(_s)


def random_case(seed, max_nodes=2000):
    """a random contig graph: chains between random junction reads; the first reads of a pair go to the tails of random chains, their mates
    mostly to the heads of chains that start where that chain ends, some as reverse nodes; thresholds low enough that links of every kind occur"""
    rng = np.random.RandomState(1000 + seed)
    b = Build(seed=seed)
    n_junc = int(rng.randint(2, 9))
    junc = b.reads(n_junc)
    ends, seen = [], set()
    for _ in range(int(rng.randint(n_junc, 3 * n_junc + 1))):
        s_, t_ = junc[int(rng.randint(n_junc))], junc[int(rng.randint(n_junc))]
        if rng.rand() < 0.15:
            t_ ^= 1
        if (s_, t_) in seen or (t_ ^ 1, s_ ^ 1) in seen:
            continue
        seen.add((s_, t_))
        ends.append((s_, t_))
    heads, tails = [[] for _ in ends], [[] for _ in ends]
    for A, B in zip(*b.mates(int(rng.randint(20, 150)), swap=bool(seed & 1))):
        x = int(rng.randint(len(ends)))
        after = [y for y, (s_, _) in enumerate(ends) if s_ == ends[x][1]]
        y = after[int(rng.randint(len(after)))] if after and rng.rand() < 0.8 else int(rng.randint(len(ends)))
        tails[x].append(A)
        heads[y].append(B ^ 1 if rng.rand() < 0.2 else B)
    for (s_, t_), h, t in zip(ends, heads, tails):
        inner = h + b.reads(int(rng.randint(1, 12))) + t
        offs = rng.randint(0 if rng.rand() < 0.3 else 1, 40, size=len(inner) + 1).tolist()
        if sum(offs) == 0:
            offs[0] = 7
        b.chain([s_] + inner + [t_], offs)
    assert 2 * b.n_reads <= max_nodes
    return b.done(mcw=int(rng.randint(0, 60)), mconn=int(rng.randint(1, 4)), max_insert=int(rng.choice([30, 100, 1000])))
