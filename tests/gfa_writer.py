"""The GFA 1.0 export of the overlap graph, stated in Python (the checker of alga_write_gfa_device, include/alga_amd.h).

Output: the header line, the segments in ascending name order, the links in edge-list order; fields separated by one tab,
every line ends with a newline.

Twin layout (twins=True, ALGA's: node 2k+1 = read k, node 2k = its reverse complement):
  segment k  = twin pair k, written when len[2k+1] > 0:   S <k> <ACGT of node 2k+1 | *> LN:i:<len>
  node 2k+1 is orientation +, node 2k is -.
  The twin of edge (a -> b, o) is (b^1 -> a^1, len[b] - len[a] + o): the same GFA link.  An edge is emitted unless its exact
  twin is in the list too and the twin's (src, dst) is lexicographically smaller; a self-twin (b == a^1) is emitted once,
  an edge whose twin is missing on its own.
Plain layout: node i with len[i] > 0 is segment i, every orientation +, every edge is one link.
Link of edge (a -> b, o):  L <name a> <oa> <name b> <ob> <len[a] - o>M
"""
import numpy as np

HEADER = b"H\tVN:Z:1.0\n"


def decode_rows(words, lens):
    """2-bit rows (A C G T = 0..3, 16 codes per uint32, low bits first) -> list of bytes strings of their lengths"""
    words = np.ascontiguousarray(words, dtype=np.uint32).reshape(len(lens), -1)
    shifts = (2 * np.arange(16, dtype=np.uint32))
    codes = ((words[:, :, None] >> shifts) & 3).reshape(len(lens), -1).astype(np.uint8)
    ascii_ = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    return [ascii_[i, : int(lens[i])].tobytes() for i in range(len(lens))]


def check(lens, edges, twins):
    """the input checks of the device call; raises ValueError where it answers ALGA_ERR_INVALID_ARGUMENT"""
    lens = np.asarray(lens, dtype=np.int64)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 3)
    n = len(lens)
    if (lens < 0).any():
        raise ValueError("negative length")
    if twins and (n % 2 or (lens[0::2] != lens[1::2]).any()):
        raise ValueError("not a twin layout")
    if len(e) and ((e[:, :2] < 0).any() or (e[:, :2] >= n).any()):
        raise ValueError("node id out of range")
    if len(e) > 1:
        a, b = e[:-1], e[1:]
        gt = (a[:, 0] > b[:, 0]) | ((a[:, 0] == b[:, 0]) & ((a[:, 1] > b[:, 1]) | ((a[:, 1] == b[:, 1]) & (a[:, 2] > b[:, 2]))))
        if gt.any():
            raise ValueError("edges not sorted by (src, dst, offset)")


def gfa_bytes(words, lens, edges, twins=True, sequences=True):
    """-> (the GFA text as bytes, dict(segments, links, links_merged, bytes))"""
    check(lens, edges, twins)
    lens = np.asarray(lens, dtype=np.int64)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 3)
    n = len(lens)
    seg_nodes = np.arange(1, n, 2) if twins else np.arange(n)
    out = [HEADER]
    live = [int(x) for x in seg_nodes if lens[x] > 0]
    seqs = decode_rows(np.asarray(words).reshape(n, -1)[live], lens[live]) if sequences and live else None
    for j, node in enumerate(live):
        name = node >> 1 if twins else node
        out.append(b"S\t%d\t%s\tLN:i:%d\n" % (name, seqs[j] if sequences else b"*", lens[node]))
    segments = len(live)
    have = set(map(tuple, e.tolist())) if twins else set()
    links = merged = 0
    for a, b, o in e.tolist():
        if twins:
            t = (b ^ 1, a ^ 1, int(lens[b] - lens[a]) + o)
            if t in have and (t[0], t[1]) < (a, b):
                merged += 1
                continue
            out.append(b"L\t%d\t%s\t%d\t%s\t%dM\n" % (a >> 1, b"+" if a & 1 else b"-", b >> 1, b"+" if b & 1 else b"-", int(lens[a]) - o))
        else:
            out.append(b"L\t%d\t+\t%d\t+\t%dM\n" % (a, b, int(lens[a]) - o))
        links += 1
    text = b"".join(out)
    return text, dict(segments=segments, links=links, links_merged=merged, bytes=len(text))


def expand_links(text, lens, twins=True):
    """GFA text -> set of edge triples: every link as both of its edges (twin layout) or its one edge (plain)"""
    lens = np.asarray(lens, dtype=np.int64)
    got = set()
    for line in text.split(b"\n"):
        if not line.startswith(b"L\t"):
            continue
        _, na, oa, nb, ob, ov = line.split(b"\t")
        assert ov.endswith(b"M")
        if twins:
            a = 2 * int(na) + (1 if oa == b"+" else 0)
            b = 2 * int(nb) + (1 if ob == b"+" else 0)
        else:
            assert oa == b"+" and ob == b"+"
            a, b = int(na), int(nb)
        o = int(lens[a]) - int(ov[:-1])
        got.add((a, b, o))
        if twins:
            got.add((b ^ 1, a ^ 1, int(lens[b] - lens[a]) + o))
    return got
