"""The definition of the pair calls over both placement passes and of the SAM text (include/alga_amd.h: alga_judge_pairs_device,
alga_write_sam_device) in plain Python.  It works from the outputs of place_checker.place and gapped_checker.gapped_banded (dicts of arrays) and
shares nothing with the device's method: every read's view is a small dict, the text is put together line by line with %-formatting."""
import numpy as np

import gapped_checker as GC
import place_checker as P

NAMES_DEPTH, SKIP_UNPLACED = 1, 2
ARRAYS = ("flag", "tlen", "insert_hist")
COUNTERS = ("reads", "live", "placed_h", "placed_g", "unplaced", "pairs", "pairs_proper", "pairs_improper", "pairs_split", "pairs_not_unique", "pairs_with_gapped",
            "proper_with_gapped", "insert_median", "insert_mean_x100")
PAIR_COUNTERS = ("pairs", "pairs_proper", "pairs_improper", "pairs_split", "pairs_not_unique", "insert_median", "insert_mean_x100")   # shared with place_checker


def check(lens, pair_off, pl, gp, max_insert, flags=0):
    if not 1 <= max_insert <= 1 << 20 or flags:
        raise ValueError("parameter out of range")
    n = len(lens)
    if n % 2 or n // 2 != len(pl["state"]) or (gp is not None and len(gp["state"]) != n // 2):
        raise ValueError("not the placement's reads")
    if pair_off is not None:
        po = np.asarray(pair_off)
        for v in range(n):
            if po[v] > 2 or po[v] != po[v ^ 1] or (po[v] == 1 and (v + 2 >= n or po[v + 2] != 2)) or (po[v] == 2 and (v < 2 or po[v - 2] != 1)):
                raise ValueError("pair_off")


def view(lens, pl, gp, r):
    """rule 1: the combined view of read r"""
    L = int(lens[2 * r + 1])
    v = dict(L=L, live=L >= 1, kind=None, target=-1, pos=-1, end=-1, minus=False, unique=False, nm=0, runs=[])
    if not v["live"]:
        return v
    hs = int(pl["state"][r])
    if hs & P.PLACED:
        p = int(pl["pos"][r])
        v.update(kind="H", target=int(pl["target"][r]), pos=p, end=p + L, minus=bool(hs & P.MINUS), unique=bool(hs & P.UNIQUE), nm=int(pl["mm"][r]), runs=[(L, "M")])
    elif gp is not None and int(gp["state"][r]) & GC.PLACED:
        gs = int(gp["state"][r])
        runs = [(int(x) >> 2, "MID"[int(x) & 3]) for x in gp["cigar"][int(gp["cigar_off"][r]):int(gp["cigar_off"][r + 1])]]
        v.update(kind="G", target=int(gp["target"][r]), pos=int(gp["pos"][r]), end=int(gp["end"][r]), minus=bool(gs & GC.MINUS), unique=bool(gs & GC.UNIQUE),
                 nm=int(gp["edits"][r]), runs=runs)
    return v


def mate_of(lens, pair_off, pl, gp, r):
    """the mate of read r in a live pair, or None"""
    if pair_off is None or pair_off[2 * r + 1] not in (1, 2):
        return None
    m = r + 1 if pair_off[2 * r + 1] == 1 else r - 1
    return m if lens[2 * r + 1] >= 1 and lens[2 * m + 1] >= 1 else None


def verdict(a, b, max_insert):
    """rule 2 for the views of two mates -> ('not_unique' | 'split' | 'improper' | 'proper', insert)"""
    if not (a["unique"] and b["unique"]):
        return "not_unique", None
    if a["target"] != b["target"]:
        return "split", None
    if a["minus"] == b["minus"]:
        return "improper", None
    p, m = (b, a) if a["minus"] else (a, b)
    ins = m["end"] - p["pos"]
    if p["pos"] <= m["pos"] and p["end"] <= m["end"] and ins <= max_insert:
        return "proper", ins
    return "improper", None


def pair_calls(lens, pair_off, pl, gp=None, max_insert=1000, flags=0):
    check(lens, pair_off, pl, gp, max_insert, flags)
    R = len(lens) // 2
    out = dict(flag=np.zeros(R, np.uint16), tlen=np.zeros(R, np.int32), insert_hist=np.zeros(max_insert + 1, np.uint64))
    info = dict.fromkeys(COUNTERS, 0)
    info["reads"] = R
    total = 0
    for r in range(R):
        me = view(lens, pl, gp, r)
        if not me["live"]:
            continue
        info["live"] += 1
        info["placed_h" if me["kind"] == "H" else "placed_g" if me["kind"] == "G" else "unplaced"] += 1
        fl = 0
        if me["kind"] is None:
            fl |= 0x4
        elif me["minus"]:
            fl |= 0x10
        m = mate_of(lens, pair_off, pl, gp, r)
        if m is not None:
            mt = view(lens, pl, gp, m)
            fl |= 0x1 | (0x40 if r < m else 0x80)
            if mt["kind"] is None:
                fl |= 0x8
            elif mt["minus"]:
                fl |= 0x20
            what, ins = verdict(me, mt, max_insert)
            if what == "proper":
                fl |= 0x2
            if me["kind"] and mt["kind"] and me["target"] == mt["target"]:
                span = max(me["end"], mt["end"]) - min(me["pos"], mt["pos"])
                out["tlen"][r] = span if (me["pos"], r) < (mt["pos"], m) else -span
            if r < m:
                g = me["kind"] == "G" or mt["kind"] == "G"
                info["pairs"] += 1
                info["pairs_" + what] += 1
                info["pairs_with_gapped"] += g
                if what == "proper":
                    info["proper_with_gapped"] += g
                    out["insert_hist"][ins] += 1
                    total += ins
        out["flag"][r] = fl
    info["insert_median"] = info["insert_mean_x100"] = -1
    if info["pairs_proper"]:
        cum = np.cumsum(out["insert_hist"].astype(np.int64))
        info["insert_median"] = int(np.nonzero(cum >= (info["pairs_proper"] + 1) // 2)[0][0])
        info["insert_mean_x100"] = 100 * total // info["pairs_proper"]
    out["info"] = {k: int(v) for k, v in info.items()}
    return out


def target_lengths(pl):
    co = pl["col_off"].astype(np.int64)
    return [int(co[t + 1] - co[t]) for t in range(len(co) - 1)]


def name(pl, t, depth):
    """name(t): the first token of the final FASTA's header, in the depth form that of the depth FASTA's"""
    length = target_lengths(pl)[t]
    return P.depth_header(t, length, pl["t_reads"][t], pl["t_bases"][t])[1:] if depth else "contig_id=%d_length=%d" % (t, length)


def header(pl, depth=False):
    lines = ["@HD\tVN:1.6\tSO:unsorted\tGO:query"]
    lines += ["@SQ\tSN:%s\tLN:%d" % (name(pl, t, depth), n) for t, n in enumerate(target_lengths(pl)) if n >= 1]
    lines += ["@PG\tID:alga_amd\tPN:alga_amd"]
    return "".join(x + "\n" for x in lines)


def sam_cigar(v):
    """the runs as SAM text, an I run at either end as S -> (text, the clipped bases)"""
    if v["kind"] is None:
        return "*", 0
    out, clip = [], 0
    for i, (n, op) in enumerate(v["runs"]):
        if op == "I" and i in (0, len(v["runs"]) - 1):
            op = "S"
            clip += n
        out.append("%d%s" % (n, op))
    return "".join(out), clip


def sam(rows, lens, pair_off, pl, gp, calls, flags=0):
    """the whole text as bytes; calls = pair_calls(...) of the same pl and gp"""
    depth = bool(flags & NAMES_DEPTH)
    R = len(lens) // 2
    stride = rows.shape[1] if R else 0
    out = [header(pl, depth)]

    def where(v, mate):                                                  # the RNAME / POS fields of a record: its own, else its placed live mate's
        for x in (v, mate):
            if x is not None and x["kind"]:
                return name(pl, x["target"], depth), x["pos"] + 1
        return "*", 0
    for r in range(R):
        me = view(lens, pl, gp, r)
        if not me["live"] or (flags & SKIP_UNPLACED and me["kind"] is None):
            continue
        if me["L"] > 16 * stride:
            raise ValueError("a live read is longer than its row")
        m = mate_of(lens, pair_off, pl, gp, r)
        mt = view(lens, pl, gp, m) if m is not None else None
        if me["kind"] == "G" and (not me["runs"] or sum(n for n, op in me["runs"] if op != "D") != me["L"]):
            raise ValueError("script")
        rname, pos = where(me, mt)
        rnext, pnext = where(mt, me) if mt is not None else ("*", 0)
        if rnext != "*" and rnext == rname:
            rnext = "="
        cigar, clip = sam_cigar(me)
        seq = "".join("ACGT"[b] for b in P.codes_of(rows[2 * r if me["kind"] and me["minus"] else 2 * r + 1], 0, me["L"]))
        f = ["r%d" % (min(r, m) if m is not None else r), "%d" % int(calls["flag"][r]), rname, "%d" % pos, "60" if me["kind"] and me["unique"] else "0", cigar, rnext, "%d" % pnext,
             "%d" % int(calls["tlen"][r]), seq, "*"]
        if me["kind"]:
            f += ["NM:i:%d" % (me["nm"] - clip), "XP:A:%s" % me["kind"]]
        out.append("\t".join(f) + "\n")
    return "".join(out).encode()
