"""An independent reading of a SAM text as alga_write_sam_device writes it: what must hold of any such file, whatever wrote it.  It shares no code
with tests/sam_checker.py and knows nothing of placements: only the text, the input reads and the target bases.

check(text, reads, targets, complete=True) -> dict of what it saw.  reads: the input reads as code arrays (None = removed), in read order;
targets: the target sequences as code arrays, target t named contig_id=<t>_...; complete: every live read has a record (no skipped ones)."""
import re

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _cigar(text):
    ops = re.findall(r"(\d+)([MIDS])", text)
    assert "".join(n + o for n, o in ops) == text and ops, ("CIGAR", text)
    ops = [(int(n), o) for n, o in ops]
    assert all(n >= 1 for n, _ in ops)
    assert all(o != "S" or i in (0, len(ops) - 1) for i, (_, o) in enumerate(ops)), ("a clip inside", text)
    return ops


def _letters(codes):
    return "".join("ACGT"[int(b)] for b in codes)


def check(text, reads, targets, complete=True):
    lines = text.decode().split("\n")
    assert lines[-1] == "" and lines[0] == "@HD\tVN:1.6\tSO:unsorted\tGO:query"
    lines.pop()
    ln, recs = {}, []
    n_head = 0
    for s in lines:
        if s.startswith("@"):
            assert not recs, "a header line behind a record"
            n_head += 1
            if s.startswith("@SQ"):
                tag, sn, l = s.split("\t")
                assert sn.startswith("SN:") and l.startswith("LN:") and sn[3:] not in ln and int(l[3:]) >= 1
                ln[sn[3:]] = int(l[3:])
        else:
            recs.append(s.split("\t"))
    assert lines[n_head - 1] == "@PG\tID:alga_amd\tPN:alga_amd"
    tid = {}
    for nm in ln:
        m = re.match(r"contig_id=(\d+)_length=(\d+)(_reads=\d+_depth=\d+\.\d\d)?$", nm)
        assert m and int(m.group(2)) == ln[nm] == len(targets[int(m.group(1))]), nm
        tid[nm] = int(m.group(1))
    assert sorted(tid.values()) == [t for t in range(len(targets)) if len(targets[t])], "one @SQ per target with a length"
    seen = dict(records=len(recs), placed=0, clipped=0, pairs=0, proper=0, borrowed=0, minus=0)
    by_name = {}
    index_of = []
    for f in recs:
        assert len(f) >= 11, f
        qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
        flag, pos, mapq, pnext, tlen = int(flag), int(pos), int(mapq), int(pnext), int(tlen)
        assert re.match(r"r\d+$", qname) and qual == "*" and flag & ~0xFF == 0 and mapq in (0, 60) and re.match(r"[ACGT]+$", seq)
        q = int(qname[1:])
        r = q + 1 if flag & 0x80 else q
        index_of.append(r)
        assert bool(flag & 0x1) == bool(flag & 0xC0) and (flag & 0xC0) != 0xC0, ("exactly one of 0x40 / 0x80 on a paired record, none on a single one", f)
        if not flag & 0x1:
            assert flag & (0x2 | 0x8 | 0x20) == 0 and rnext == "*" and pnext == 0 and tlen == 0, f
        read = _letters(reads[r])
        assert seq == ("".join(COMP[c] for c in reversed(read)) if flag & 0x10 else read), ("SEQ", r)
        tags = dict((t[:4], t[5:]) for t in f[11:])
        if flag & 0x4:
            assert cigar == "*" and mapq == 0 and not tags and not flag & 0x10 and (rname == "*") == (pos == 0), f
            if rname != "*":
                assert flag & 0x1 and not flag & 0x8, ("borrowed from a placed mate", f)
                seen["borrowed"] += 1
        else:
            ops = _cigar(cigar)
            assert sum(n for n, o in ops if o in "MIS") == len(seq), ("query length", f)
            ref = sum(n for n, o in ops if o in "MD")
            assert rname in ln and pos >= 1 and pos - 1 + ref <= ln[rname], ("inside the target", f)
            assert sorted(tags) == ["NM:i", "XP:A"] and tags["XP:A"] in ("H", "G"), f
            if tags["XP:A"] == "H":
                assert len(ops) == 1 and ops[0][1] == "M"
            t, at, qi, diff = targets[tid[rname]], pos - 1, 0, 0
            for n, o in ops:
                if o == "M":
                    diff += sum(1 for i in range(n) if "ACGT"[int(t[at + i])] != seq[qi + i])
                    at, qi = at + n, qi + n
                elif o == "I":
                    diff, qi = diff + n, qi + n
                elif o == "D":
                    diff, at = diff + n, at + n
                else:
                    qi += n
            assert diff == int(tags["NM:i"]), ("NM", f, diff)
            seen["placed"] += 1
            seen["clipped"] += any(o == "S" for _, o in ops)
            seen["minus"] += bool(flag & 0x10)
        if flag & 0x1:
            by_name.setdefault(qname, []).append((f, flag, rname, pos, rnext, pnext, tlen))
    assert index_of == sorted(set(index_of)), "read order, one record per read"
    if complete:
        assert index_of == [r for r in range(len(reads)) if reads[r] is not None and len(reads[r]) >= 1], "one record per live read"
    for qname, mates in by_name.items():
        if len(mates) == 1:
            assert not complete, ("a mate is missing", qname)
            continue
        assert len(mates) == 2, qname
        (fa, a, rna, pa, rxa, pxa, ta), (fb, b, rnb, pb, rxb, pxb, tb) = mates
        assert a & 0x40 and b & 0x80, "the smaller index first"
        for (x, rn, p, rx, px), (y, rny, py) in (((a, rna, pa, rxa, pxa), (b, rnb, pb)), ((b, rnb, pb, rxb, pxb), (a, rna, pa))):
            assert px == py and (rx == "=" and rny == rn != "*" or rx == rny and rx != rn or rx == rny == "*"), ("RNEXT / PNEXT", fa, fb)
            assert bool(x & 0x20) == bool(y & 0x10) and bool(x & 0x8) == bool(y & 0x4), ("the mate's bits", fa, fb)
        assert ta + tb == 0 and (a & 0x2) == (b & 0x2), (fa, fb)
        if a & 0x2:
            assert not (a | b) & 0x4 and rna == rnb and (a & 0x10) != (b & 0x10) and ta != 0
        if ta:
            assert not (a | b) & 0x4 and rna == rnb and (ta > 0) == (pa <= pb), ("TLEN sign", fa, fb)
        seen["pairs"] += 1
        seen["proper"] += bool(a & 0x2)
    return seen
