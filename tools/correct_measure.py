"""Timings and effect of the read error correction (alga_correct_reads_device) on a BASELINE shape with substitution errors, generated on the
device with its genome kept.
    python tools/correct_measure.py [--config cfg2_1M_150bp] [--err 0.005] [--reads N] [--k 21] [--solid 3] [--min-run 1] [--repeat 3]
                                    [--out profiles/correct_<config>.jsonl]
One JSON line per run: alga_correct_info (slices, ms_count / ms_index / ms_fix / ms_total and the run counters); the share of the erroneous
reads that are restored to the genome and the error-free reads that were changed (a read is error-free iff it occurs in the genome, on either
strand: a 64-bit polynomial hash of every genome window against the hash of the read); and the exact build on the reads before and after the
correction, both on this tree in this process: its time (alga_prefsuf_stats.ms_total, best of three), edge count and pile_buckets.  After
the correction reads that have become equal (on either strand) are reduced to one, as the duplicate removal behind the stage would.
For the per-kernel times run this script under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alga_amd  # noqa: E402
from alga_amd import workload  # noqa: E402

B = 0x9E3779B97F4A7C15 - (1 << 64)                              # odd: invertible modulo 2^64 (as a wrapped int64)


def codes_of(rows, m):
    """[n, stride] int32 rows -> [n, m] uint8 bases"""
    import torch
    i = torch.arange(m, device=rows.device)
    return ((rows[:, (i >> 4)].to(torch.int64) >> (2 * (i & 15))[None, :]) & 3).to(torch.uint8)


def powers(n, device):
    import torch
    p = torch.full((n,), B, dtype=torch.int64, device=device)
    p[0] = 1
    return torch.cumprod(p, 0)


def genome_hashes(genome, m):
    """sorted 64-bit hashes of every m-window of the genome"""
    import torch
    pw = powers(m, genome.device)
    g = genome.to(torch.int64) + 1
    out = torch.empty(len(g) - m + 1, dtype=torch.int64, device=g.device)
    CH = 1 << 20
    for s0 in range(0, len(out), CH):
        n = min(CH, len(out) - s0)
        win = g[s0:s0 + n + m - 1].unfold(0, m, 1)
        out[s0:s0 + n] = (win * pw[None, :]).sum(dim=1)
    return torch.sort(out).values


def in_genome(rows, m, sorted_hashes, chunk=1 << 20):
    """per pair of rows: the forward read or its reverse complement occurs in the genome"""
    import torch
    R = rows.shape[0] // 2
    pw = powers(m, rows.device)
    ok = torch.zeros(R, dtype=torch.bool, device=rows.device)
    for s0 in range(0, R, chunk):
        for strand in (0, 1):
            c = codes_of(rows[2 * s0 + strand: 2 * min(R, s0 + chunk) + strand: 2], m).to(torch.int64) + 1
            h = (c * pw[None, :]).sum(dim=1)
            at = torch.searchsorted(sorted_hashes, h).clamp(max=len(sorted_hashes) - 1)
            ok[s0:s0 + len(h)] |= sorted_hashes[at] == h
    return ok


def without_duplicates(rows, lens, m):
    """one pair of every group of pairs whose reads are equal on either strand"""
    import torch
    pw = powers(m, rows.device)
    R = rows.shape[0] // 2
    key = torch.empty(R, dtype=torch.int64, device=rows.device)
    CH = 1 << 20
    for s0 in range(0, R, CH):
        hs = []
        for strand in (0, 1):
            c = codes_of(rows[2 * s0 + strand: 2 * min(R, s0 + CH) + strand: 2], m).to(torch.int64) + 1
            hs.append((c * pw[None, :]).sum(dim=1))
        key[s0:s0 + len(hs[0])] = torch.minimum(hs[0], hs[1])
    order = torch.argsort(key, stable=True)
    first = torch.ones(R, dtype=torch.bool, device=rows.device)
    first[1:] = key[order][1:] != key[order][:-1]
    keep = torch.sort(order[first]).values
    idx = torch.stack([2 * keep, 2 * keep + 1], dim=1).flatten()
    return rows[idx].contiguous(), lens[idx].contiguous()


def build(eng, w, l, lo, rs, repeat=3):
    best, m, st = None, 0, None
    for _ in range(repeat):
        _, m = eng.prefsuf_device(w, l, lo, rs, collect_stats=True)
        st = eng.last_stats()
        best = st["ms_total"] if best is None else min(best, st["ms_total"])
    return dict(ms=best, edges=m, pile_buckets=st["pile_buckets"], pile_irregular=st["pile_irregular"], nodes=int(l.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2_1M_150bp", choices=sorted(workload.CONFIGS))
    ap.add_argument("--err", type=float, default=0.005)
    ap.add_argument("--reads", type=int, default=0, help="override the config's read count (and scale its genome with it): a quick look")
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--solid", type=int, default=3)
    ap.add_argument("--min-run", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    n, L, G, seed, _ = workload.CONFIGS[a.config]
    if a.reads:
        G, n = max(10 * L, int(G * a.reads / n)), a.reads
    import torch
    ws = workload.device_build(n, L, G, seed, err=a.err, return_genome=True)
    torch.cuda.synchronize()
    w, l = ws["words"], ws["lens"]
    m = int(l[1])
    genome = torch.from_numpy(ws["genome_codes"]).to(w.device)
    gh = genome_hashes(genome, m)
    clean_before = in_genome(w, m, gh)
    eng = alga_amd.Engine(0)
    sink = open(a.out, "a") if a.out else None
    try:
        before = build(eng, w, l, ws["min_overlap"], ws["rsoemo"])
        for r in range(a.repeat):
            rows = w.clone()
            torch.cuda.synchronize()
            info = eng.correct_reads_device(rows, l, k=a.k, solid_min=a.solid, min_run=a.min_run)
            out = dict(config=a.config, reads=n, err=a.err, run=r, k=a.k, solid_min=a.solid, min_run=a.min_run, source=alga_amd.engine.source_fingerprint(), **info)
            if r == a.repeat - 1:
                clean_after = in_genome(rows, m, gh)
                changed = (rows[1::2] != w[1::2]).any(dim=1)
                bad = int((~clean_before).sum())
                out.update(erroneous_before=bad, erroneous_after=int((~clean_after).sum()), restored=int((~clean_before & clean_after).sum()),
                           restored_share=float((~clean_before & clean_after).sum()) / max(bad, 1), clean_reads_changed=int((clean_before & changed).sum()),
                           clean_reads_spoilt=int((clean_before & ~clean_after).sum()))
                w2, l2 = without_duplicates(rows, l, m)
                torch.cuda.synchronize()
                out.update(build_before=before, build_after=build(eng, w2, l2, ws["min_overlap"], ws["rsoemo"]))
            line = json.dumps(out)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
    finally:
        if sink:
            sink.close()
        eng.close()


if __name__ == "__main__":
    main()
