"""Timings of the break stage (alga_break_placed_device) on a BASELINE shape: a paired read set generated on the device (the recipe of
tools/scaffold_measure.py), the chain build -> cut -> [parallel paths] -> [clip] -> contigs -> consensus -> final contigs, misjoins planted
in the final contigs, every read placed on them, the break, a second placement on the pieces and the scaffolds from it.
    python tools/break_measure.py [--config cfg3_5M_150bp] [--reads N] [--genome-factor F] [--plant K] [--min-length 1800] [--paths 0|1]
                                  [--clip 0|1] [--min-span 1] [--inset 21] [--fasta PATH] [--repeat 3] [--out profiles/break_<config>.jsonl]
--plant K swaps the tails of K randomly chosen pairs of contigs of at least --min-length columns (both tails are half as long as the shorter
contig of the pair, so no length changes): 2 K misjoins at known columns.  A planted misjoin counts as found iff a cut lies within
50 columns of it.
One JSON line per run: alga_break_info (ms_span / ms_cut / ms_total and the counters) beside the same run's placement times (ms_depth does the
same kind of work: atomics per read, a scan over the columns), cuts found against cuts planted, and the N50 before, after the break and after
break -> place -> scaffold; run 0 is marked cold.  --fasta also writes the piece FASTA of the last run and adds its bytes and wall time.
For the per-kernel times run this script under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import alga_amd  # noqa: E402
from alga_amd import workload  # noqa: E402
from extend_measure import paired_device_build  # noqa: E402


def plant(words, begin, lens, k, min_length, seed):
    """swap equally long tails between k pairs of targets of a column-space target set, on the device
    -> new words (int32, the bits of uint32), the planted junctions as columns"""
    import torch
    dev = words.device
    n_cols = int(lens.sum())
    w = words[:(n_cols + 15) // 16].to(torch.int64) & 0xFFFFFFFF
    codes = ((w[:, None] >> (2 * torch.arange(16, device=dev))[None, :]) & 3).reshape(-1)[:n_cols]
    long_ones = torch.nonzero(lens >= min_length).reshape(-1)
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    pick = long_ones[torch.randperm(len(long_ones), generator=g)[:2 * k].to(dev)].cpu().tolist()
    b, n = begin.cpu().tolist(), lens.cpu().tolist()
    perm = torch.arange(n_cols, device=dev)
    junctions = []
    for i, j in zip(pick[0::2], pick[1::2]):
        m = min(n[i], n[j]) // 2
        ai, aj = b[i] + n[i] - m, b[j] + n[j] - m
        perm[ai:ai + m] = torch.arange(aj, aj + m, device=dev)
        perm[aj:aj + m] = torch.arange(ai, ai + m, device=dev)
        junctions += [ai, aj]
    codes = codes[perm]
    pad = (-n_cols) % 16
    codes = torch.cat([codes, torch.zeros(pad + 32, dtype=codes.dtype, device=dev)]).reshape(-1, 16)
    out = (codes << (2 * torch.arange(16, device=dev))[None, :]).sum(dim=1)
    out = torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32).contiguous()
    return out, sorted(junctions)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3_5M_150bp", choices=sorted(workload.CONFIGS))
    ap.add_argument("--reads", type=int, default=0, help="override the config's read count (and scale its genome with it): a quick look")
    ap.add_argument("--genome-factor", type=float, default=1.0, help="stretch the genome (divide the coverage) by this factor")
    ap.add_argument("--plant", type=int, default=0, help="pairs of contigs whose tails are swapped before the placement")
    ap.add_argument("--min-length", type=int, default=1800, help="the shortest contig that takes part in a swap")
    ap.add_argument("--paths", type=int, default=0)
    ap.add_argument("--clip", type=int, default=0)
    ap.add_argument("--min-span", type=int, default=1)
    ap.add_argument("--inset", type=int, default=21)
    ap.add_argument("--fasta", default=None, help="write the piece FASTA of the last run here")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    n, L, G, seed, err = workload.CONFIGS[a.config]
    if a.reads:
        G, n = max(10 * L, int(G * a.reads / n)), a.reads
    G = int(G * a.genome_factor)
    import torch
    ws = paired_device_build(n, L, G, seed, err)
    torch.cuda.synchronize()
    w, l, po = ws["words"], ws["lens"], ws["pair_off"]
    nn = int(l.shape[0])
    mopp = max(250, int(1.75 * L))
    eng = alga_amd.Engine(0)
    sink = open(a.out, "a") if a.out else None
    try:
        d_edges, m = eng.prefsuf_device(w, l, ws["min_overlap"], ws["rsoemo"])
        d_cut, m_cut, _ = eng.cut_triangles_device(nn, d_edges, m, mopp)
        edges = alga_amd.engine.device_view(d_cut, (m_cut, 3), "cuda:0").clone()
        if a.paths:
            edges = eng.remove_short_parallel_paths(nn, edges, mopp)[0].clone()
        if a.clip:
            edges = eng.remove_dangling_branches(nn, edges, mopp)[0].clone()
        u = eng.contigs(w, l, edges, mopp)
        c = eng.unitig_consensus(w, l, u)
        fin = eng.final_contigs(u, c, max(200, int(1.75 * L)), 95, 25)
        # the final contigs as a target set in column space: a break call without pairs cuts nothing and keeps its own copy of the bases
        pl = eng.place_reads(w, l, final=fin, pair_off=po)
        whole = eng.break_contigs(w, l, None, pl, margin=0)
        tw, tb, tl = (x.clone() for x in whole.targets())
        junctions = []
        if a.plant:
            tw, junctions = plant(tw, tb, tl, a.plant, a.min_length, seed)
        planted = torch.tensor(junctions, dtype=torch.int64)
        for r in range(a.repeat):
            pl = eng.place_reads(w, l, targets=(tw, tb, tl), pair_off=po)
            median = int(pl.info["insert_median"])
            bk = eng.break_contigs(w, l, po if median >= 0 else None, pl, margin=max(median, 0), min_span=a.min_span, inset=a.inset)
            cuts = bk.cut_cols.cpu().to(torch.int64) & 0xFFFFFFFF
            found = int(((cuts[None, :] - planted[:, None]).abs().min(dim=1).values <= 50).sum()) if len(planted) and len(cuts) else 0
            out = dict(config=a.config, genome=G, reads=nn // 2, pairs=ws["pairs"], err=err, paths=a.paths, clip=a.clip, run=r, cold=r == 0, min_span=a.min_span,
                       inset=a.inset, margin=max(median, 0), source=alga_amd.engine.source_fingerprint(), contigs=fin.n_written, columns=pl.n_columns,
                       insert_median=median, ms_index=pl.info["ms_index"], ms_place=pl.info["ms_place"], ms_depth=pl.info["ms_depth"],
                       ms_place_total=pl.info["ms_total"], proper_matches=bk.info["pairs_proper"] == pl.info["pairs_proper"] or median < 0, planted=len(junctions),
                       planted_found=found, cuts_elsewhere=int(bk.info["cuts"]) - found, **bk.info)
            if a.fasta and r == a.repeat - 1:
                gi = eng.write_broken_fasta(a.fasta, bk)
                out.update(fasta_bytes=gi["bytes"], fasta_ms_total=gi["ms_total"])
            # break -> place on the pieces -> scaffold
            pl2 = eng.place_reads(w, l, targets=bk.targets(), pair_off=po)
            median2 = int(pl2.info["insert_median"])
            sc = eng.scaffold(w, l, po if median2 >= 0 else None, pl2, insert=max(median2, 0))
            out.update(ms_place2_total=pl2.info["ms_total"], joins_after=sc.info["joins"], scaffolds_after=sc.info["scaffolds"], n50_scaffolds_after=sc.info["n50_scaffolds"],
                       ms_scaffold_total=sc.info["ms_total"])
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
