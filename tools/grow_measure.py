"""Timings of the grow stage (alga_grow_placed_device) on a BASELINE shape: a paired read set generated on the device (the recipe of
tools/extend_measure.py: fragments of 401 nt, mates of the config's read length), the chain build -> cut -> [parallel paths] -> [clip] ->
contigs -> consensus -> final contigs, every read placed on the final contigs, then rounds of grow -> placement on the grown contigs.
    python tools/grow_measure.py [--config cfg3_5M_150bp] [--reads N] [--genome-factor F] [--paths 0|1] [--clip 0|1] [--rounds 2]
                                 [--min-anchor 63] [--max-mismatches 2] [--min-cover 3] [--min-percent 80] [--max-grow 64] [--fasta PATH]
                                 [--repeat 3] [--out profiles/grow_<config>.jsonl]
--genome-factor F stretches the genome F times under the same reads: at the configs' coverage the chain ends in a single contig with two
ends; at a few-fold coverage it ends in thousands of contigs with gaps between them, which is what growing ends is for.
One JSON line per run and round: alga_grow_info (ms_index / ms_place / ms_build / ms_total and the counters) beside the times of the
placement the round grew from (pl_ms_index / pl_ms_place / pl_ms_depth / pl_ms_total), the ratio of the two ms_place, the contigs and their
columns; run 0 is marked cold.  --fasta also writes the grown FASTA of the last run's last round and adds its bytes and wall time.  For the
per-kernel times run this script under `rocprofv3 --kernel-trace --stats` in a run of its own."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3_5M_150bp", choices=sorted(workload.CONFIGS))
    ap.add_argument("--reads", type=int, default=0, help="override the config's read count (and scale its genome with it): a quick look")
    ap.add_argument("--genome-factor", type=float, default=1.0, help="stretch the genome (divide the coverage) by this factor")
    ap.add_argument("--paths", type=int, default=0)
    ap.add_argument("--clip", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--min-anchor", type=int, default=63)
    ap.add_argument("--max-mismatches", type=int, default=2)
    ap.add_argument("--min-cover", type=int, default=3)
    ap.add_argument("--min-percent", type=int, default=80)
    ap.add_argument("--max-grow", type=int, default=64)
    ap.add_argument("--fasta", default=None, help="write the grown FASTA of the last run's last round here")
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
    params = dict(min_anchor=a.min_anchor, max_mismatches=a.max_mismatches, min_cover=a.min_cover, min_percent=a.min_percent, max_grow=a.max_grow)
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
        for r in range(a.repeat):
            pl = eng.place_reads(w, l, final=fin, pair_off=po)
            for rnd in range(1, a.rounds + 1):
                gw = eng.grow_ends(w, l, pl, **params)
                out = dict(config=a.config, genome=G, reads=nn // 2, pairs=ws["pairs"], err=err, paths=a.paths, clip=a.clip, run=r, cold=r == 0, round=rnd,
                           source=alga_amd.engine.source_fingerprint(), contigs=gw.n_targets, columns=pl.n_columns, placed=pl.info["placed"], unplaced=pl.info["unplaced"],
                           pl_ms_index=pl.info["ms_index"], pl_ms_place=pl.info["ms_place"], pl_ms_depth=pl.info["ms_depth"], pl_ms_total=pl.info["ms_total"],
                           place_ratio=gw.info["ms_place"] / pl.info["ms_place"] if pl.info["ms_place"] else None, **params, **gw.info)
                if a.fasta and r == a.repeat - 1 and (rnd == a.rounds or not gw.info["bases_added"]):
                    gi = eng.write_grown_fasta(a.fasta, gw)
                    out.update(fasta_bytes=gi["bytes"], fasta_ms_total=gi["ms_total"])
                line = json.dumps(out)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                if not gw.info["bases_added"]:
                    break
                pl = eng.place_reads(w, l, targets=gw.targets(), pair_off=po)
    finally:
        if sink:
            sink.close()
        eng.close()


if __name__ == "__main__":
    main()
