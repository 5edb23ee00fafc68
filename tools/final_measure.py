"""Timings of the final contig set (alga_final_contigs_device): the graph of a BASELINE config, built on the device (supplemented when the config
has errors), cut by the first simplifier step, optionally without its short parallel paths and tips; the contigs and their consensus; then the
new-read filter, the numbering and the trim of the contig ends against each other, and the FASTA.
    python tools/final_measure.py [--config cfg2_1M_150bp] [--repeat 3] [--paths] [--clip] [--min-votes 3] [--min-length N] [--percent 95]
                                  [--threshold 25] [--reads N] [--out profiles/final_<config>.jsonl]
One JSON line per run: alga_final_info (pairs per verdict, filter_rounds, trim_edges, ms_filter / ms_trim / ms_total), and beside it two
yardsticks of the same run: `contigs_ms_total` -- alga_contigs_device on the same input -- and `host_route`: what the tree offered before this
call for the trim alone (download the windows of the accepted contigs, pad them to one stride, alga_contig_trim_host), its wall time or, where
it refuses (a contig above 4 194 303 nt, rows above 64 GB), the refusal."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alga_amd  # noqa: E402
from alga_amd import workload  # noqa: E402


def host_route(eng, u, c, fin, threshold):
    """-> dict(ms=wall, equal=the same trim_left) or dict(refused=message)"""
    t0 = time.perf_counter()
    order = fin.order.cpu().numpy()
    if not len(order):
        return dict(ms=0.0, equal=True)
    wo = u.word_off.cpu().numpy()
    clen = c.len.cpu().numpy()[order]
    ctrim = c.trim_left.cpu().numpy()[order]
    if int(clen.max()) > 4194303:
        return dict(refused="a window of %d nt: alga_contig_trim_host stops at 4 194 303" % int(clen.max()))
    stride = (int(clen.max()) + 15) // 16
    if 2 * len(order) * stride * 4 > (64 << 30):
        return dict(refused="%d rows of %d words: more than 64 GB at one stride" % (2 * len(order), stride))
    words = c.words.cpu().numpy().view(np.uint32)
    rows = np.zeros((len(order), stride), dtype=np.uint32)
    for j, k in enumerate(order.tolist()):
        q = int(ctrim[j]) + np.arange(int(clen[j]), dtype=np.int64)
        codes = (words[int(wo[k]) + (q >> 4)] >> (2 * (q & 15)).astype(np.uint32)) & np.uint32(3)
        pad = np.zeros(16 * stride, dtype=np.uint64)
        pad[: len(codes)] = codes
        rows[j] = (pad.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
    try:
        got = eng.contig_trim(rows, clen.astype(np.int32), threshold)
    except alga_amd.AlgaError as e:
        return dict(refused=str(e))
    ms = (time.perf_counter() - t0) * 1e3
    return dict(ms=ms, equal=bool((got == fin.trim_left.cpu().numpy()[order]).all()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2_1M_150bp", choices=sorted(workload.CONFIGS))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--paths", action="store_true", help="remove the short parallel paths between the cut and the contigs")
    ap.add_argument("--clip", action="store_true", help="clip the tips (after the parallel paths) before the contigs")
    ap.add_argument("--min-votes", type=int, default=3)
    ap.add_argument("--min-length", type=int, default=-1, help="default: max(200, int(1.75 * read length))")
    ap.add_argument("--percent", type=int, default=95)
    ap.add_argument("--threshold", type=int, default=25)
    ap.add_argument("--reads", type=int, default=0, help="override the config's read count (and scale its genome with it): a quick look")
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    n, L, G, seed, err = workload.CONFIGS[a.config]
    if a.reads:
        G, n = max(10 * L, int(G * a.reads / n)), a.reads
    min_length = a.min_length if a.min_length >= 0 else max(200, int(1.75 * L))
    import torch
    ws = workload.device_build(n, L, G, seed, err=err)
    torch.cuda.synchronize()                                      # made on torch's stream; the engine's own stream does not order with it
    eng = alga_amd.Engine(0)
    w, l = ws["words"], ws["lens"]
    nn = int(l.shape[0])
    d, m = eng.prefsuf_device(w, l, ws["min_overlap"], ws["rsoemo"])
    if err > 0:
        m_len = int(l[1])
        d, m = eng.pkb_supplement_device(w, l, d, m, eng.pkb_params(float(m_len), err, min(2 * m_len // 3, 60)))
    mopp = max(250, int(1.75 * L))
    d, m, _ = eng.cut_triangles_device(nn, d, m, mopp)
    # the trim runs a build of its own on the engine: the graph has to outlive it
    edges = alga_amd.engine.device_view(d, (m, 3), "cuda:%d" % eng.device).clone()
    bound = int(mopp * float(int(l[1])) / np.float32(100))
    if a.paths:
        edges = eng.remove_short_parallel_paths(nn, edges, bound)[0].clone()
    if a.clip:
        edges = eng.remove_dangling_branches(nn, edges, bound)[0].clone()
    sink = open(a.out, "a") if a.out else None
    fasta = os.path.join(tempfile.mkdtemp(prefix="alga_final_"), "final.fasta")
    try:
        for r in range(a.repeat):
            k = eng.contigs(w, l, edges, mopp)
            kc = eng.unitig_consensus(w, l, k, min_votes=a.min_votes)
            fin = eng.final_contigs(k, kc, min_length, a.percent, a.threshold)
            fi = eng.write_final_fasta(fasta, fin)
            lens = fin.len.cpu().numpy()
            out = dict(config=a.config, reads=n, run=r, nodes=nn, paths=a.paths, clip=a.clip, min_votes=a.min_votes, min_length=min_length, percent=a.percent,
                       threshold=a.threshold, n_accepted=fin.n_accepted, n_written=fin.n_written, longest_written=int(lens.max()) if len(lens) else 0,
                       nonzero_trims=int((fin.trim_left > 0).sum()), contigs_ms_total=k.info["ms_total"], consensus_ms_total=kc.info["ms_total"],
                       ms_total_over_contigs_ms_total=fin.info["ms_total"] / max(k.info["ms_total"], 1e-9), fasta_bytes=fi["bytes"], fasta_ms_total=fi["ms_total"],
                       source=alga_amd.engine.source_fingerprint(), **fin.info)
            if not a.no_host_route and r == a.repeat - 1:
                out["host_route"] = host_route(eng, k, kc, fin, a.threshold)
            line = json.dumps(out)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
    finally:
        if sink:
            sink.close()
        if os.path.exists(fasta):
            os.remove(fasta)
        os.rmdir(os.path.dirname(fasta))
        eng.close()


if __name__ == "__main__":
    main()
