"""Timings of the extension of contigs by paired connections (alga_extend_contigs_device).
    python tools/extend_measure.py --input f8_pbranch                                  the golden fixture, from the reference's after-simplifier graph
    python tools/extend_measure.py --input cfg3_5M_150bp [--reads N]                   a paired set of the config's shape, after the cut
    python tools/extend_measure.py --input cfg5_10M_150bp_err2 --paths --clip          ... with errors, supplemented, after paths and clip
                                   [--repeat 3] [--out profiles/extend_<input>.jsonl]
A paired set is made on the device: fragments of 401 nt at distinct even starts, mate 1 = the first L nt, mate 2 = the first L nt of the
fragment's reverse complement, the mates swapped at random, the pairs shuffled, interleaved as the ingest interleaves --file1 / --file2 (an odd
fragment length keeps a mate 2 from being the reverse complement of another fragment's mate 1: the set has no duplicates to remove).
One JSON line per run: alga_extend_info (counts and ms_* per stage) next to `contigs_ms_total` -- alga_contigs_device on the same input, the
yardstick -- and N50 / longest of the consensus windows with and without the extension."""
import argparse
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import alga_amd  # noqa: E402
from alga_amd import workload  # noqa: E402

FRAG = 401


def n50(lengths):
    ls = np.sort(np.asarray(lengths, dtype=np.int64))[::-1]
    if not len(ls) or ls.sum() == 0:
        return 0
    return int(ls[np.searchsorted(np.cumsum(ls), (ls.sum() + 1) // 2)])


def paired_device_build(n_reads, L, G, seed, err, trim=3, chunk=1 << 20):
    """-> dict(words, lens, pair_off (device tensors), min_overlap, rsoemo, pairs)"""
    import torch
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    genome = torch.randint(0, 4, (G,), dtype=torch.uint8, device=dev, generator=g)
    starts = torch.unique(2 * torch.randint(0, (G - FRAG + 1) // 2, (n_reads // 2,), device=dev, generator=g))
    R = int(starts.shape[0])
    starts = starts[torch.randperm(R, device=dev, generator=g)]
    swap = torch.rand(R, device=dev, generator=g) < 0.5
    m = L - 2 * trim
    W = (2 * m + 31) // 32
    stride = 4 if W <= 4 else (8 if W <= 8 else (W + 15) & ~15)
    words = torch.zeros((4 * R, stride), dtype=torch.int32, device=dev)
    shifts = (2 * torch.arange(16, device=dev, dtype=torch.int64))[None, None, :]

    def pack(codes):
        codes = torch.cat([codes, torch.zeros((codes.shape[0], W * 16 - m), dtype=codes.dtype, device=dev)], dim=1)
        x = (codes.view(-1, W, 16).to(torch.int64) << shifts).sum(dim=2)
        return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)

    ar = torch.arange(L, device=dev)[None, :]
    for s0 in range(0, R, chunk):
        st = starts[s0:s0 + chunk]
        k = int(st.shape[0])
        one = genome[st[:, None] + ar]
        two = (3 - genome[st[:, None] + (FRAG - L) + ar]).flip(1)
        if err > 0:
            idx = torch.arange(s0, s0 + k, device=dev)
            one = workload._with_errors(one, 2 * idx, err, seed)
            two = workload._with_errors(two, 2 * idx + 1, err, seed)
        sw = swap[s0:s0 + k][:, None]
        a, b = torch.where(sw, two, one)[:, trim:trim + m], torch.where(sw, one, two)[:, trim:trim + m]
        for j, fw in enumerate((a, b)):                                        # read 2p + j: node 4p + 2j + 1 forward, 4p + 2j its reverse complement
            words[4 * s0 + 2 * j + 1: 4 * (s0 + k): 4, :W] = pack(fw)
            words[4 * s0 + 2 * j: 4 * (s0 + k): 4, :W] = pack((3 - fw).flip(1))
    lens = torch.full((4 * R,), m, dtype=torch.int32, device=dev)
    pair_off = torch.tensor([1, 1, 2, 2], dtype=torch.uint8, device=dev).repeat(R)
    lo, rs = alga_amd.derive_params(float(m))
    return dict(words=words, lens=lens, pair_off=pair_off, min_overlap=lo, rsoemo=rs, pairs=R)


def golden_input(name):
    import oracle_lib as O
    gold = os.path.join(ROOT, "tests", "golden")
    fx = O.Fixture(gold, name)
    try:
        f1, f2 = fx.inputs()
        nd = O.ingest(f1, f2)
    finally:
        fx.cleanup()
    with gzip.open(os.path.join(gold, name + ".aftersimplifier.graph.gz"), "rb") as f:
        _, edges = O.parse_graph(f.read())
    return nd["words"], nd["len"], nd["pair_off"], edges, max(250, int(1.75 * nd["LEN"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", default="f8_pbranch", help="f8_pbranch or a config of alga_amd.workload.CONFIGS")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--paths", action="store_true", help="remove the short parallel paths between the cut and the contigs")
    ap.add_argument("--clip", action="store_true", help="clip the tips (after the parallel paths) before the contigs")
    ap.add_argument("--min-votes", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="override the config's read count (and scale its genome with it): a quick look")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    import torch
    eng = alga_amd.Engine(0)
    dev = torch.device("cuda", eng.device)
    m_edges = None
    if a.input in workload.CONFIGS:
        n, L, G, seed, err = workload.CONFIGS[a.input]
        if a.reads:
            G, n = max(10 * L, int(G * a.reads / n)), a.reads
        ws = paired_device_build(n, L, G, seed, err)
        torch.cuda.synchronize()                                  # made on torch's stream; the engine's own stream does not order with it
        w, l, po = ws["words"], ws["lens"], ws["pair_off"]
        nn = int(l.shape[0])
        d, m = eng.prefsuf_device(w, l, ws["min_overlap"], ws["rsoemo"])
        if err > 0:
            m_len = int(l[1])
            d, m = eng.pkb_supplement_device(w, l, d, m, eng.pkb_params(float(m_len), err, min(2 * m_len // 3, 60)))
        mopp = max(250, int(1.75 * L))
        edges, m_edges, _ = eng.cut_triangles_device(nn, d, m, mopp)
        bound = int(mopp * float(int(l[1])) / np.float32(100))
        if a.paths:
            edges, _ = eng.remove_short_parallel_paths(nn, edges, bound, n_edges=m_edges)
            m_edges = None
        if a.clip:
            edges, _ = eng.remove_dangling_branches(nn, edges, bound, n_edges=m_edges)
            m_edges = None
        mcw = int(2 * float(int(l[1])))
    else:
        words, lens, pair_off, edges, mopp = golden_input(a.input)
        w = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev)
        l = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
        po = torch.from_numpy(np.ascontiguousarray(pair_off, dtype=np.uint8)).to(dev)
        nn = int(l.shape[0])
        mcw = int(2 * float(lens[lens > 0].mean()))
    sink = open(a.out, "a") if a.out else None
    try:
        for r in range(a.repeat):
            k = eng.contigs(w, l, edges, mopp, n_edges=m_edges)
            ki = dict(k.info)
            kw = eng.unitig_consensus(w, l, k, min_votes=a.min_votes).len.cpu().numpy()
            k = eng.contigs(w, l, edges, mopp, n_edges=m_edges)               # (the consensus does not change the contigs; a fresh result all the same)
            x = eng.extend_contigs(w, l, po, k, mcw)
            xw = eng.unitig_consensus(w, l, x, min_votes=a.min_votes).len.cpu().numpy()
            out = dict(input=a.input, run=r, nodes=nn, paths=a.paths, clip=a.clip, max_offset=mopp, min_chain_weight=mcw, contigs_ms_total=ki["ms_total"],
                       ms_total_over_contigs_ms_total=x.info["ms_total"] / max(ki["ms_total"], 1e-9), seams=int(x.seams[1].shape[0]),
                       windows=dict(extended_n50=n50(xw), extended_longest=int(xw.max()) if len(xw) else 0, contig_n50=n50(kw),
                                    contig_longest=int(kw.max()) if len(kw) else 0),
                       head_slice=alga_amd.engine.EXTEND_HEAD_SLICE, source=alga_amd.engine.source_fingerprint(), **x.info)
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
