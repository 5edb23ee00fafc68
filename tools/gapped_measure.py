"""Timings of the gapped placement (alga_place_gapped_device) on a planted set generated on the device: a random genome cut into targets, reads
of one length drawn from both strands, a share of them with one planted 1-base insertion or deletion; the Hamming placement first, then the
gapped pass over what it left unplaced.
    python tools/gapped_measure.py [--genome 10000000] [--target 50000] [--reads 2000000] [--len 150] [--indel-share 0.1] [--seed 5]
                                   [--k 21] [--max-edits 6] [--max-occ 256] [--repeat 3] [--out profiles/gapped_<name>.jsonl]
One JSON line per run: alga_gapped_info (ms_index / ms_place / ms_trace / ms_depth / ms_total and every counter), the placement's times next to
them as the yardstick, and how many of the planted reads came back UNIQUE on their true target and strand with their start within max_edits of
the true one.  For the per-kernel times run this script under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def planted(genome, target, reads, L, share, seed, device):
    """-> rows int32 [2 reads, stride], lens int32 [2 reads] in twin layout, targets (words int32, begin int64, len int32), and per read the true
    target, the true first column, the strand and whether it carries an indel"""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    T = (genome + target - 1) // target
    tlen = torch.full((T,), target, dtype=torch.int64, device=device)
    tlen[-1] = genome - target * (T - 1)
    tbegin = torch.arange(T, dtype=torch.int64, device=device) * target
    codes = torch.randint(0, 4, (genome,), generator=g, device=device, dtype=torch.int64)

    def pack(c):                                                     # [.., 16 m] codes -> [.., m] words (the bits of uint32 in int32)
        sh = 2 * torch.arange(16, device=device, dtype=torch.int64)
        w = (c.reshape(*c.shape[:-1], -1, 16) << sh).sum(-1)
        return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    gpad = torch.cat([codes, torch.zeros((-genome) % 16 + 32, dtype=torch.int64, device=device)])
    twords = pack(gpad)
    t = torch.randint(0, T, (reads,), generator=g, device=device)
    room = tlen[t] - (L + 1)
    a = (torch.rand(reads, generator=g, device=device, dtype=torch.float64) * room.to(torch.float64)).to(torch.int64).clamp_(min=0)
    indel = torch.rand(reads, generator=g, device=device) < share
    dele = indel & (torch.rand(reads, generator=g, device=device) < 0.5)
    ins = indel & ~dele
    at = torch.randint(1, L - 1, (reads,), generator=g, device=device)
    i = torch.arange(L, device=device, dtype=torch.int64).unsqueeze(0)
    # a deletion skips genome base `at`; an insertion repeats the walk at `at` with another base
    src = i + (dele.unsqueeze(1) & (i >= at.unsqueeze(1))).to(torch.int64) - (ins.unsqueeze(1) & (i > at.unsqueeze(1))).to(torch.int64)
    rc = codes[(tbegin[t] + a).unsqueeze(1) + src]
    rc = torch.where(ins.unsqueeze(1) & (i == at.unsqueeze(1)), (rc + 2) & 3, rc)
    minus = torch.rand(reads, generator=g, device=device) < 0.5
    fwd = torch.where(minus.unsqueeze(1), 3 - rc.flip(1), rc)
    stride = (L + 15) // 16
    pad = torch.zeros((reads, 16 * stride - L), dtype=torch.int64, device=device)
    rows = torch.empty((2 * reads, stride), dtype=torch.int32, device=device)
    rows[1::2] = pack(torch.cat([fwd, pad], 1))
    rows[0::2] = pack(torch.cat([3 - fwd.flip(1), pad], 1))
    lens = torch.full((2 * reads,), L, dtype=torch.int32, device=device)
    return rows.contiguous(), lens, (twords.contiguous(), tbegin, tlen.to(torch.int32)), dict(target=t, start=a, minus=minus, indel=indel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--target", type=int, default=50_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--indel-share", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--max-edits", type=int, default=6)
    ap.add_argument("--max-occ", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    import torch
    import alga_amd
    rows, lens, tg, truth = planted(a.genome, a.target, a.reads, a.len, a.indel_share, a.seed, torch.device("cuda", 0))
    torch.cuda.synchronize()
    eng = alga_amd.Engine(0)
    sink = open(a.out, "a") if a.out else None
    try:
        for r in range(a.repeat):
            pl = eng.place_reads(rows, lens, targets=tg, k=a.k, max_occ=a.max_occ)
            gp = eng.place_gapped(rows, lens, pl, targets=tg, k=a.k, max_edits=a.max_edits, max_occ=a.max_occ)
            tried = (pl.state & 1) == 0
            planted_tried = int((tried & truth["indel"]).sum().item())
            ok = tried & truth["indel"] & ((gp.state & 2) != 0) & (gp.target.to(torch.int64) == truth["target"]) & (((gp.state & 4) != 0) == truth["minus"]) & \
                ((gp.pos.to(torch.int64) - truth["start"]).abs() <= a.max_edits)
            out = dict(genome=a.genome, targets=int(tg[2].shape[0]), reads=a.reads, len=a.len, indel_share=a.indel_share, seed=a.seed, run=r, cold=r == 0, k=a.k,
                       max_edits=a.max_edits, max_occ=a.max_occ, source=alga_amd.engine.source_fingerprint(), planted=int(truth["indel"].sum().item()),
                       planted_unplaced_by_hamming=planted_tried, planted_unique_at_true_locus=int(ok.sum().item()),
                       place=dict(placed=pl.info["placed"], unplaced=pl.info["unplaced"], ms_index=pl.info["ms_index"], ms_place=pl.info["ms_place"],
                                  ms_depth=pl.info["ms_depth"], ms_total=pl.info["ms_total"]), **gp.info)
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
