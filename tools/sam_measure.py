"""Timings of the pair calls over both placement passes (alga_judge_pairs_device) and of the SAM writer (alga_write_sam_device) on a planted set
generated on the device: a random genome cut into targets, read pairs of one length drawn from both strands at inserts of 300 .. 499, a share of
the reads with one planted 1-base insertion or deletion; the Hamming placement, the gapped pass, then the judge and the SAM (to /dev/null).
    python tools/sam_measure.py [--genome 10000000] [--target 50000] [--reads 2000000] [--len 150] [--indel-share 0.1] [--seed 5]
                                [--k 21] [--max-edits 6] [--max-occ 256] [--repeat 3] [--out profiles/sam_<name>.jsonl]
One JSON line per run (run 0 is marked cold): alga_pair_info under `judge` (ms_judge, every counter), ms_format and the bytes of the SAM, and
the same run's yardsticks: the placement's ms_depth (it holds k_pl_pairs) and the ms_format and bytes of alga_write_gapped_tsv_device; the
proper pairs before (the placement's) and after the re-judging."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def planted_pairs(genome, target, reads, L, share, seed, device):
    """-> rows int32 [2 reads, stride], lens int32 [2 reads] in twin layout, pair_off uint8 [2 reads], targets (words int32, begin int64, len
    int32); reads 2i and 2i + 1 are mates: one `+` at the left end of the insert, one `-` at its right end, in either order"""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    reads -= reads & 1
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
    P = reads // 2
    t = torch.randint(0, T, (P,), generator=g, device=device)
    ins_size = torch.randint(300, 500, (P,), generator=g, device=device)
    room = tlen[t] - (ins_size + 2)
    left = (torch.rand(P, generator=g, device=device, dtype=torch.float64) * room.to(torch.float64)).to(torch.int64).clamp_(min=0)
    swap = torch.rand(P, generator=g, device=device) < 0.5           # the `-` mate is the first of the pair
    # per read: its first column and its strand
    a = torch.stack([left, left + ins_size - L], 1)
    minus = torch.stack([torch.zeros_like(swap), torch.ones_like(swap)], 1)
    a = torch.where(swap.unsqueeze(1), a.flip(1), a).reshape(-1)
    minus = torch.where(swap.unsqueeze(1), minus.flip(1), minus).reshape(-1)
    t = t.repeat_interleave(2)
    indel = torch.rand(reads, generator=g, device=device) < share
    dele = indel & (torch.rand(reads, generator=g, device=device) < 0.5)
    ins = indel & ~dele
    at = torch.randint(1, L - 1, (reads,), generator=g, device=device)
    i = torch.arange(L, device=device, dtype=torch.int64).unsqueeze(0)
    src = i + (dele.unsqueeze(1) & (i >= at.unsqueeze(1))).to(torch.int64) - (ins.unsqueeze(1) & (i > at.unsqueeze(1))).to(torch.int64)
    rc = codes[(tbegin[t] + a).unsqueeze(1) + src]
    rc = torch.where(ins.unsqueeze(1) & (i == at.unsqueeze(1)), (rc + 2) & 3, rc)
    fwd = torch.where(minus.unsqueeze(1), 3 - rc.flip(1), rc)
    stride = (L + 15) // 16
    pad = torch.zeros((reads, 16 * stride - L), dtype=torch.int64, device=device)
    rows = torch.empty((2 * reads, stride), dtype=torch.int32, device=device)
    rows[1::2] = pack(torch.cat([fwd, pad], 1))
    rows[0::2] = pack(torch.cat([3 - fwd.flip(1), pad], 1))
    lens = torch.full((2 * reads,), L, dtype=torch.int32, device=device)
    pair_off = torch.tensor([1, 1, 2, 2], dtype=torch.uint8, device=device).repeat(P)
    return rows.contiguous(), lens, pair_off.contiguous(), (twords.contiguous(), tbegin, tlen.to(torch.int32)), int(indel.sum().item())


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
    rows, lens, po, tg, n_indel = planted_pairs(a.genome, a.target, a.reads, a.len, a.indel_share, a.seed, torch.device("cuda", 0))
    torch.cuda.synchronize()
    eng = alga_amd.Engine(0)
    sink = open(a.out, "a") if a.out else None
    try:
        for r in range(a.repeat):
            pl = eng.place_reads(rows, lens, targets=tg, pair_off=po, k=a.k, max_occ=a.max_occ)
            gp = eng.place_gapped(rows, lens, pl, targets=tg, k=a.k, max_edits=a.max_edits, max_occ=a.max_occ)
            tsv = eng.write_gapped_tsv("/dev/null", gp)
            calls = eng.judge_pairs(rows, lens, pl, gapped=gp, pair_off=po)
            sam = eng.write_sam("/dev/null", rows, lens, pl, calls, gapped=gp)
            out = dict(genome=a.genome, targets=int(tg[2].shape[0]), reads=int(lens.shape[0]) // 2, len=a.len, indel_share=a.indel_share, seed=a.seed, run=r, cold=r == 0,
                       k=a.k, max_edits=a.max_edits, max_occ=a.max_occ, source=alga_amd.engine.source_fingerprint(), planted=n_indel,
                       place=dict(placed=pl.info["placed"], pairs_proper=pl.info["pairs_proper"], pairs_not_unique=pl.info["pairs_not_unique"], ms_depth=pl.info["ms_depth"],
                                  ms_total=pl.info["ms_total"]),
                       gapped=dict(placed=gp.info["placed"], ms_total=gp.info["ms_total"]),
                       gapped_tsv=dict(bytes=tsv["bytes"], ms_format=tsv["ms_format"], ns_per_byte=1e6 * tsv["ms_format"] / max(1, tsv["bytes"])),
                       sam=dict(bytes=sam["bytes"], records=sam["segments"], ms_format=sam["ms_format"], ms_total=sam["ms_total"],
                                ns_per_byte=1e6 * sam["ms_format"] / max(1, sam["bytes"])),
                       proper_before=pl.info["pairs_proper"], proper_after=calls.info["pairs_proper"], judge=dict(calls.info))
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
