"""Timings of the polish with the gapped reads (alga_polish_indels_device) on a planted set generated on the device: a random genome cut into
targets, one 1-base indel planted per about `--every` columns IN THE TARGETS (half of them a base too many, half a base too few), error-free reads
of one length drawn from both strands of the genome; place -> gapped -> polish (the yardstick) -> polish_indels, in one process.
    python tools/ipolish_measure.py [--genome 10000000] [--target 50000] [--reads 2000000] [--len 150] [--every 5000] [--seed 5]
                                    [--repeat 3] [--out profiles/ipolish_<name>.jsonl]
One JSON line per run (run 0 is marked cold): alga_ipolish_info (ms_votes / ms_inserts / ms_build / ms_total and every counter); beside them the
same run's alga_polish_placed_device ms_sort + ms_vote -- it does the same gather over the H voters alone -- and the times of the placement and of
the gapped pass; the events found against the events planted, counted from the planted truth: the events of the result, and how many targets came
back equal to the genome.  No checker comparison at this size.  For the per-kernel times run this script under `rocprofv3 --kernel-trace --stats`
in a run of its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pack(c, device):
    """[.., 16 m] codes -> [.., m] words (the bits of uint32 in int32)"""
    import torch
    sh = 2 * torch.arange(16, device=device, dtype=torch.int64)
    w = (c.reshape(*c.shape[:-1], -1, 16) << sh).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack(words, n, device):
    import torch
    sh = 2 * torch.arange(16, device=device, dtype=torch.int64)
    w = words.to(torch.int64) & 0xFFFFFFFF
    return ((w.unsqueeze(1) >> sh) & 3).reshape(-1)[:n]


def planted(genome, target, reads, L, every, seed, device):
    """-> rows, lens (twin layout), the targets with their planted indels (words int32, begin int64, len int32), the genome's codes, its targets'
    begin, and the number of planted events"""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    T = (genome + target - 1) // target
    tlen = torch.full((T,), target, dtype=torch.int64, device=device)
    tlen[-1] = genome - target * (T - 1)
    tbegin = torch.arange(T, dtype=torch.int64, device=device) * target
    codes = torch.randint(0, 4, (genome,), generator=g, device=device, dtype=torch.int64)
    # the events: one per `every` columns, at least 200 columns from the ends of its target
    at = torch.arange(every // 2, genome, every, device=device, dtype=torch.int64)
    at = at + torch.randint(0, every // 4, at.shape, generator=g, device=device)
    inside = ((at % target) >= 200) & ((at % target) < tlen[at // target] - 200)
    at = at[inside]
    dele = torch.rand(at.shape, generator=g, device=device) < 0.5      # the target lacks this base / has one more behind it
    counts = torch.ones(genome, dtype=torch.int64, device=device)
    counts[at] = torch.where(dele, torch.zeros_like(at), torch.full_like(at, 2))
    tcodes = torch.repeat_interleave(codes, counts)
    cum = torch.cumsum(counts, 0)
    second = cum[at[~dele]] - 1                                       # the second copy of a doubled base: another base
    tcodes[second] = (tcodes[second] + 2) & 3
    excl = torch.cat([torch.zeros(1, dtype=torch.int64, device=device), cum])
    nb = excl[tbegin]
    nl = excl[tbegin + tlen] - nb
    n_t = int(tcodes.shape[0])
    twords = pack(torch.cat([tcodes, torch.zeros((-n_t) % 16 + 32, dtype=torch.int64, device=device)]), device)
    # the reads: error-free, from the genome
    t = torch.randint(0, T, (reads,), generator=g, device=device)
    a = (torch.rand(reads, generator=g, device=device, dtype=torch.float64) * (tlen[t] - L).to(torch.float64)).to(torch.int64).clamp_(min=0)
    i = torch.arange(L, device=device, dtype=torch.int64).unsqueeze(0)
    rc = codes[(tbegin[t] + a).unsqueeze(1) + i]
    minus = torch.rand(reads, generator=g, device=device) < 0.5
    fwd = torch.where(minus.unsqueeze(1), 3 - rc.flip(1), rc)
    stride = (L + 15) // 16
    pad = torch.zeros((reads, 16 * stride - L), dtype=torch.int64, device=device)
    rows = torch.empty((2 * reads, stride), dtype=torch.int32, device=device)
    rows[1::2] = pack(torch.cat([fwd, pad], 1), device)
    rows[0::2] = pack(torch.cat([3 - fwd.flip(1), pad], 1), device)
    lens = torch.full((2 * reads,), L, dtype=torch.int32, device=device)
    return rows.contiguous(), lens, (twords.contiguous(), nb.contiguous(), nl.to(torch.int32).contiguous()), codes, tbegin, tlen, int(at.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--target", type=int, default=50_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--every", type=int, default=5000)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    import torch
    import alga_amd
    dev = torch.device("cuda", 0)
    rows, lens, tg, codes, gbegin, glen, n_planted = planted(a.genome, a.target, a.reads, a.len, a.every, a.seed, dev)
    torch.cuda.synchronize()
    eng = alga_amd.Engine(0)
    sink = open(a.out, "a") if a.out else None
    try:
        for r in range(a.repeat):
            pl = eng.place_reads(rows, lens, targets=tg)
            gp = eng.place_gapped(rows, lens, pl, targets=tg)
            po = eng.polish(rows, lens, pl)
            ip = eng.polish_indels(rows, lens, pl, gp)
            new = unpack(ip.words, ip.n_columns, dev)
            off = ip.col_off.to(torch.int64) & 0xFFFFFFFF
            same_len = (off[1:] - off[:-1]) == glen
            restored = 0
            if bool(same_len.all()) and ip.n_columns == a.genome:
                wrong = torch.zeros(a.genome + 1, dtype=torch.int64, device=dev)
                wrong[:a.genome] = (new != codes).to(torch.int64)
                c = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(wrong[:a.genome], 0)])
                restored = int(((c[gbegin + glen] - c[gbegin]) == 0).sum().item())
            else:
                restored = int(same_len.sum().item())                 # (an upper bound: only the lengths were compared)
            out = dict(genome=a.genome, targets=int(tg[2].shape[0]), reads=a.reads, len=a.len, every=a.every, seed=a.seed, run=r, cold=r == 0,
                       source=alga_amd.engine.source_fingerprint(), planted=n_planted, events=ip.n_events, targets_equal_to_the_genome=restored,
                       lengths_all_restored=bool(same_len.all()),
                       place=dict(placed=pl.info["placed"], unplaced=pl.info["unplaced"], ms_index=pl.info["ms_index"], ms_place=pl.info["ms_place"],
                                  ms_depth=pl.info["ms_depth"], ms_total=pl.info["ms_total"]),
                       gapped={k: gp.info[k] for k in ("tried", "placed", "unique", "ms_index", "ms_place", "ms_trace", "ms_depth", "ms_total")},
                       polish=dict(ms_sort=po.info["ms_sort"], ms_vote=po.info["ms_vote"], ms_total=po.info["ms_total"], changed=po.info["changed"]), **ip.info)
            out["ratio_votes_to_polish"] = (ip.info["ms_votes"] + ip.info["ms_inserts"] + ip.info["ms_build"]) / max(po.info["ms_sort"] + po.info["ms_vote"], 1e-9)
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
