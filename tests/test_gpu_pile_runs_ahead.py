"""k_pile_runs_consensus_list with its piles' records read a round ahead (alga_amd/csrc/prefsuf_pile.hip; engine option "pile_runs_ahead"):

  pile_runs_ahead  1: before a block works on round r of its piles it asks for the list entries of round r + 2 and the records of round r + 1;
                   0: every round reads its piles, then works on them.

The option changes when loads are issued and nothing that is computed.  A block takes 32 segments of k_pile_build (192 entries each) and walks
their piles in rounds of 128: the node counts give 1, 32, 33, 64 and 65 segments (one block, a full one, a second block of one segment, two full
blocks, a third), the coverages 3, 30 and 120 from several dozen rounds per block down to a few.  Every case: the graph with the option off and
on, in the pure and the mixed form, equals the pairwise kernels' and the oracle's, and the run-list harness (pile_check) finds no member whose
own list differs from its pile's -- over the look-ahead loop, the plain loop and the tile sweep (pile_runs_list 0), the in-tree reference."""
import numpy as np
import pytest

import alga_amd
from pile_option_common import PB_TILE, PR_SEGS, TK_ROWS, build, counts_of, nodes, option_off_and_on, sorted_keys

OPT = "pile_runs_ahead"
DEFAULTS = {"pile": 1, OPT: 0, "pile_runs_list": 1, "pile_check": 0}
LENGTH = 150
# segments -> nodes (two per read).  1: 128 nodes, no more piles than one round holds; 33 and 65: a last block of one segment, 64 and 192 entries
NODES = {1: 128, 32: 32 * PB_TILE, 33: 32 * PB_TILE + 64, 64: 64 * PB_TILE, 65: 65 * PB_TILE}
CASES = [(segs, cov) for segs in (1, 32, 33, 64, 65) for cov in (3, 30, 120)]


@pytest.fixture(scope="module")
def eng():
    e = alga_amd.Engine(0)
    yield e
    e.close()


def _case(segs, cov):
    n_reads = NODES[segs] // 2
    # (duplicate reads are dropped on the way to nodes: some more are sampled, and the first NODES[segs] nodes -- whole reads, each with its twin -- kept)
    words, lens = nodes(4 * n_reads + 64, LENGTH, max(2 * LENGTH, n_reads * LENGTH // cov), 7000 + 10 * segs + cov)
    assert len(lens) >= NODES[segs], (segs, cov, len(lens))
    words, lens = np.ascontiguousarray(words[:NODES[segs]]), np.ascontiguousarray(lens[:NODES[segs]])
    assert (len(lens) + PB_TILE - 1) // PB_TILE == segs
    lo, rs = alga_amd.derive_params(float(LENGTH - 6))
    return words, lens, lo, rs


@pytest.mark.gpu
@pytest.mark.parametrize("segs,cov", CASES, ids=["segs%d_cov%d" % c for c in CASES])
def test_records_a_round_ahead_change_nothing(eng, segs, cov):
    words, lens, lo, rs = _case(segs, cov)
    want, _ = option_off_and_on(eng, words, lens, lo, rs, OPT, DEFAULTS)
    checked = []
    for settings in ({"pile_runs_list": 1, OPT: 0}, {"pile_runs_list": 1, OPT: 1}, {"pile_runs_list": 0, OPT: 1}):
        got, st = build(eng, words, lens, lo, rs, dict(settings, pile=2, pile_check=1), DEFAULTS)
        assert got.shape == want.shape and (got == want).all(), (segs, cov, settings)
        assert st["pile_list_mismatch"] == 0, (segs, cov, settings, st)
        checked.append(st["pile_list_checked"])
    assert checked[0] == checked[1] == checked[2] and checked[0] > 0, (segs, cov, checked)


@pytest.mark.gpu
def test_the_inputs_hold_blocks_of_one_round_of_a_round_just_begun_and_of_many(eng):
    """From the sorted keys, on the host.  A pile is a k-mer group (up to four) of a bucket of no more than 64 entries, listed in the segment
    of its leftmost member: a block's piles are at most the groups of the buckets that touch its 32 segments (`hi`, a bound), and but for the
    one bucket that may straddle each of its edges (four piles) and buckets whose members differ (none to speak of in an error-free random
    genome) they are the groups of the buckets that start in it (`est`)."""
    seen = set()
    for segs, cov in CASES:
        words, lens, lo, rs = _case(segs, cov)
        keys, shift = sorted_keys(eng, words, lens, lo, rs)
        bfirst, bcount = counts_of(keys >> np.uint64(shift))
        low = np.uint64((1 << (shift - 6)) - 1)
        groups = np.array([len(np.unique(keys[f:f + c] & low)) for f, c in zip(bfirst, bcount)])
        piles = np.where((bcount <= 64) & (groups <= 4), groups, 0)
        span = PR_SEGS * PB_TILE
        for b in range((len(lens) + span - 1) // span):
            lo_e, hi_e = b * span, (b + 1) * span
            hi = int(piles[(bfirst < hi_e) & (bfirst + bcount > lo_e)].sum())
            est = int(piles[(bfirst >= lo_e) & (bfirst < hi_e)].sum())
            print("segs %d cov %d block %d: piles <= %d, about %d (%d rounds)" % (segs, cov, b, hi, est, (est + TK_ROWS - 1) // TK_ROWS))
            if hi <= TK_ROWS:
                seen.add("one round or none")
            if est > TK_ROWS and 8 <= est % TK_ROWS <= 48:
                seen.add("a round just begun")
            if est >= 24 * TK_ROWS:
                seen.add("many rounds")
            if 2 * TK_ROWS < est <= 8 * TK_ROWS:
                seen.add("a few rounds")
    assert seen == {"one round or none", "a round just begun", "many rounds", "a few rounds"}, seen
