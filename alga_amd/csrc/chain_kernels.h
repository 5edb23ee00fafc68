// alga_amd/csrc/chain_kernels.h -- the chain core (chain_kernels.hip; device templates in chain_device.h): end-to-end joins between contigs turned
// into ordered, oriented paths, for the scaffolder, the merge stage and the stitch stage.  State x = 2c + e is "contig c entered at end e": it is
// left at end x ^ 1 through that end's join, so succ(x) = join[x ^ 1].  Two phases of pointer jumping over the 2T states: cycles (the smallest
// contig id rides along; a state that still has a successor afterwards is on a cycle, and the contig that is its own minimum drops the join at
// its end 2c), then ranks over the paths that are left (states, weights and the last state to the path's end).  Then per contig the direction
// whose first contig has the smaller id, and ids and member lists from two scans.  DESIGN.md, "The chain core", has the table of pieces.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct alga_engine;

namespace alga {

constexpr int      CHAIN_BLOCK = 256;
constexpr uint32_t CHAIN_NONE = 0xFFFFFFFFu;                              // no successor / no join (a memset of 0xFF)

// the lists over the 2T states, twice: a jump reads one set and writes the other
struct ChainLists {
    unsigned long long *wsum;         // rank phase: the weights summed from here to the list's end
    uint32_t *nxt, *aux, *tail;       // aux: the smallest contig id seen (cycle phase) / the states from here to the list's end (rank phase)
};
// the engine's one chain workspace, carved for T contigs: nothing in it outlives a call
struct ChainWork {
    ChainLists set[2];
    uint32_t *join;                   // 2T + 2: the join of every end, for a stage that keeps none of its own
    uint32_t *head, *first, *members; // T + 2 each: a contig's first contig; 1 / the path's contigs where it is that contig itself, else 0; entry T is 0
    uint32_t *first_scan, *members_scan;   // the exclusive scans: entry T holds the totals
};

// max_blocks: the cap of the launch's grid (block 256; at least 1 block)
void launch_ch_cycle_init(const uint32_t *join, uint64_t n_states, const ChainLists &l, uint32_t max_blocks, hipStream_t s);
void launch_ch_cycle_jump(uint64_t n_states, const ChainLists &from, const ChainLists &to, uint32_t max_blocks, hipStream_t s);
void launch_ch_rank_jump(uint64_t n_states, const ChainLists &from, const ChainLists &to, uint32_t max_blocks, hipStream_t s);

}  // namespace alga

// The workspace for T contigs and the scan scratch, ensured and carved.  One workspace serves the three stages: a stage call ends with the
// wait for its stream (AlgaStageCall), so no call finds another's kernels still reading it.
int alga_chain_work(alga_engine *e, uint64_t T, alga::ChainWork *w);
// The phases: init from join[] (cycles) or the stage's own init kernel into set[0] (ranks), then ceil(log2(n_states)) + 1 jumps (after so many
// doublings a jump is longer than any path); *res = the set that holds the result.  may_join false (the counts say there is no join): no
// launch, *res = null (cycles: there is none) or set[0] (ranks: paths of one).
int alga_chain_cycles(alga_engine *e, const alga::ChainWork &w, const uint32_t *join, uint64_t n_states, bool may_join, uint32_t max_blocks, hipStream_t s,
                      const alga::ChainLists **res);
int alga_chain_ranks(alga_engine *e, const alga::ChainWork &w, uint64_t n_states, bool may_join, uint32_t max_blocks, hipStream_t s, const alga::ChainLists **res);
// first_scan and members_scan from first and members (T + 1 entries each)
int alga_chain_scans(alga_engine *e, const alga::ChainWork &w, uint64_t T, const char *what, hipStream_t s);
