// alga_amd/host/alga_hip_main.cpp -- `alga_hip`: ALGA's command line in front of the MI355X overlap engine.
//
//   alga_hip --file1=reads.fasta [--file2=mates.fasta] --output=contigs.fasta [--threads=N] [--error_rate=R | --error-rate=R]
//            [--serialize=1] [-l MINOVERLAP] [--rsoemo=N] [--scale=F] [--retl=N --retr=N] [--remove_reads_with_n=0|1] [--rna=0|1]
//            [--device=K] [--gpus=N | --gpu-list=0,1,2,...] [--alga=/path/to/stock/ALGA] [--gfa=graph.gfa] [--unitigs=unitigs.gfa] [--clip_tips=0|1]
//            [--parallel_paths=0|1] [--consensus=unitigs.fasta] [--consensus_min_length=200] [--consensus_min_votes=3]
//            [--contigs=contigs.fasta] [--contigs_gfa=contigs.gfa] [--contigs_min_length=N]
//            [--contigs_final=final.fasta] [--contigs_new_reads_percent=95] [--contigs_trim_threshold=25] [--paired_extend=0|1]
//            [--correct_reads=0|1] [--correct_k=21] [--correct_solid=3] [--corrected_reads=reads.fasta]
//            [--contigs_depth=0|1] [--placements=placements.tsv] [--polish=0|1] [--polish_changes=changes.tsv]
//
// --gpus=N: the overlap graph on the GPUs K .. K+N-1 of this node (alga_multi_*, include/alga_amd.h: one host thread and one engine
// per GPU, keys and edge lists exchanged over RCCL / xGMI) -- the counterpart of the reference's --threads for this stage
// (src/Params.cpp:237-294).  Every GPU runs the input stage on the files itself (each over its own PCIe link), so no node set
// crosses xGMI.  --gpu-list names the devices explicitly; a device named more than once selects the copy transport (testing).
//
// It reads the input exactly like the reference (src/IO/InputReader.cpp, src/IO/ReadPreprocess.cpp, src/main.cpp:93-266),
// builds the overlap graph on the GPU and writes `<TEST_NAME>_beforeSimplifier.graph` in the reference's own dump
// format (src/DataStructures/Graph.cpp:269-297).  Stock ALGA started with the same arguments plus
// --deserialize_graph=1 loads that file instead of running its GraphCreator (src/main.cpp:242) and carries on with
// the unchanged simplifier / contig stages; `--alga=` does that hand-off in one go.
// Both spellings of the error-rate option are accepted (the reference registers `error_rate` only, src/Params.cpp:226).
// --gfa=PATH also writes that graph (after the supplement, rank 0's under --gpus) as GFA 1.0 with sequences, formatted on the GPU
// (alga_write_gfa_device); it is not handed on to stock ALGA.
// --unitigs=PATH: after the build (and the supplement), on the device: the first simplifier step (alga_cut_triangles_device with the reference's
// max(250, int(1.75 * LEN))), then the unitig graph without isolated reads (alga_unitigs_device), written as GFA 1.0 with the spelled
// sequences.  The graph handed on to stock ALGA and --gfa= are what they are without it; the option is not passed through.
// --clip_tips=1 (default 0: every invocation without it behaves as before): with --unitigs=, the dangling branches go between the cut and the
// unitigs (alga_remove_dangling_branches_device: GraphSimplifier::removeDanglingBranches / removeDanglingUpperBranches iterated as in
// simplifyGraphOld), build -> supplement -> cut -> clip -> unitigs -> GFA.  The bound is the reference's,
// int(max(250, int(1.75 * LEN)) * AVG_READ_LENGTH / 100.0f) with AVG_READ_LENGTH the integer mean length of the live reads
// (Global::calculateAvgReadLength).  Without --unitigs= it does nothing; it is not passed through.
// --parallel_paths=1 (default 0: every invocation without it behaves as before): with --unitigs=, the short parallel paths go between the cut and
// the clip (alga_remove_short_parallel_paths_device: GraphSimplifier::removeShortParallelPaths), build -> supplement -> cut -> parallel paths ->
// clip (with --clip_tips=1) -> unitigs -> GFA.  The bound is the reference's, int(double(max(250, int(1.75 * LEN)) * AVG_READ_LENGTH) / 100.0f)
// with the same AVG_READ_LENGTH.  Without --unitigs= it does nothing; it is not passed through.
// --consensus=PATH: the same chain as --unitigs= (it honours --clip_tips and --parallel_paths, and works with or without --unitigs=), then the
// consensus of every unitig (alga_unitig_consensus_device: each column a majority vote of the reads over it, the ends cut back to the first / last
// column with more than --consensus_min_votes votes -- Contig::correctSnipsInContig, whose THR is 3), written as FASTA for the windows of at
// least --consensus_min_length bases (alga_write_consensus_fasta_device).  --unitigs= still writes the spelled sequences.  None of the three
// options is passed through; every invocation without --consensus= behaves as before.
// --contigs=PATH: the same chain up to the clip (it honours --parallel_paths and --clip_tips), then the contigs (alga_contigs_device: contract, cut the
// contracted graph with the cut's own bound, contract again), their consensus with --consensus_min_votes, written as FASTA with the reference's
// record names (`>contig_id=<j>_length=<len>`) for the windows of at least --contigs_min_length bases (default max(200, int(1.75 * LEN)),
// src/main.cpp:94); --contigs_gfa=PATH beside it: the contig graph with the spelled sequences.  No stock binary (--alga=) is needed for these
// contigs.  None of the three options is passed through; every invocation without them behaves as before.
// --contigs_final=PATH: the same chain through the contigs and their consensus (with or without --contigs=; it honours --contigs_min_length and
// --consensus_min_votes), then the final set (alga_final_contigs_device: OutputWriterNew::filterContigs' length and new-read filter longest first with
// --contigs_new_reads_percent, the numbering, the trim of the contig ends against each other at --contigs_trim_threshold, 0 = none), written as
// FASTA in id order (alga_write_final_fasta_device).  None of the three options is passed through.
// --paired_extend=1 (default 0; honoured by --contigs=, --contigs_gfa= and --contigs_final=; not passed through): with --file2 the contigs are
// extended through the junctions that paired reads support (alga_extend_contigs_device: min_chain_weight = int(2 * mean length of the live reads),
// 5 connections, inserts up to 1000) before the GFA, the consensus and the final set are made.  Without --file2 it changes nothing and says so.
// --correct_reads=1 (default 0: every invocation without it behaves as before): the reads are parsed on the host cores, corrected on the GPU
// (alga_correct_parsed_reads: k-mer spectrum with --correct_k, solid from --correct_solid occurrences on, one substitution per weak run) and join
// the GPU again at the duplicate / prefix removal; the counters go to stderr.  --corrected_reads=PATH writes the corrected forward reads as
// FASTA (from the rows the call brought back; the sequences are the trimmed ones: a run on that file needs --retl=0 --retr=0).  None of the four
// is passed through, and with --alga= they are refused: stock ALGA would read the original files, whose nodes are not this graph's.
// --contigs_depth=1 (default 0; needs --contigs_final=): every input read -- the files parsed again, corrected again with --correct_reads=1 -- is
// placed on the final contigs (alga_place_reads_on_final_device), the FASTA headers end in `_reads=<n>_depth=<q>.<dd>` and one line on stderr
// gives placed / unique / multi / unplaced reads, proper pairs and the median insert.  --placements=PATH (needs --contigs_final= too): one line
// `read target pos strand mm hits` per read, tab separated, target -1 and strand `.` for an unplaced read.  With both off every file is what it
// was without them; neither is passed through.
// --polish=1 (default 0; needs --contigs_final= and implies the placement): every column of the final contigs is voted again by every uniquely
// placed read (alga_polish_placed_device with its defaults: cover 3, 60 %) and the final FASTA holds the polished sequences
// (alga_write_polished_fasta_device); its headers carry the depth iff --contigs_depth=1.  One line on stderr gives voters / voted columns /
// changed / ambiguous.  --polish_changes=PATH (needs --polish=1): one line `contig pos old new A C G T` per changed column, tab separated, no
// header line, the four counts of the column behind the bases.  Neither is passed through.
// --scaffolds=PATH (needs --contigs_final= and --file2=; implies the placement): the final contigs joined through the pairs whose mates lie on two
// of them (alga_scaffold_placed_device: insert = the placement's median, max_insert the placement's; --scaffold_min_links= (5), --scaffold_min_gap= (10),
// --scaffold_max_second_percent= (50)), one record `>scaffold_id=<j>_length=<len>_contigs=<m>` per scaffold with the gaps as runs of N
// (alga_write_scaffold_fasta_device); with --polish=1 the bases are the polished ones.  --scaffold_layout=PATH (needs --scaffolds=): one line
// `scaffold rank contig orient(+/-) start length gap_after links` per member contig, tab separated.  One line on stderr gives links / bundles
// supported / joins / scaffolds / N50 of the contigs -> N50 of the scaffolds.  Without a proper pair (no median) the scaffolding is skipped with a
// message and every contig is its own scaffold in the FASTA.  None is passed through.
// --break_misjoins=1 (default 0; needs --contigs_final= and --file2=; implies the placement): the final contigs are cut where no proper pair spans
// them (alga_break_placed_device: --break_min_span= (1), --break_inset= (21), --break_margin= (the placement's median insert)).  --broken=PATH: the
// pieces as FASTA, `>contig_id=<j>_length=<len>_from=<t>_start=<s>` (alga_write_broken_fasta_device); --break_cuts=PATH: one line
// `contig cut run_first run_last` per cut, tab separated, in the contig's own columns (both need --break_misjoins=1).  One line on stderr gives
// proper and spanning pairs, weak columns, runs with the open ones, cuts, contigs cut, pieces, N50 of the contigs -> N50 of the pieces.  With
// --polish=1 the pieces carry the polished bases.  With --scaffolds= the same reads are placed a second time, on the pieces, and the scaffolds and
// their layout come from that placement (contig ids there are piece ids).  Without a proper pair nothing is cut, with a message: every contig is
// one piece.  Without --break_misjoins=1 every file is what it was.  None is passed through.
// --grow_ends=N (rounds, 0 .. 16, default 0; needs --contigs_final=; implies the placement): the ends of the contigs (with --break_misjoins=1: of
// the pieces, on which the reads are then placed also without --scaffolds=) grow with the unplaced reads that hang over them (alga_grow_placed_device:
// --grow_min_anchor= (63), --grow_max_mismatches= (2), --grow_min_cover= (3), --grow_min_percent= (80), --grow_max= (64)).  A round is a grow on
// the current placement and then a placement of the same reads on the grown contigs; the rounds end early when one adds no base.  They run
// behind the break and before the scaffolder: the scaffolds and their layout come from the last placement.  With --polish=1 the first round
// takes the polished bases (unless the break already carried them into the pieces); later rounds grow what the round before left.
// --grown=PATH: the contigs after the last round that ran, `>contig_id=<t>_length=<len>_left=<xl>_right=<xr>` with xl / xr that round's growth
// (alga_write_grown_fasta_device); --grow_layout=PATH: one line `contig left right voters_left voters_right stop_left stop_right` per contig of
// that round, tab separated (both need --grow_ends >= 1).  One line on stderr per round gives candidates / voting reads / ends grown / bases
// added / N50 before -> after.  Without --grow_ends every file is what it was.  None is passed through.
// --merge_ends=1 (default 0; needs --grow_ends >= 1): after the last grow round the grown contigs whose ends overlap are merged into one
// (alga_merge_targets_device: --merge_min_overlap= (42), --merge_max_mismatches= (1)), the reads are placed again on the merged contigs, and the
// scaffolds and their layout come from that placement (contig ids there are merged ids).  --merged=PATH: the merged contigs,
// `>contig_id=<j>_length=<len>_contigs=<m>` (alga_write_merged_fasta_device); --merge_layout=PATH: one line `merged rank contig orient start
// length overlap_after mm` per member, tab separated (both need --merge_ends=1).  One line on stderr gives overlaps / ambiguous ends / joins /
// bases removed / N50 before -> after.  Without --merge_ends=1 every file is what it was.  None is passed through.
// --drop_contained=1 (default 0; needs --merge_ends=1): the merged contigs whose whole sequence, or its reverse complement, lies inside a longer
// one within --contain_max_permille= (10) substitutions per 1000 bases are dropped (alga_drop_contained_device), the reads are placed on the kept
// contigs instead of the merged ones, and the scaffolds and their layout come from that placement (contig ids there are kept ids).
// --kept=PATH: the kept contigs, `>contig_id=<j>_length=<len>_absorbed=<m>` (alga_write_kept_fasta_device); --contain_layout=PATH: one line
// `contig length state new host host_pos host_orient mm hits root root_pos root_orient` per merged contig, tab separated (both need
// --drop_contained=1).  One line on stderr gives queries / candidates / contained (minus, duplicates) / ambiguous / bases removed / N50 before ->
// after.  Without --drop_contained=1 every file is what it was.  None is passed through.
// --stitch=1 (default 0; needs --scaffolds=): the placement the scaffolds would be made from is scaffolded a first time, the joins whose two contig
// ends overlap are stitched into one sequence (alga_stitch_scaffolds_device: --stitch_min_overlap= (16), --stitch_max_mismatches= (2),
// --stitch_slack= (2^20); with --polish=1 the bases are the polished ones), the reads are placed again on the stitched contigs, and --scaffolds= and
// --scaffold_layout= describe the scaffolding of that placement (contig ids there are stitched ids).  --stitched=PATH: the stitched contigs,
// `>contig_id=<j>_length=<len>_contigs=<m>` (alga_write_stitched_fasta_device); --stitch_layout=PATH: one line `stitched rank contig orient start
// length overlap_after mm` per member, tab separated (both need --stitch=1).  One line on stderr gives selected / with an overlap / ambiguous /
// stitched / bases removed / N50 before -> after.  Without --stitch=1 every file is what it was.  None is passed through.
// --gapped=1 (default 0; needs --contigs_final=; implies the placement): behind the placement on the final contigs the reads it left unplaced are
// laid onto the same contigs by edit distance (alga_place_gapped_device: --gapped_edits= (6, 1 .. 15)).  --gapped_placements=PATH (needs
// --gapped=1): one line `read target pos end strand edits unique cigar` per gapped-placed read, tab separated, formatted on the device
// (alga_write_gapped_tsv_device).  One line on stderr gives tried / placed / unique / with indel / edits.  It changes no other output: the depth
// headers and --placements= are the Hamming placement's.  Neither is passed through.
// --polish_indels=1 (default 0; needs --gapped=1): the final contigs voted by the Hamming-placed and the gapped reads together
// (alga_polish_indels_device: --polish_max_ins= (6, 1 .. 13)): columns substituted or deleted, strings inserted, contigs that change length.
// --ipolished=PATH: the new contigs, `>contig_id=<t>_length=<len>_subs=<s>_ins=<i>_dels=<d>` (alga_write_ipolished_fasta_device);
// --ipolish_events=PATH: one line `contig pos kind len old new votes cover` per event, tab separated (alga_write_ipolish_events_tsv_device); both
// need --polish_indels=1.  One line on stderr gives voters / substituted / deleted / inserted / ambiguous / columns before -> after.  Like
// --gapped it changes no other output.  None is passed through.
// --sam=PATH (needs --contigs_final=; implies the placement): every input read as a SAM record on the final contigs, from the first placement
// (alga_judge_pairs_device with the placement's max_insert, alga_write_sam_device; formatted on the device).  With --gapped=1 the gapped reads
// are in it with their CIGARs and the pairs are judged over both passes; with --contigs_depth=1 the @SQ names are the depth form, the first
// token of the headers the same run writes to --contigs_final=.  --sam_unplaced=0 (default 1; needs --sam=): no records for unplaced reads.
// QNAME is r<read index> (the engine keeps no read names), QUAL is `*`.  One line on stderr gives pairs / proper / improper / split / not unique,
// the pairs and proper pairs with a gapped mate and the median insert.  --sam= with --polish=1 is refused: NM and the names would describe
// sequences the FASTA no longer holds.  It changes no other output.  Neither is passed through.
#include <spawn.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "GraphCreatorHIP.hpp"
#include "ingest.hpp"

static const char *USAGE =
    "alga_hip --file1=reads.fasta [--file2=mates.fasta] --output=contigs.fasta [--threads=N] [--error_rate=R] [--serialize=1] [-l MINOVERLAP] [--rsoemo=N]\n"
    "         [--scale=F] [--retl=N --retr=N] [--remove_reads_with_n=0|1] [--rna=0|1] [--device=K] [--gpus=N | --gpu-list=0,1,...] [--alga=/path/to/ALGA]\n"
    "         [--gfa=graph.gfa] [--unitigs=unitigs.gfa] [--clip_tips=0|1] [--parallel_paths=0|1] [--consensus=unitigs.fasta] [--consensus_min_length=200]\n"
    "         [--consensus_min_votes=3] [--contigs=contigs.fasta] [--contigs_gfa=contigs.gfa] [--contigs_min_length=N] [--contigs_final=final.fasta]\n"
    "         [--contigs_new_reads_percent=95] [--contigs_trim_threshold=25] [--paired_extend=0|1]\n"
    "         [--correct_reads=0|1] [--correct_k=21 (odd, 5 .. 31)] [--correct_solid=3] [--corrected_reads=reads.fasta]\n"
    "         [--contigs_depth=0|1] [--placements=placements.tsv] [--polish=0|1] [--polish_changes=changes.tsv]\n"
    "         [--scaffolds=scaffolds.fasta] [--scaffold_layout=layout.tsv] [--scaffold_min_links=5] [--scaffold_min_gap=10] [--scaffold_max_second_percent=50]\n"
    "         [--break_misjoins=0|1] [--break_min_span=1] [--break_inset=21] [--break_margin=N] [--broken=pieces.fasta] [--break_cuts=cuts.tsv]\n"
    "         [--grow_ends=N] [--grown=grown.fasta] [--grow_layout=grow.tsv] [--grow_min_anchor=63] [--grow_max_mismatches=2] [--grow_min_cover=3]\n"
    "         [--grow_min_percent=80] [--grow_max=64]\n"
    "         [--merge_ends=0|1] [--merged=merged.fasta] [--merge_layout=merge.tsv] [--merge_min_overlap=42] [--merge_max_mismatches=1]\n"
    "         [--drop_contained=0|1] [--kept=kept.fasta] [--contain_layout=contain.tsv] [--contain_max_permille=10]\n"
    "         [--stitch=0|1] [--stitched=stitched.fasta] [--stitch_layout=stitch.tsv] [--stitch_min_overlap=16] [--stitch_max_mismatches=2] [--stitch_slack=1048576]\n"
    "         [--gapped=0|1] [--gapped_edits=6] [--gapped_placements=gapped.tsv]\n"
    "         [--polish_indels=0|1] [--polish_max_ins=6] [--ipolished=ipolished.fasta] [--ipolish_events=events.tsv]\n"
    "         [--sam=reads.sam] [--sam_unplaced=0|1]\n";

static bool opt(const char *arg, const char *name, std::string &val) {
    size_t n = strlen(name);
    if (strncmp(arg, name, n) == 0 && arg[n] == '=') { val = arg + n + 1; return true; }
    return false;
}

int main(int argc, char **argv) {
    using clk = std::chrono::steady_clock;
    std::string file1, file2, output, alga_exe, gfa, unitigs, consensus, contigs, contigs_gfa, contigs_final, v;
    alga_host::IngestParams ip;
    double error_rate = 0.0;
    int device = 0, serialize = 1, gpus = 1, clip_tips = 0, parallel_paths = 0, consensus_min_length = 200, consensus_min_votes = 3, contigs_min_length = -1, contigs_new_reads_percent = 95, contigs_trim_threshold = 25, paired_extend = 0;
    int correct_reads = 0;
    std::string corrected_reads, placements, polish_changes;
    int contigs_depth = 0, polish = 0;
    std::string scaffolds, scaffold_layout;
    alga_scaffold_params scp;
    alga_scaffold_default_params(&scp);
    int break_misjoins = 0, break_margin = 0;
    bool break_margin_given = false;
    std::string broken, break_cuts;
    alga_break_params brp;
    alga_break_default_params(&brp);
    int grow_ends = 0;
    std::string grown, grow_layout;
    alga_grow_params grp;
    alga_grow_default_params(&grp);
    int merge_ends = 0;
    int gapped = 0, gapped_edits = -1;
    std::string gapped_placements;
    int polish_indels = 0, polish_max_ins = -1;
    std::string ipolished, ipolish_events;
    std::string sam;
    int sam_unplaced = -1;
    std::string merged_path, merge_layout;
    alga_merge_params mgp;
    alga_merge_default_params(&mgp);
    int drop_contained = 0;
    std::string kept_path, contain_layout;
    alga_contain_params ctp;
    alga_contain_default_params(&ctp);
    int stitch = 0;
    std::string stitched_path, stitch_layout;
    alga_stitch_params stp;
    alga_stitch_default_params(&stp);
    alga_correct_params crp;
    alga_correct_default_params(&crp);
    std::vector<int32_t> gpu_list;
    std::vector<std::string> passthrough;
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
        if (opt(a, "--file1", v)) file1 = v;
        else if (opt(a, "--file2", v)) file2 = v;
        else if (opt(a, "--output", v)) output = v;
        else if (opt(a, "--threads", v)) ip.threads = std::max(1, atoi(v.c_str()));
        else if (opt(a, "--error_rate", v) || opt(a, "--error-rate", v) || opt(a, "--er", v)) error_rate = atof(v.c_str());
        else if (opt(a, "--serialize", v)) serialize = atoi(v.c_str());
        else if (opt(a, "--rsoemo", v)) ip.rsoemo = atoi(v.c_str());
        else if (opt(a, "--scale", v)) ip.scale = (float) atof(v.c_str());
        else if (opt(a, "--retl", v) || opt(a, "--read_end_trim_left", v)) ip.trim_left = atoi(v.c_str());
        else if (opt(a, "--retr", v) || opt(a, "--read_end_trim_right", v)) ip.trim_right = atoi(v.c_str());
        else if (opt(a, "--remove_reads_with_n", v)) ip.remove_reads_with_n = atoi(v.c_str());
        else if (opt(a, "--rna", v)) ip.rna = atoi(v.c_str());
        else if (opt(a, "--device", v)) device = atoi(v.c_str());
        else if (opt(a, "--gpus", v)) gpus = std::max(1, atoi(v.c_str()));
        else if (opt(a, "--gpu-list", v)) { gpu_list.clear(); for (size_t k = 0; k < v.size();) { gpu_list.push_back(atoi(v.c_str() + k)); size_t c = v.find(',', k); if (c == std::string::npos) break; k = c + 1; } }
        else if (opt(a, "--alga", v)) alga_exe = v;
        else if (opt(a, "--gfa", v)) gfa = v;
        else if (opt(a, "--unitigs", v)) unitigs = v;
        else if (opt(a, "--clip_tips", v)) clip_tips = atoi(v.c_str());
        else if (opt(a, "--parallel_paths", v)) parallel_paths = atoi(v.c_str());
        else if (opt(a, "--consensus", v)) consensus = v;
        else if (opt(a, "--contigs", v)) contigs = v;
        else if (opt(a, "--contigs_gfa", v)) contigs_gfa = v;
        else if (opt(a, "--contigs_min_length", v)) contigs_min_length = atoi(v.c_str());
        else if (opt(a, "--contigs_final", v)) contigs_final = v;
        else if (opt(a, "--contigs_depth", v)) contigs_depth = atoi(v.c_str());
        else if (opt(a, "--placements", v)) placements = v;
        else if (opt(a, "--polish", v)) polish = atoi(v.c_str());
        else if (opt(a, "--polish_changes", v)) polish_changes = v;
        else if (opt(a, "--scaffolds", v)) scaffolds = v;
        else if (opt(a, "--scaffold_layout", v)) scaffold_layout = v;
        else if (opt(a, "--scaffold_min_links", v)) scp.min_links = atoi(v.c_str());
        else if (opt(a, "--scaffold_min_gap", v)) scp.min_gap = atoi(v.c_str());
        else if (opt(a, "--scaffold_max_second_percent", v)) scp.max_second_percent = atoi(v.c_str());
        else if (opt(a, "--break_misjoins", v)) break_misjoins = atoi(v.c_str());
        else if (opt(a, "--break_min_span", v)) brp.min_span = atoi(v.c_str());
        else if (opt(a, "--break_inset", v)) brp.inset = atoi(v.c_str());
        else if (opt(a, "--break_margin", v)) { break_margin = atoi(v.c_str()); break_margin_given = true; }
        else if (opt(a, "--broken", v)) broken = v;
        else if (opt(a, "--break_cuts", v)) break_cuts = v;
        else if (opt(a, "--grow_ends", v)) grow_ends = atoi(v.c_str());
        else if (opt(a, "--grown", v)) grown = v;
        else if (opt(a, "--grow_layout", v)) grow_layout = v;
        else if (opt(a, "--grow_min_anchor", v)) grp.min_anchor = atoi(v.c_str());
        else if (opt(a, "--grow_max_mismatches", v)) grp.max_mismatches = atoi(v.c_str());
        else if (opt(a, "--grow_min_cover", v)) grp.min_cover = atoi(v.c_str());
        else if (opt(a, "--grow_min_percent", v)) grp.min_percent = atoi(v.c_str());
        else if (opt(a, "--grow_max", v)) grp.max_grow = atoi(v.c_str());
        else if (opt(a, "--merge_ends", v)) merge_ends = atoi(v.c_str());
        else if (opt(a, "--gapped_placements", v)) gapped_placements = v;
        else if (opt(a, "--gapped_edits", v)) gapped_edits = atoi(v.c_str());
        else if (opt(a, "--gapped", v)) gapped = atoi(v.c_str());
        else if (opt(a, "--polish_indels", v)) polish_indels = atoi(v.c_str());
        else if (opt(a, "--polish_max_ins", v)) polish_max_ins = atoi(v.c_str());
        else if (opt(a, "--ipolished", v)) ipolished = v;
        else if (opt(a, "--ipolish_events", v)) ipolish_events = v;
        else if (opt(a, "--sam_unplaced", v)) sam_unplaced = atoi(v.c_str());
        else if (opt(a, "--sam", v)) sam = v;
        else if (opt(a, "--merged", v)) merged_path = v;
        else if (opt(a, "--drop_contained", v)) drop_contained = atoi(v.c_str());
        else if (opt(a, "--kept", v)) kept_path = v;
        else if (opt(a, "--contain_layout", v)) contain_layout = v;
        else if (opt(a, "--contain_max_permille", v)) ctp.max_permille = atoi(v.c_str());
        else if (opt(a, "--merge_layout", v)) merge_layout = v;
        else if (opt(a, "--merge_min_overlap", v)) mgp.min_overlap = atoi(v.c_str());
        else if (opt(a, "--merge_max_mismatches", v)) mgp.max_mismatches = atoi(v.c_str());
        else if (opt(a, "--stitch", v)) stitch = atoi(v.c_str());
        else if (opt(a, "--stitched", v)) stitched_path = v;
        else if (opt(a, "--stitch_layout", v)) stitch_layout = v;
        else if (opt(a, "--stitch_min_overlap", v)) stp.min_overlap = atoi(v.c_str());
        else if (opt(a, "--stitch_max_mismatches", v)) stp.max_mismatches = atoi(v.c_str());
        else if (opt(a, "--stitch_slack", v)) stp.slack = atoi(v.c_str());
        else if (opt(a, "--contigs_new_reads_percent", v)) contigs_new_reads_percent = atoi(v.c_str());
        else if (opt(a, "--contigs_trim_threshold", v)) contigs_trim_threshold = atoi(v.c_str());
        else if (opt(a, "--paired_extend", v)) paired_extend = atoi(v.c_str());
        else if (opt(a, "--consensus_min_length", v)) consensus_min_length = atoi(v.c_str());
        else if (opt(a, "--consensus_min_votes", v)) consensus_min_votes = atoi(v.c_str());
        else if (opt(a, "--correct_reads", v)) correct_reads = atoi(v.c_str());
        else if (opt(a, "--correct_k", v)) crp.k = atoi(v.c_str());
        else if (opt(a, "--correct_solid", v)) crp.solid_min = atoi(v.c_str());
        else if (opt(a, "--corrected_reads", v)) corrected_reads = v;
        else if (!strcmp(a, "--help") || !strcmp(a, "-h")) { fprintf(stderr, "%s", USAGE); return 2; }
        else if (!strcmp(a, "-l") && i + 1 < argc) ip.min_overlap = atoi(argv[++i]);
        else { fprintf(stderr, "alga_hip: unrecognized option '%s'\n", a); return 2; }
        // the hand-off to stock ALGA drops the error-rate option: the supplement it switches on (src/Params.cpp:357-359) has
        // already run here and nothing downstream reads the rate
        // ... and --serialize / --deserialize_graph: the hand-off always goes through the dump this program writes
        const bool is_er = !strncmp(a, "--error_rate", 12) || !strncmp(a, "--error-rate", 12) || !strncmp(a, "--er=", 5);
        const bool is_ser = !strncmp(a, "--serialize", 11) || !strncmp(a, "--deserialize_graph", 19);
        if (strncmp(a, "--device", 8) && strncmp(a, "--alga", 6) && strncmp(a, "--gpus", 6) && strncmp(a, "--gpu-list", 10) && strncmp(a, "--gfa=", 6) && strncmp(a, "--unitigs=", 10) && strncmp(a, "--clip_tips=", 12) && strncmp(a, "--parallel_paths=", 17) && strncmp(a, "--consensus", 11) && strncmp(a, "--contigs", 9) && strncmp(a, "--paired_extend=", 16) && strncmp(a, "--correct", 9) && strncmp(a, "--placements=", 13) && strncmp(a, "--polish", 8) && strncmp(a, "--scaffold", 10) && strncmp(a, "--break_", 8) && strncmp(a, "--broken=", 9) && strncmp(a, "--grow", 6) && strncmp(a, "--sam", 5) && !is_er && !is_ser) { passthrough.push_back(a); if (!strcmp(a, "-l")) passthrough.push_back(argv[i]); }
    }
    if (file1.empty()) { fprintf(stderr, "\nERROR - PLEASE PROVIDE THE INPUT FILE using --file1 option!\n"); return 1; }
    if (output.empty()) { fprintf(stderr, "\nERROR - PLEASE PROVIDE THE OUTPUT FILE NAME!\n"); return 1; }
    if (crp.k < 5 || crp.k > 31 || !(crp.k & 1)) { fprintf(stderr, "alga_hip: --correct_k must be odd and in [5, 31] (got %d)\n", crp.k); return 2; }
    if (crp.solid_min < 1) { fprintf(stderr, "alga_hip: --correct_solid must be >= 1 (got %d)\n", crp.solid_min); return 2; }
    if (!correct_reads && !corrected_reads.empty()) { fprintf(stderr, "alga_hip: --corrected_reads= needs --correct_reads=1\n"); return 2; }
    if ((contigs_depth || !placements.empty()) && contigs_final.empty()) { fprintf(stderr, "alga_hip: --contigs_depth=1 and --placements= need --contigs_final=\n"); return 2; }
    if (polish && contigs_final.empty()) { fprintf(stderr, "alga_hip: --polish=1 needs --contigs_final=\n"); return 2; }
    if (!polish && !polish_changes.empty()) { fprintf(stderr, "alga_hip: --polish_changes= needs --polish=1\n"); return 2; }
    if (!scaffolds.empty() && (contigs_final.empty() || file2.empty())) { fprintf(stderr, "alga_hip: --scaffolds= needs --contigs_final= and --file2=\n"); return 2; }
    if (scaffolds.empty() && !scaffold_layout.empty()) { fprintf(stderr, "alga_hip: --scaffold_layout= needs --scaffolds=\n"); return 2; }
    if (scp.min_links < 1 || scp.min_gap < 1 || scp.min_gap > (1 << 20) || scp.max_second_percent < 1 || scp.max_second_percent > 100) {
        fprintf(stderr, "alga_hip: --scaffold_min_links must be >= 1, --scaffold_min_gap in [1, 2^20], --scaffold_max_second_percent in [1, 100]\n");
        return 2;
    }
    if (break_misjoins && (contigs_final.empty() || file2.empty())) { fprintf(stderr, "alga_hip: --break_misjoins=1 needs --contigs_final= and --file2=\n"); return 2; }
    if (!break_misjoins && (!broken.empty() || !break_cuts.empty())) { fprintf(stderr, "alga_hip: --broken= and --break_cuts= need --break_misjoins=1\n"); return 2; }
    if (brp.min_span < 1 || brp.inset < 0 || brp.inset > (1 << 20) || break_margin < 0 || break_margin > (1 << 20)) {
        fprintf(stderr, "alga_hip: --break_min_span must be >= 1, --break_inset and --break_margin in [0, 2^20]\n");
        return 2;
    }
    if (grow_ends < 0 || grow_ends > 16) { fprintf(stderr, "alga_hip: --grow_ends must be in [0, 16] (got %d)\n", grow_ends); return 2; }
    if (grow_ends && contigs_final.empty()) { fprintf(stderr, "alga_hip: --grow_ends= needs --contigs_final=\n"); return 2; }
    if (!grow_ends && (!grown.empty() || !grow_layout.empty())) { fprintf(stderr, "alga_hip: --grown= and --grow_layout= need --grow_ends >= 1\n"); return 2; }
    if (grp.min_anchor < grp.k || grp.min_anchor > (1 << 20) || grp.max_mismatches < 0 || grp.max_mismatches > 254 || grp.min_cover < 1 || grp.min_percent < 51 ||
        grp.min_percent > 100 || grp.max_grow < 1 || grp.max_grow > 4096) {
        fprintf(stderr, "alga_hip: --grow_min_anchor must be in [21, 2^20], --grow_max_mismatches in [0, 254], --grow_min_cover >= 1, --grow_min_percent in [51, 100], "
                        "--grow_max in [1, 4096]\n");
        return 2;
    }
    if (gapped != 0 && gapped != 1) { fprintf(stderr, "alga_hip: --gapped must be 0 or 1 (got %d)\n", gapped); return 2; }
    if (gapped && contigs_final.empty()) { fprintf(stderr, "alga_hip: --gapped=1 needs --contigs_final=\n"); return 2; }
    if (!gapped && (!gapped_placements.empty() || gapped_edits != -1)) { fprintf(stderr, "alga_hip: --gapped_placements= and --gapped_edits= need --gapped=1\n"); return 2; }
    if (gapped && gapped_edits != -1 && (gapped_edits < 1 || gapped_edits > 15)) { fprintf(stderr, "alga_hip: --gapped_edits must be in [1, 15] (got %d)\n", gapped_edits); return 2; }
    if (polish_indels != 0 && polish_indels != 1) { fprintf(stderr, "alga_hip: --polish_indels must be 0 or 1 (got %d)\n", polish_indels); return 2; }
    if (polish_indels && !gapped) { fprintf(stderr, "alga_hip: --polish_indels=1 needs --gapped=1\n"); return 2; }
    if (!polish_indels && (!ipolished.empty() || !ipolish_events.empty() || polish_max_ins != -1)) {
        fprintf(stderr, "alga_hip: --ipolished=, --ipolish_events= and --polish_max_ins= need --polish_indels=1\n"); return 2;
    }
    if (polish_indels && polish_max_ins != -1 && (polish_max_ins < 1 || polish_max_ins > ALGA_IPOLISH_MAX_INS)) {
        fprintf(stderr, "alga_hip: --polish_max_ins must be in [1, 13] (got %d)\n", polish_max_ins); return 2;
    }
    if (!sam.empty() && contigs_final.empty()) { fprintf(stderr, "alga_hip: --sam= needs --contigs_final=\n"); return 2; }
    if (sam.empty() && sam_unplaced != -1) { fprintf(stderr, "alga_hip: --sam_unplaced= needs --sam=\n"); return 2; }
    if (!sam.empty() && sam_unplaced != -1 && sam_unplaced != 0 && sam_unplaced != 1) { fprintf(stderr, "alga_hip: --sam_unplaced must be 0 or 1 (got %d)\n", sam_unplaced); return 2; }
    if (!sam.empty() && polish) { fprintf(stderr, "alga_hip: --sam= must be used without --polish=1 (its NM and names describe the unpolished contigs)\n"); return 2; }
    if (merge_ends != 0 && merge_ends != 1) { fprintf(stderr, "alga_hip: --merge_ends must be 0 or 1 (got %d)\n", merge_ends); return 2; }
    if (merge_ends && !grow_ends) { fprintf(stderr, "alga_hip: --merge_ends=1 needs --grow_ends >= 1\n"); return 2; }
    if (!merge_ends && (!merged_path.empty() || !merge_layout.empty())) { fprintf(stderr, "alga_hip: --merged= and --merge_layout= need --merge_ends=1\n"); return 2; }
    if (drop_contained != 0 && drop_contained != 1) { fprintf(stderr, "alga_hip: --drop_contained must be 0 or 1 (got %d)\n", drop_contained); return 2; }
    if (drop_contained && !merge_ends) { fprintf(stderr, "alga_hip: --drop_contained=1 needs --merge_ends=1\n"); return 2; }
    if (!drop_contained && (!kept_path.empty() || !contain_layout.empty())) { fprintf(stderr, "alga_hip: --kept= and --contain_layout= need --drop_contained=1\n"); return 2; }
    if (ctp.max_permille < 0 || ctp.max_permille > 100) { fprintf(stderr, "alga_hip: --contain_max_permille must be in [0, 100]\n"); return 2; }
    if (stitch != 0 && stitch != 1) { fprintf(stderr, "alga_hip: --stitch must be 0 or 1 (got %d)\n", stitch); return 2; }
    if (stitch && scaffolds.empty()) { fprintf(stderr, "alga_hip: --stitch=1 needs --scaffolds=\n"); return 2; }
    if (!stitch && (!stitched_path.empty() || !stitch_layout.empty())) { fprintf(stderr, "alga_hip: --stitched= and --stitch_layout= need --stitch=1\n"); return 2; }
    if (stp.min_overlap < 8 || stp.min_overlap > stp.max_overlap || stp.max_mismatches < 0 || stp.max_mismatches > 254 || stp.slack < 0 || stp.slack > (1 << 20)) {
        fprintf(stderr, "alga_hip: --stitch_min_overlap must be in [8, 512], --stitch_max_mismatches in [0, 254], --stitch_slack in [0, 2^20]\n");
        return 2;
    }
    if (mgp.min_overlap < mgp.k || mgp.min_overlap > mgp.max_overlap || mgp.max_mismatches < 0 || mgp.max_mismatches > 254) {
        fprintf(stderr, "alga_hip: --merge_min_overlap must be in [21, 512], --merge_max_mismatches in [0, 254]\n");
        return 2;
    }
    if (correct_reads && !alga_exe.empty()) {
        fprintf(stderr, "alga_hip: --correct_reads=1 cannot be combined with --alga=: stock ALGA would read the original files, whose nodes are not the corrected graph's\n");
        return 2;
    }
    const std::string graph = alga_host::test_name(file1, ip.scale, ip.remove_reads_with_n) + "_beforeSimplifier.graph";
    if (!alga_exe.empty()) {
        // The hand-off is the dump: it is always written, and a file of that name left behind by an earlier run must not be
        // what stock ALGA loads if this run fails half-way (src/main.cpp:241-242 falls back to its own CPU creator without one).
        serialize = 1;
        (void) unlink(graph.c_str());
    }
    auto t0 = clk::now();
    // Input stages (src/IO/InputReader.cpp, src/IO/ReadPreprocess.cpp, src/main.cpp:93-266) on the GPU: the host maps the files and
    // moves their bytes, the node set stays in HBM for the graph creator.  Inputs that stage does not take (file types other than
    // FASTA / FASTQ, random replacement of N) are parsed on the host cores and join the GPU at the duplicate / prefix removal.
    if (gpu_list.empty()) for (int k = 0; k < gpus; k++) gpu_list.push_back(device + k);
    const int n_ranks = (int) gpu_list.size();
    alga_multi *multi = nullptr;
    alga_engine *engine = nullptr;
    if (n_ranks > 1) {
        bool distinct = true;
        for (int a = 0; a < n_ranks; a++) for (int b = 0; b < a; b++) distinct = distinct && gpu_list[(size_t) a] != gpu_list[(size_t) b];
        int rc = alga_multi_create(gpu_list.data(), n_ranks, distinct ? ALGA_TRANSPORT_AUTO : ALGA_TRANSPORT_COPY, &multi);
        if (rc == ALGA_ERR_UNSUPPORTED) rc = alga_multi_create(gpu_list.data(), n_ranks, ALGA_TRANSPORT_COPY, &multi);     // no RCCL on this box
        if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot open %d HIP devices (status %d)\n", n_ranks, rc); return 1; }
        engine = alga_multi_engine(multi, 0);
    } else if (alga_engine_create(gpu_list[0], &engine) != ALGA_OK) { fprintf(stderr, "alga_amd: no usable HIP device\n"); return 1; }
    const auto t_engine = clk::now();
    alga_device_node_set nodes;
    alga_host::Parsed parsed;
    alga_ingest_params cp;
    alga_ingest_default_params(&cp);
    cp.trim_left = ip.trim_left; cp.trim_right = ip.trim_right; cp.remove_reads_with_n = ip.remove_reads_with_n; cp.rna = ip.rna; cp.scale = ip.scale;
    cp.min_overlap = ip.min_overlap; cp.rsoemo = ip.rsoemo; cp.remove_pref_reads = ip.remove_pref_reads; cp.threads = ip.threads;
    alga_ingest_info info;
    auto t1 = t_engine;
    // the input stage on every GPU of the run, side by side (rank 0's on this thread): the node set never crosses xGMI
    std::vector<alga_device_node_set> rank_nodes((size_t) n_ranks);
    std::vector<alga_ingest_info> rank_info((size_t) n_ranks);
    std::vector<int> rank_rc((size_t) n_ranks, ALGA_OK);
    if (correct_reads) rank_rc.assign((size_t) n_ranks, ALGA_ERR_UNSUPPORTED);       // the host parser, the correction, then the removals on every GPU
    else {
        std::vector<std::thread> th;
        auto ingest = [&](int r) {
            alga_engine *er = multi ? alga_multi_engine(multi, r) : engine;
            rank_rc[(size_t) r] = alga_ingest_device(er, file1.c_str(), file2.empty() ? nullptr : file2.c_str(), &cp, &rank_nodes[(size_t) r], &rank_info[(size_t) r]);
        };
        for (int r = 1; r < n_ranks; r++) th.emplace_back(ingest, r);
        ingest(0);
        for (std::thread &x : th) x.join();
    }
    int irc = ALGA_OK;
    for (int r = 0; r < n_ranks; r++) if (rank_rc[(size_t) r] != ALGA_OK) { irc = rank_rc[(size_t) r]; if (irc != ALGA_ERR_UNSUPPORTED) { fprintf(stderr, "%s\n", alga_last_error(multi ? alga_multi_engine(multi, r) : engine)); return 1; } }
    nodes = rank_nodes[0]; info = rank_info[0];
    if (irc == ALGA_OK) {
        fprintf(stderr, "device ingest: upload %.1f ms, lines + records %.1f ms, duplicate/prefix removal %.1f ms (wall)\n", info.ms_upload,
                info.ms_parse - info.ms_upload, info.ms_preprocess);
        parsed.records = info.records; parsed.removed_n = info.removed_n; parsed.removed_str = info.removed_str;
        parsed.min_overlap = info.min_overlap; parsed.rsoemo = info.rsoemo; parsed.li_kmer_length = info.li_kmer_length; parsed.LEN = info.LEN;
        t1 = t_engine + std::chrono::duration_cast<clk::duration>(std::chrono::duration<double, std::milli>(info.ms_parse));
    } else {                                               // ALGA_ERR_UNSUPPORTED: the host parser, then the duplicate / prefix removal on every GPU
        std::string err = alga_host::parse(file1, file2, ip, parsed);
        if (!err.empty()) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
        t1 = clk::now();
        if (correct_reads) {
            alga_parsed_reads pr{};
            pr.n_nodes = (int64_t) (2 * parsed.R); pr.stride_words = parsed.W; pr.rows = parsed.rows.data(); pr.len = parsed.len.data();
            alga_correct_info ci;
            if (alga_correct_parsed_reads(engine, &pr, &crp, &ci) != ALGA_OK) { fprintf(stderr, "%s\n", alga_last_error(engine)); return 1; }
            fprintf(stderr, "Reads corrected (k %d, solid from %d): %llu reads, %llu k-mers (%llu distinct, %llu solid) in %llu slices; %llu weak runs: %llu fixed, "
                    "%llu ambiguous, %llu without candidate, %llu skipped; %llu reads changed; device ms: count %.3f index %.3f fix %.3f, call %.1f ms wall\n", crp.k,
                    crp.solid_min, (unsigned long long) ci.reads, (unsigned long long) ci.kmers_total, (unsigned long long) ci.kmers_distinct,
                    (unsigned long long) ci.kmers_solid, (unsigned long long) ci.slices, (unsigned long long) ci.runs, (unsigned long long) ci.runs_fixed,
                    (unsigned long long) ci.runs_ambiguous, (unsigned long long) ci.runs_no_candidate, (unsigned long long) ci.runs_skipped,
                    (unsigned long long) ci.reads_changed, ci.ms_count, ci.ms_index, ci.ms_fix, ci.ms_total);
            if (!corrected_reads.empty()) {                // not a hot path: the host writes from the rows that came back
                FILE *f = fopen(corrected_reads.c_str(), "w");
                if (!f) { fprintf(stderr, "alga_hip: cannot write %s\n", corrected_reads.c_str()); return 1; }
                std::string seq;
                for (size_t r = 0; r < parsed.R; r++) {
                    const int32_t l = parsed.len[2 * r + 1];
                    if (l <= 0) continue;
                    const uint32_t *w = parsed.row(2 * r + 1);
                    seq.resize((size_t) l);
                    for (int32_t j = 0; j < l; j++) seq[(size_t) j] = "ACGT"[(w[j >> 4] >> ((j & 15) << 1)) & 3u];
                    fprintf(f, ">read_%zu\n%s\n", r, seq.c_str());
                }
                if (fclose(f) != 0) { fprintf(stderr, "alga_hip: cannot write %s\n", corrected_reads.c_str()); return 1; }
            }
        }
        alga_preprocess_input pin{parsed.rows.data(), parsed.W, parsed.len.data(), (int64_t) (2 * parsed.R), ip.remove_pref_reads, 3 + parsed.li_kmer_length};
        for (int r = 0; r < n_ranks; r++) {
            alga_engine *er = multi ? alga_multi_engine(multi, r) : engine;
            if (alga_preprocess_nodes(er, &pin, &rank_nodes[(size_t) r]) != ALGA_OK) { fprintf(stderr, "%s\n", alga_last_error(er)); return 1; }
        }
        nodes = rank_nodes[0];
    }
    auto t1b = clk::now();
    fprintf(stderr, "input read: %lld records -> %d nodes (removed: %d with N, %d STR, %d duplicate/prefix, %d too short)\n",
            (long long) parsed.records, nodes.n, parsed.removed_n, parsed.removed_str, nodes.removed_prefix, nodes.removed_short);
    fprintf(stderr, "MIN_OVERLAP_PREF_SUF: %d\nREMOVE_SMALL_OVERLAP_EDGES_MIN_OVERLAP: %d\n", parsed.min_overlap, parsed.rsoemo);
    fprintf(stderr, "Creating GraphCreator\n");
    alga_prefsuf_stats st;
    const alga_edge *d_final = nullptr;
    uint64_t n_final = 0;
    alga_host::GraphCreatorPrefSufHIP creator(engine, nodes.d_words, nodes.stride_words, nodes.d_len, nodes.n, parsed.min_overlap, parsed.rsoemo);
    if (multi) {
        std::vector<alga_nodes> per_rank;
        for (int r = 0; r < n_ranks; r++) per_rank.push_back(alga_nodes{rank_nodes[(size_t) r].d_words, rank_nodes[(size_t) r].stride_words, rank_nodes[(size_t) r].d_len, rank_nodes[(size_t) r].n, nullptr, nullptr});
        alga_prefsuf_params pp;
        alga_prefsuf_default_params(&pp);
        pp.min_overlap = parsed.min_overlap; pp.rsoe_min_overlap = parsed.rsoemo;
        int rc = alga_multi_prefsuf_build_device(multi, per_rank.data(), &pp, &d_final, &n_final);
        if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: %s (status %d)\n", alga_multi_last_error(multi), rc); return 1; }
        alga_multi_stats ms;
        std::vector<alga_prefsuf_stats> rs((size_t) n_ranks);
        alga_multi_last_stats(multi, &ms, rs.data());
        st = rs[0];
        fprintf(stderr, "%d GPUs (%s): keys %.1f ms, key all-gather %.1f ms, build %.1f ms, edge gather %.1f ms (rank 0's host clock)%s\n", n_ranks,
                ms.transport == ALGA_TRANSPORT_RCCL ? "RCCL" : "peer copies", ms.ms_keys, ms.ms_share, ms.ms_build, ms.ms_gather,
                ms.fell_back_to_one_gpu ? "; the source-side form does not take this input: rank 0 built the graph alone" : "");
    } else {
        creator.startAlignmentGraphCreation();
        st = creator.stats();
        d_final = creator.deviceEdges();
        n_final = creator.countEdges();
    }
    auto t2 = clk::now();
    if (error_rate > 0.01) {                                                   // src/Params.cpp:358-359, src/main.cpp:300-355
        fprintf(stderr, "Before supplement, G has %llu edges\n", (unsigned long long) n_final);
        std::vector<int32_t> hl((size_t) nodes.n);
        if (nodes.n && alga_copy_to_host(engine, hl.data(), nodes.d_len, hl.size() * sizeof(int32_t)) != ALGA_OK) { fprintf(stderr, "alga_amd: cannot read node lengths back\n"); return 1; }
        double sum = 0; long long cnt = 0;
        for (int32_t l : hl) if (l > 0) { sum += l; cnt++; }
        alga_pkb_params pp;
        alga_pkb_derive_params(cnt ? sum / (double) cnt : 0.0, ip.scale, error_rate, parsed.li_kmer_length, &pp);
        alga_nodes nd{nodes.d_words, nodes.stride_words, nodes.d_len, nodes.n, nullptr, nullptr};
        int rc;
        if (multi) {
            // the k-mer groups dealt out over the GPUs by hash; every rank ends with the same graph, rank 0's comes back
            std::vector<alga_nodes> per_rank;
            for (int r = 0; r < n_ranks; r++) per_rank.push_back(alga_nodes{rank_nodes[(size_t) r].d_words, rank_nodes[(size_t) r].stride_words, rank_nodes[(size_t) r].d_len, rank_nodes[(size_t) r].n, nullptr, nullptr});
            rc = alga_multi_pkb_supplement_device(multi, per_rank.data(), &pp, d_final, n_final, &d_final, &n_final);
            if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: %s (status %d)\n", alga_multi_last_error(multi), rc); return 1; }
        } else {
            rc = alga_pkb_supplement_device(engine, &nd, &pp, d_final, n_final, nullptr, &d_final, &n_final);
            if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: %s (status %d)\n", alga_last_error(engine), rc); return 1; }
        }
        fprintf(stderr, "After supplement G has %llu edges\n", (unsigned long long) n_final);
    }
    if (!gfa.empty()) {                                                        // from the device edges, before they are copied back
        alga_nodes nd{nodes.d_words, nodes.stride_words, nodes.d_len, nodes.n, nullptr, nullptr};
        alga_gfa_info gi;
        int rc = alga_write_gfa_device(engine, &nd, d_final, n_final, gfa.c_str(), ALGA_GFA_TWINS | ALGA_GFA_SEQUENCES, &gi);
        if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot write %s: %s (status %d)\n", gfa.c_str(), alga_last_error(engine), rc); return 1; }
        fprintf(stderr, "GFA written -> %s: %llu segments, %llu links (%llu twin edges merged), %llu bytes; device %.3f ms, wall %.1f ms\n", gfa.c_str(),
                (unsigned long long) gi.segments, (unsigned long long) gi.links, (unsigned long long) gi.links_merged, (unsigned long long) gi.bytes,
                gi.ms_format, gi.ms_total);
    }
    std::vector<alga_edge> final_edges((size_t) n_final);
    if (n_final && alga_copy_to_host(engine, final_edges.data(), d_final, final_edges.size() * sizeof(alga_edge)) != ALGA_OK) { fprintf(stderr, "alga_amd: cannot read the edges back\n"); return 1; }
    fprintf(stderr, "Before first simplifier graph has %llu edges\n", (unsigned long long) n_final);
    const bool want_unitigs = !unitigs.empty() || !consensus.empty();
    if (want_unitigs || !contigs.empty() || !contigs_final.empty()) {                                    // the edges are on the host already: nothing below touches what is handed on
        alga_nodes nd{nodes.d_words, nodes.stride_words, nodes.d_len, nodes.n, nullptr, nullptr};
        const int mopp = std::max(250, (int) (1.75 * parsed.LEN));            // Params::MAX_OFFSET_PARALLEL_PATHS, src/main.cpp:95
        const alga_edge *d_cut = nullptr;
        uint64_t n_cut = 0, n_removed = 0;
        int rc = alga_cut_triangles_device(engine, nodes.n, d_final, n_final, mopp, nullptr, &d_cut, &n_cut, &n_removed);
        // Global::calculateAvgReadLength: the mean length (a double) over the reads that are alive, i.e. have an edge in the graph at hand
        // (Global::removeIsolatedReads).  A host pass over the lengths and the edge list, run only where an option asks for a bound made from it.
        auto live_average = [&](const alga_edge *d_e, uint64_t n_e, double *avg) -> int {
            std::vector<int32_t> hl((size_t) nodes.n);
            std::vector<alga_edge> hc((size_t) n_e);
            int r = ALGA_OK;
            if (nodes.n) r = alga_copy_to_host(engine, hl.data(), nodes.d_len, hl.size() * sizeof(int32_t));
            if (r == ALGA_OK && n_e) r = alga_copy_to_host(engine, hc.data(), d_e, hc.size() * sizeof(alga_edge));
            std::vector<char> has_edge((size_t) nodes.n, 0);
            for (const alga_edge &x : hc) { has_edge[(size_t) x.src] = 1; has_edge[(size_t) x.dst] = 1; }
            double sum = 0; long long cnt = 0;
            for (size_t k = 0; k < hl.size(); k++) if (hl[k] > 0 && has_edge[k]) { sum += hl[k]; cnt++; }
            *avg = cnt ? sum / (double) cnt : 0.0;
            return r;
        };
        alga_unitigs u;
        alga_unitig_info ui;
        alga_gfa_info gi;
        if (rc == ALGA_OK && (clip_tips || parallel_paths)) {
            // Global::calculateAvgReadLength at src/GraphSimplifiers/GraphSimplifier.cpp:179: the mean (a double) over the reads alive after the cut,
            // i.e. without those the cut graph has no edge at (Global::removeIsolatedReads, :117)
            double avg = 0.0;
            rc = live_average(d_cut, n_cut, &avg);
            const int bound = (int) (mopp * avg / (float) 100);                  // MAX_OFFSET_DANGLING_BRANCHES has MAX_OFFSET_PARALLEL_PATHS's value, src/main.cpp:95-96
            if (rc == ALGA_OK && parallel_paths) {
                alga_mst_info mi;
                rc = alga_remove_short_parallel_paths_device(engine, nodes.n, d_cut, n_cut, bound, nullptr, &d_cut, &n_cut, &mi);
                if (rc == ALGA_OK)
                    fprintf(stderr, "Short parallel paths removed: bound %d (average live read length %.3f), %llu edges in, %llu edges out, %llu rounds; %llu of %llu branching nodes "
                            "ran, %llu by the overflow route, largest ball %llu nodes; device ms: prepare %.3f rounds %.3f, call %.1f ms wall\n", bound, avg,
                            (unsigned long long) mi.edges_in, (unsigned long long) mi.edges_out, (unsigned long long) mi.rounds, (unsigned long long) mi.begs_run,
                            (unsigned long long) mi.branching_nodes, (unsigned long long) mi.overflow_begs, (unsigned long long) mi.ball_max, mi.ms_prepare, mi.ms_rounds,
                            mi.ms_total);
            }
            alga_tips_info ti;
            if (rc == ALGA_OK && clip_tips) rc = alga_remove_dangling_branches_device(engine, nodes.n, d_cut, n_cut, bound, nullptr, &d_cut, &n_cut, &ti);
            if (rc == ALGA_OK && clip_tips) {
                fprintf(stderr, "Tips clipped: bound %d (average live read length %.3f), %d iterations, %llu edges removed (", bound, avg, ti.iterations,
                        (unsigned long long) ti.removed_total);
                for (int k = 0; k < ti.passes && k < ALGA_TIPS_MAX_PASSES; k++) fprintf(stderr, "%s%llu", k ? " / " : "", (unsigned long long) ti.removed[k]);
                fprintf(stderr, "), %llu edges left; %llu branching nodes walked, %llu by the overflow route; device ms: prepare %.3f passes %.3f, call %.1f ms wall\n",
                        (unsigned long long) ti.edges_out, (unsigned long long) ti.branching_nodes, (unsigned long long) ti.overflow_nodes, ti.ms_prepare,
                        ti.ms_passes, ti.ms_total);
            }
        }
        if (rc == ALGA_OK && want_unitigs) rc = alga_unitigs_device(engine, &nd, d_cut, n_cut, ALGA_UNITIG_SKIP_ISOLATED, nullptr, &u, &ui);
        std::vector<int32_t> ul;
        if (rc == ALGA_OK && want_unitigs) { ul.resize((size_t) u.n_pairs); if (u.n_pairs) rc = alga_copy_to_host(engine, ul.data(), u.d_len, ul.size() * sizeof(int32_t)); }
        if (rc == ALGA_OK && !unitigs.empty()) rc = alga_write_unitig_gfa_device(engine, &u, unitigs.c_str(), ALGA_GFA_SEQUENCES, &gi);
        if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot write %s: %s (status %d)\n", (unitigs.empty() ? consensus : unitigs).c_str(), alga_last_error(engine), rc); return 1; }
        if (!consensus.empty()) {
            alga_consensus cs;
            alga_consensus_info ci;
            alga_gfa_info fi;
            rc = alga_unitig_consensus_device(engine, &nd, &u, consensus_min_votes, 0, nullptr, &cs, &ci);
            if (rc == ALGA_OK) rc = alga_write_consensus_fasta_device(engine, &u, &cs, consensus.c_str(), consensus_min_length, &fi);
            if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot write %s: %s (status %d)\n", consensus.c_str(), alga_last_error(engine), rc); return 1; }
            fprintf(stderr, "Consensus written -> %s: %llu records of %llu unitigs (%llu with a window), %llu of %llu columns kept, %llu columns differ from the spelled "
                    "sequences, depth up to %llu (%llu words by the wide route); device ms: vote %.3f window %.3f, call %.1f ms wall; FASTA %llu bytes, device %.3f ms, "
                    "wall %.1f ms\n", consensus.c_str(), (unsigned long long) fi.segments, (unsigned long long) ci.pairs, (unsigned long long) ci.pairs_kept,
                    (unsigned long long) ci.trimmed_bases, (unsigned long long) ci.columns, (unsigned long long) ci.changed, (unsigned long long) ci.max_depth,
                    (unsigned long long) ci.wide_words, ci.ms_vote, ci.ms_window, ci.ms_total, (unsigned long long) fi.bytes, fi.ms_format, fi.ms_total);
        }
        if (!unitigs.empty()) {
        std::sort(ul.begin(), ul.end(), [](int32_t a, int32_t b) { return a > b; });
        long long n50 = 0; uint64_t acc = 0;
        for (int32_t l : ul) { acc += (uint64_t) l; if (2 * acc >= ui.total_bases) { n50 = l; break; } }
        fprintf(stderr, "Unitigs written -> %s: %d segments, %llu links, longest %llu nt (%llu reads), N50 %lld, %llu bases; %llu triangle edges cut, %llu isolated reads left out; "
                "device ms: edges %.3f ranking %.3f (%d rounds) layout %.3f sequences %.3f unitig edges %.3f, call %.1f ms wall; GFA %llu bytes, device %.3f ms, wall %.1f ms\n",
                unitigs.c_str(), u.n_pairs, (unsigned long long) gi.links, (unsigned long long) ui.longest_bases, (unsigned long long) ui.longest_nodes, n50,
                (unsigned long long) ui.total_bases, (unsigned long long) n_removed, (unsigned long long) ui.isolated_skipped, ui.ms_sym, ui.ms_rank, ui.rank_rounds,
                ui.ms_layout, ui.ms_seq, ui.ms_edges, ui.ms_total, (unsigned long long) gi.bytes, gi.ms_format, gi.ms_total);
        }
        if (!contigs.empty() || !contigs_final.empty()) {                     // last: the contig result replaces the unitigs on the engine; d_cut stays valid
            alga_unitigs cu;
            alga_contig_info ki;
            alga_consensus cs;
            alga_consensus_info ci;
            alga_gfa_info fi, cgi;
            const int min_len = contigs_min_length >= 0 ? contigs_min_length : std::max(200, (int) (1.75 * parsed.LEN));   // src/main.cpp:94
            rc = alga_contigs_device(engine, &nd, d_cut, n_cut, mopp, 0, nullptr, &cu, &ki);
            if (rc == ALGA_OK && paired_extend && file2.empty()) fprintf(stderr, "--paired_extend=1 without --file2: there are no pairs, the contigs stay as they are\n");
            if (rc == ALGA_OK && paired_extend && !file2.empty()) {
                // Global::calculateAvgReadLength at ContigCreatorSinglePath.cpp:274: the mean over the reads that are alive, i.e. have an edge left
                // d_cut is what the contigs were made from (after the parallel paths and the clip where they ran): the reads alive in it are the
                // reference's at this call, its second one -- the first, for the clip's bound, sees the graph right after the cut
                double avg = 0.0;
                rc = live_average(d_cut, n_cut, &avg);
                const int min_chain_weight = (int) (2 * avg);
                alga_unitigs xu;
                alga_extend_info xi;
                if (rc == ALGA_OK) rc = alga_extend_contigs_device(engine, &nd, nodes.d_pair_off, &cu, min_chain_weight, 5, 1000, 0, nullptr, &xu, &xi);
                if (rc == ALGA_OK) {
                    cu = xu;
                    fprintf(stderr, "Contigs extended by paired connections: %llu -> %llu contigs (min chain weight %d); %llu candidates, %llu direct links, %llu links, "
                            "%llu joinable, %llu ambiguous, %llu cycles cut, largest head %llu entries (%llu passes), longest %llu nt (%llu reads); device ms: count %.3f "
                            "paths %.3f layout %.3f sequences %.3f graph %.3f, call %.1f ms wall\n", (unsigned long long) xi.pairs_in, (unsigned long long) xi.pairs_out,
                            min_chain_weight, (unsigned long long) xi.candidates, (unsigned long long) xi.direct_links, (unsigned long long) xi.links,
                            (unsigned long long) xi.joinable, (unsigned long long) xi.ambiguous, (unsigned long long) xi.cycles_cut, (unsigned long long) xi.head_max,
                            (unsigned long long) xi.head_passes, (unsigned long long) xi.longest_bases, (unsigned long long) xi.longest_nodes, xi.ms_count, xi.ms_paths,
                            xi.ms_layout, xi.ms_seq, xi.ms_edges, xi.ms_total);
                }
            }
            if (rc == ALGA_OK && !contigs_gfa.empty()) rc = alga_write_unitig_gfa_device(engine, &cu, contigs_gfa.c_str(), ALGA_GFA_SEQUENCES, &cgi);
            if (rc == ALGA_OK) rc = alga_unitig_consensus_device(engine, &nd, &cu, consensus_min_votes, 0, nullptr, &cs, &ci);
            if (rc == ALGA_OK && !contigs.empty()) rc = alga_write_consensus_fasta_device(engine, &cu, &cs, contigs.c_str(), min_len, &fi);
            if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot write %s: %s (status %d)\n", (contigs.empty() ? contigs_final : contigs).c_str(), alga_last_error(engine), rc); return 1; }
            if (!contigs.empty())
            fprintf(stderr, "Contigs written -> %s: %llu records of %d contigs (min length %d), longest %llu nt (%llu reads); %llu rounds, %llu -> %llu edges, %llu reads "
                    "dropped, %llu path nodes, %llu junction nodes; device ms: edges %.3f rounds %.3f layout %.3f sequences %.3f contig graph %.3f, call %.1f ms "
                    "wall; consensus %.1f ms wall; FASTA %llu bytes, wall %.1f ms\n", contigs.c_str(), (unsigned long long) fi.segments, cu.n_pairs, min_len,
                    (unsigned long long) ki.longest_bases, (unsigned long long) ki.longest_nodes, (unsigned long long) ki.rounds, (unsigned long long) ki.edges_sym,
                    (unsigned long long) ki.final_edges, (unsigned long long) ki.reads_dropped, (unsigned long long) ki.path_nodes, (unsigned long long) ki.junction_nodes,
                    ki.ms_sym, ki.ms_rounds, ki.ms_layout, ki.ms_seq, ki.ms_edges, ki.ms_total, ci.ms_total, (unsigned long long) fi.bytes, fi.ms_total);
            if (!contigs_gfa.empty())
                fprintf(stderr, "Contig graph written -> %s: %llu segments, %llu links, %llu bytes\n", contigs_gfa.c_str(), (unsigned long long) cgi.segments,
                        (unsigned long long) cgi.links, (unsigned long long) cgi.bytes);
            if (!contigs_final.empty()) {
                alga_final_contigs fc;
                alga_final_info fci;
                alga_gfa_info ffi;
                rc = alga_final_contigs_device(engine, &cu, &cs, min_len, contigs_new_reads_percent, contigs_trim_threshold, 0, nullptr, &fc, &fci);
                if (rc == ALGA_OK && (contigs_depth || !placements.empty() || polish || !scaffolds.empty() || break_misjoins || grow_ends || gapped || !sam.empty())) {
                    // every input read, as the files give it (corrected where the graph's reads were), laid over the final contigs
                    alga_parsed_reads pr{};
                    char perr[512] = {0};
                    if (alga_parse_files(file1.c_str(), file2.empty() ? nullptr : file2.c_str(), &cp, &pr, perr, sizeof(perr)) != ALGA_OK) { fprintf(stderr, "%s\n", perr); return 1; }
                    if (correct_reads && alga_correct_parsed_reads(engine, &pr, &crp, nullptr) != ALGA_OK) { fprintf(stderr, "%s\n", alga_last_error(engine)); return 1; }
                    const size_t pn = (size_t) pr.n_nodes, row_bytes = pn * (size_t) pr.stride_words * sizeof(uint32_t);
                    std::vector<uint8_t> po(pn, 0);
                    if (pr.paired) for (size_t q = 0; q + 3 < pn; q += 4) { po[q] = po[q + 1] = 1; po[q + 2] = po[q + 3] = 2; }
                    void *d_rows = nullptr, *d_plen = nullptr, *d_po = nullptr;
                    rc = alga_device_alloc(engine, row_bytes + 16, &d_rows);
                    if (rc == ALGA_OK) rc = alga_device_alloc(engine, pn * sizeof(int32_t) + 16, &d_plen);
                    if (rc == ALGA_OK) rc = alga_device_alloc(engine, pn + 16, &d_po);
                    if (rc == ALGA_OK && pn) rc = alga_copy_to_device(engine, d_rows, pr.rows, row_bytes);
                    if (rc == ALGA_OK && pn) rc = alga_copy_to_device(engine, d_plen, pr.len, pn * sizeof(int32_t));
                    if (rc == ALGA_OK && pn) rc = alga_copy_to_device(engine, d_po, po.data(), pn);
                    const alga_nodes pnd{(const uint32_t *) d_rows, pr.stride_words, (const int32_t *) d_plen, (int32_t) pn, nullptr, nullptr};
                    alga_place_params pp;
                    alga_place_default_params(&pp);
                    alga_placements pl;
                    alga_place_info pi;
                    if (rc == ALGA_OK) rc = alga_place_reads_on_final_device(engine, &pnd, pr.paired ? (const uint8_t *) d_po : nullptr, &cu, &cs, &fc, &pp, nullptr, &pl, &pi);
                    if (rc == ALGA_OK)
                        fprintf(stderr, "Reads placed on the final contigs: %llu reads, %llu placed (%llu unique, %llu multi), %llu unplaced; %llu proper pairs of %llu, "
                                "median insert %lld; device ms: index %.3f place %.3f depth %.3f, call %.1f ms wall\n", (unsigned long long) pi.reads,
                                (unsigned long long) pi.placed, (unsigned long long) pi.unique, (unsigned long long) pi.multi, (unsigned long long) pi.unplaced,
                                (unsigned long long) pi.pairs_proper, (unsigned long long) pi.pairs, (long long) pi.insert_median, pi.ms_index, pi.ms_place, pi.ms_depth,
                                pi.ms_total);
                    if (rc == ALGA_OK && !placements.empty()) {            // not a hot path: the host formats from the arrays that came back
                        const size_t nr = (size_t) pl.n_reads;
                        std::vector<int32_t> tg(nr), ps(nr);
                        std::vector<uint8_t> mm(nr), hits(nr), state(nr);
                        if (nr) {
                            rc = alga_copy_to_host(engine, tg.data(), pl.d_target, nr * sizeof(int32_t));
                            if (rc == ALGA_OK) rc = alga_copy_to_host(engine, ps.data(), pl.d_pos, nr * sizeof(int32_t));
                            if (rc == ALGA_OK) rc = alga_copy_to_host(engine, mm.data(), pl.d_mm, nr);
                            if (rc == ALGA_OK) rc = alga_copy_to_host(engine, hits.data(), pl.d_hits, nr);
                            if (rc == ALGA_OK) rc = alga_copy_to_host(engine, state.data(), pl.d_state, nr);
                        }
                        FILE *f = rc == ALGA_OK ? fopen(placements.c_str(), "w") : nullptr;
                        if (rc == ALGA_OK && !f) { fprintf(stderr, "alga_hip: cannot write %s\n", placements.c_str()); return 1; }
                        for (size_t r = 0; f && r < nr; r++)
                            fprintf(f, "%zu\t%d\t%d\t%c\t%d\t%d\n", r, tg[r], ps[r], !(state[r] & ALGA_PLACE_PLACED) ? '.' : (state[r] & ALGA_PLACE_MINUS) ? '-' : '+',
                                    (int) mm[r], (int) hits[r]);
                        if (f && fclose(f) != 0) { fprintf(stderr, "alga_hip: cannot write %s\n", placements.c_str()); return 1; }
                    }
                    // --sam=: the pairs judged over the passes at hand, every read as a record
                    auto write_sam = [&](const alga_gapped *gpp) -> int {
                        alga_pair_params jq;
                        alga_pair_default_params(&jq);
                        jq.max_insert = pp.max_insert;
                        alga_pair_calls jc;
                        alga_pair_info ji;
                        int r = alga_judge_pairs_device(engine, &pnd, pr.paired ? (const uint8_t *) d_po : nullptr, &pl, gpp, &jq, nullptr, &jc, &ji);
                        if (r != ALGA_OK) return r;
                        alga_sam_params sq{};
                        sq.flags = (contigs_depth ? ALGA_SAM_NAMES_DEPTH : 0) | (sam_unplaced == 0 ? ALGA_SAM_SKIP_UNPLACED : 0);
                        alga_gfa_info si;
                        r = alga_write_sam_device(engine, &pnd, &pl, gpp, &jc, &sq, sam.c_str(), &si);
                        if (r != ALGA_OK) return r;
                        fprintf(stderr, "SAM written: %llu records; %llu pairs: %llu proper, %llu improper, %llu split, %llu not unique; with a gapped mate %llu pairs, %llu proper; "
                                "median insert %lld; device ms: judge %.3f format %.3f, %llu bytes\n", (unsigned long long) si.segments, (unsigned long long) ji.pairs,
                                (unsigned long long) ji.pairs_proper, (unsigned long long) ji.pairs_improper, (unsigned long long) ji.pairs_split,
                                (unsigned long long) ji.pairs_not_unique, (unsigned long long) ji.pairs_with_gapped, (unsigned long long) ji.proper_with_gapped,
                                (long long) ji.insert_median, ji.ms_judge, si.ms_format, (unsigned long long) si.bytes);
                        return ALGA_OK;
                    };
                    if (rc == ALGA_OK && !gapped && !sam.empty()) rc = write_sam(nullptr);
                    if (rc == ALGA_OK && gapped) {
                        // the targets of that placement once more, as arrays: target j = the window of the pair order[j] (not a hot path: made on the host)
                        const size_t np = (size_t) fc.n_pairs, nt = (size_t) fc.n_accepted;
                        std::vector<uint64_t> woff(np + 1), tb(nt + 1);
                        std::vector<uint8_t> verdict(np + 1);
                        std::vector<int32_t> order(nt + 1), fb(np + 1), fl(np + 1), tl(nt + 1);
                        rc = alga_copy_to_host(engine, woff.data(), cu.d_word_off, (np + 1) * sizeof(uint64_t));
                        if (rc == ALGA_OK && np) rc = alga_copy_to_host(engine, verdict.data(), fc.d_verdict, np);
                        if (rc == ALGA_OK && np) rc = alga_copy_to_host(engine, fb.data(), fc.d_begin, np * sizeof(int32_t));
                        if (rc == ALGA_OK && np) rc = alga_copy_to_host(engine, fl.data(), fc.d_len, np * sizeof(int32_t));
                        if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, order.data(), fc.d_order, nt * sizeof(int32_t));
                        for (size_t j = 0; rc == ALGA_OK && j < nt; j++) {
                            const size_t q = (size_t) order[j];
                            const bool live = verdict[q] == ALGA_FINAL_ACCEPTED;
                            tb[j] = 16ull * woff[q] + (uint64_t) (live ? fb[q] : 0);
                            tl[j] = live ? fl[q] : 0;
                        }
                        void *d_tb = nullptr, *d_tl = nullptr;
                        if (rc == ALGA_OK) rc = alga_device_alloc(engine, (nt + 1) * sizeof(uint64_t), &d_tb);
                        if (rc == ALGA_OK) rc = alga_device_alloc(engine, (nt + 1) * sizeof(int32_t), &d_tl);
                        if (rc == ALGA_OK && nt) rc = alga_copy_to_device(engine, d_tb, tb.data(), nt * sizeof(uint64_t));
                        if (rc == ALGA_OK && nt) rc = alga_copy_to_device(engine, d_tl, tl.data(), nt * sizeof(int32_t));
                        alga_gapped_params gq;
                        alga_gapped_default_params(&gq);
                        if (gapped_edits != -1) gq.max_edits = gapped_edits;
                        alga_gapped gp;
                        alga_gapped_info gi;
                        if (rc == ALGA_OK) rc = alga_place_gapped_device(engine, &pnd, cs.d_words, (const uint64_t *) d_tb, (const int32_t *) d_tl, (int32_t) nt, &pl, &gq, nullptr, &gp, &gi);
                        if (rc == ALGA_OK)
                            fprintf(stderr, "Unplaced reads laid with indels (up to %d edits): %llu tried, %llu placed, %llu unique, %llu with indel, %llu edits; "
                                    "device ms: index %.3f place %.3f trace %.3f depth %.3f, call %.1f ms wall\n", gq.max_edits, (unsigned long long) gi.tried,
                                    (unsigned long long) gi.placed, (unsigned long long) gi.unique, (unsigned long long) gi.with_indel, (unsigned long long) gi.edits,
                                    gi.ms_index, gi.ms_place, gi.ms_trace, gi.ms_depth, gi.ms_total);
                        alga_gfa_info gti;
                        if (rc == ALGA_OK && !gapped_placements.empty()) rc = alga_write_gapped_tsv_device(engine, &gp, gapped_placements.c_str(), &gti);
                        if (rc == ALGA_OK && !sam.empty()) rc = write_sam(&gp);
                        if (rc == ALGA_OK && polish_indels) {
                            alga_ipolish_params iq;
                            alga_ipolish_default_params(&iq);
                            if (polish_max_ins != -1) iq.max_ins = polish_max_ins;
                            alga_ipolished ipo;
                            alga_ipolish_info ii;
                            rc = alga_polish_indels_device(engine, &pnd, &pl, &gp, &iq, nullptr, &ipo, &ii);
                            if (rc == ALGA_OK)
                                fprintf(stderr, "Final contigs polished with the gapped reads (cover %d, %d %%, insertions up to %d): %llu + %llu voters, %llu substituted, %llu deleted, "
                                        "%llu inserted in %llu slots, %llu + %llu ambiguous, columns %llu -> %llu; device ms: votes %.3f inserts %.3f build %.3f, call %.1f ms wall\n",
                                        iq.min_cover, iq.min_percent, iq.max_ins, (unsigned long long) ii.voters_hamming, (unsigned long long) ii.voters_gapped,
                                        (unsigned long long) ii.substituted, (unsigned long long) ii.deleted, (unsigned long long) ii.inserted_bases,
                                        (unsigned long long) ii.inserted_slots, (unsigned long long) ii.ambiguous_columns, (unsigned long long) ii.ambiguous_slots,
                                        (unsigned long long) ii.columns, (unsigned long long) ii.columns_after, ii.ms_votes, ii.ms_inserts, ii.ms_build, ii.ms_total);
                            alga_gfa_info iti;
                            if (rc == ALGA_OK && !ipolished.empty()) rc = alga_write_ipolished_fasta_device(engine, &ipo, ipolished.c_str(), &iti);
                            if (rc == ALGA_OK && !ipolish_events.empty()) rc = alga_write_ipolish_events_tsv_device(engine, &ipo, ipolish_events.c_str(), &iti);
                        }
                        alga_device_free(engine, d_tb);
                        alga_device_free(engine, d_tl);
                    }
                    alga_polished pol{};
                    if (rc == ALGA_OK && polish) {
                        alga_polish_params qp;
                        alga_polish_default_params(&qp);
                        if (!polish_changes.empty()) qp.flags |= ALGA_POLISH_COUNTS;
                        alga_polish_info qi;
                        rc = alga_polish_placed_device(engine, &pnd, &pl, &qp, nullptr, &pol, &qi);
                        if (rc == ALGA_OK)
                            fprintf(stderr, "Final contigs polished (cover %d, %d %%): %llu voters, %llu voted columns of %llu, %llu changed, %llu ambiguous, cover up to %llu; "
                                    "device ms: sort %.3f vote %.3f, call %.1f ms wall\n", qp.min_cover, qp.min_percent, (unsigned long long) qi.voters,
                                    (unsigned long long) qi.voted_columns, (unsigned long long) qi.columns, (unsigned long long) qi.changed,
                                    (unsigned long long) qi.ambiguous, (unsigned long long) qi.max_cover, qi.ms_sort, qi.ms_vote, qi.ms_total);
                    }
                    if (rc == ALGA_OK && polish && !polish_changes.empty()) {   // not a hot path: the host formats from the arrays that came back
                        const size_t nc = (size_t) pol.n_changed, nt = (size_t) pol.n_targets, ncol = (size_t) pol.n_columns;
                        std::vector<uint32_t> cols(nc), off(nt + 1), counts(4 * ncol);
                        std::vector<uint8_t> bases(nc);
                        rc = alga_copy_to_host(engine, off.data(), pol.d_col_off, (nt + 1) * sizeof(uint32_t));
                        if (rc == ALGA_OK && nc) rc = alga_copy_to_host(engine, cols.data(), pol.d_changed_cols, nc * sizeof(uint32_t));
                        if (rc == ALGA_OK && nc) rc = alga_copy_to_host(engine, bases.data(), pol.d_changed_bases, nc);
                        if (rc == ALGA_OK && ncol) rc = alga_copy_to_host(engine, counts.data(), pol.d_counts, 4 * ncol * sizeof(uint32_t));
                        FILE *f = rc == ALGA_OK ? fopen(polish_changes.c_str(), "w") : nullptr;
                        if (rc == ALGA_OK && !f) { fprintf(stderr, "alga_hip: cannot write %s\n", polish_changes.c_str()); return 1; }
                        for (size_t i = 0; f && i < nc; i++) {
                            const size_t t = (size_t) (std::upper_bound(off.begin(), off.end(), cols[i]) - off.begin()) - 1;
                            const uint32_t *c4 = &counts[4 * (size_t) cols[i]];
                            fprintf(f, "%zu\t%u\t%c\t%c\t%u\t%u\t%u\t%u\n", t, cols[i] - off[t], "ACGT"[bases[i] & 3], "ACGT"[(bases[i] >> 2) & 3], c4[0], c4[1], c4[2], c4[3]);
                        }
                        if (f && fclose(f) != 0) { fprintf(stderr, "alga_hip: cannot write %s\n", polish_changes.c_str()); return 1; }
                    }
                    if (rc == ALGA_OK) rc = polish ? alga_write_polished_fasta_device(engine, &cu, &cs, &fc, &pl, &pol, contigs_depth, contigs_final.c_str(), &ffi)
                                        : contigs_depth ? alga_write_final_fasta_depth_device(engine, &cu, &cs, &fc, &pl, contigs_final.c_str(), &ffi)
                                                        : alga_write_final_fasta_device(engine, &cu, &cs, &fc, contigs_final.c_str(), &ffi);
                    // what the scaffolder works on: the placement on the contigs, or with --break_misjoins=1 a second one on the pieces
                    const alga_placements *spl = &pl;
                    const alga_place_info *spi = &pi;
                    const alga_polished *spol = polish ? &pol : nullptr;
                    alga_placements pl2;
                    alga_place_info pi2;
                    if (rc == ALGA_OK && break_misjoins) {
                        const bool have = pr.paired && pi.insert_median >= 0;
                        if (!have) fprintf(stderr, "Breaking skipped: the placement saw no proper pair, so nothing can span a column; every contig is one piece\n");
                        brp.margin = !have ? 0 : break_margin_given ? break_margin : (int32_t) std::min<long long>(pi.insert_median, 1 << 20);
                        alga_broken bk;
                        alga_break_info bi;
                        rc = alga_break_placed_device(engine, &pnd, have ? (const uint8_t *) d_po : nullptr, &pl, polish ? &pol : nullptr, &brp, nullptr, &bk, &bi);
                        if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot break the contigs: %s (status %d)\n", alga_last_error(engine), rc); return 1; }
                        fprintf(stderr, "Contigs broken: %llu proper pairs (%llu spanning), %llu weak columns, %llu runs (%llu open), %llu cuts, %llu contigs cut, %llu pieces, "
                                "N50 %llu -> %llu; min span %d, inset %d, margin %d, %llu candidate columns, span up to %llu, longest piece %llu; device ms: span %.3f "
                                "cut %.3f, call %.1f ms wall\n", (unsigned long long) bi.pairs_proper, (unsigned long long) bi.pairs_spanning,
                                (unsigned long long) bi.weak_columns, (unsigned long long) bi.runs, (unsigned long long) bi.runs_open, (unsigned long long) bi.cuts,
                                (unsigned long long) bi.targets_cut, (unsigned long long) bi.pieces, (unsigned long long) bi.n50_targets, (unsigned long long) bi.n50_pieces,
                                brp.min_span, brp.inset, brp.margin, (unsigned long long) bi.candidate_columns, (unsigned long long) bi.max_span,
                                (unsigned long long) bi.longest_piece, bi.ms_span, bi.ms_cut, bi.ms_total);
                        if (!broken.empty()) {
                            alga_gfa_info bgi;
                            rc = alga_write_broken_fasta_device(engine, &bk, broken.c_str(), &bgi);
                            if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot write %s: %s (status %d)\n", broken.c_str(), alga_last_error(engine), rc); return 1; }
                            fprintf(stderr, "Pieces written -> %s: %llu records, %llu bytes\n", broken.c_str(), (unsigned long long) bgi.segments, (unsigned long long) bgi.bytes);
                        }
                        if (!break_cuts.empty()) {                           // not a hot path: the host formats from the arrays that came back
                            const size_t nc = (size_t) bk.n_cuts, nt = (size_t) bk.n_targets;
                            std::vector<uint32_t> off(nt + 1), cols(nc), first(nc), last(nc);
                            rc = alga_copy_to_host(engine, off.data(), pl.d_col_off, (nt + 1) * sizeof(uint32_t));
                            if (rc == ALGA_OK && nc) rc = alga_copy_to_host(engine, cols.data(), bk.d_cut_cols, nc * sizeof(uint32_t));
                            if (rc == ALGA_OK && nc) rc = alga_copy_to_host(engine, first.data(), bk.d_cut_first, nc * sizeof(uint32_t));
                            if (rc == ALGA_OK && nc) rc = alga_copy_to_host(engine, last.data(), bk.d_cut_last, nc * sizeof(uint32_t));
                            FILE *f = rc == ALGA_OK ? fopen(break_cuts.c_str(), "w") : nullptr;
                            if (rc == ALGA_OK && !f) { fprintf(stderr, "alga_hip: cannot write %s\n", break_cuts.c_str()); return 1; }
                            for (size_t i = 0; f && i < nc; i++) {
                                const size_t t = (size_t) (std::upper_bound(off.begin(), off.end(), cols[i]) - off.begin()) - 1;
                                fprintf(f, "%zu\t%u\t%u\t%u\n", t, cols[i] - off[t], first[i] - off[t], last[i] - off[t]);
                            }
                            if (f && fclose(f) != 0) { fprintf(stderr, "alga_hip: cannot write %s\n", break_cuts.c_str()); return 1; }
                        }
                        if (rc == ALGA_OK && (!scaffolds.empty() || grow_ends) && have) {    // the same reads on the pieces (the break result keeps its own copy of the bases)
                            rc = alga_place_reads_device(engine, &pnd, (const uint8_t *) d_po, bk.d_words, bk.d_begin, bk.d_len, (int32_t) bk.n_pieces, &pp, nullptr, &pl2, &pi2);
                            if (rc == ALGA_OK) {
                                fprintf(stderr, "Reads placed on the pieces: %llu reads, %llu placed (%llu unique, %llu multi), %llu unplaced; %llu proper pairs of %llu, "
                                        "median insert %lld; call %.1f ms wall\n", (unsigned long long) pi2.reads, (unsigned long long) pi2.placed, (unsigned long long) pi2.unique,
                                        (unsigned long long) pi2.multi, (unsigned long long) pi2.unplaced, (unsigned long long) pi2.pairs_proper, (unsigned long long) pi2.pairs,
                                        (long long) pi2.insert_median, pi2.ms_total);
                                spl = &pl2; spi = &pi2; spol = nullptr;         // (a polish is already in the pieces' bases)
                            }
                        }
                    }
                    alga_placements pl3;
                    alga_place_info pi3;
                    if (rc == ALGA_OK && grow_ends) {
                        alga_grown gw{};
                        for (int round = 1; round <= grow_ends; round++) {
                            alga_grow_info gi;
                            rc = alga_grow_placed_device(engine, &pnd, spl, spol, &grp, nullptr, &gw, &gi);
                            if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot grow the contig ends: %s (status %d)\n", alga_last_error(engine), rc); return 1; }
                            fprintf(stderr, "Contig ends grown, round %d: %llu candidates, %llu voting, %llu ends grown, %llu bases added, N50 %llu -> %llu; %llu overhanging "
                                    "(%llu at several places), %llu ends with voters, stops: %llu cover %llu percent %llu max, longest growth %llu, %llu -> %llu columns; "
                                    "device ms: index %.3f place %.3f build %.3f, call %.1f ms wall\n", round, (unsigned long long) gi.candidates,
                                    (unsigned long long) gi.voting, (unsigned long long) gi.ends_grown, (unsigned long long) gi.bases_added, (unsigned long long) gi.n50_before,
                                    (unsigned long long) gi.n50_after, (unsigned long long) gi.overhanging, (unsigned long long) gi.multi, (unsigned long long) gi.ends_with_voters,
                                    (unsigned long long) gi.stops_cover, (unsigned long long) gi.stops_percent, (unsigned long long) gi.stops_max,
                                    (unsigned long long) gi.longest_growth, (unsigned long long) gi.columns_before, (unsigned long long) gi.columns_after, gi.ms_index, gi.ms_place,
                                    gi.ms_build, gi.ms_total);
                            if (!gi.bases_added) break;                         // the contigs are what the current placement was made on
                            // the same reads on the grown contigs (the grow result keeps its own copy of the bases)
                            rc = alga_place_reads_device(engine, &pnd, pr.paired ? (const uint8_t *) d_po : nullptr, gw.d_words, gw.d_begin, gw.d_len, (int32_t) gw.n_targets, &pp,
                                                         nullptr, &pl3, &pi3);
                            if (rc != ALGA_OK) break;
                            fprintf(stderr, "Reads placed on the grown contigs: %llu reads, %llu placed (%llu unique, %llu multi), %llu unplaced; %llu proper pairs of %llu, "
                                    "median insert %lld; call %.1f ms wall\n", (unsigned long long) pi3.reads, (unsigned long long) pi3.placed, (unsigned long long) pi3.unique,
                                    (unsigned long long) pi3.multi, (unsigned long long) pi3.unplaced, (unsigned long long) pi3.pairs_proper, (unsigned long long) pi3.pairs,
                                    (long long) pi3.insert_median, pi3.ms_total);
                            spl = &pl3; spi = &pi3; spol = nullptr;             // (a polish is already in the grown bases)
                        }
                        if (rc == ALGA_OK && !grown.empty()) {
                            alga_gfa_info ggi;
                            rc = alga_write_grown_fasta_device(engine, &gw, grown.c_str(), &ggi);
                            if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot write %s: %s (status %d)\n", grown.c_str(), alga_last_error(engine), rc); return 1; }
                            fprintf(stderr, "Grown contigs written -> %s: %llu records, %llu bytes\n", grown.c_str(), (unsigned long long) ggi.segments, (unsigned long long) ggi.bytes);
                        }
                        if (rc == ALGA_OK && !grow_layout.empty()) {         // not a hot path: the host formats from the arrays that came back
                            const size_t nt = (size_t) gw.n_targets;
                            std::vector<uint32_t> left(nt), right(nt), voters(2 * nt);
                            std::vector<uint8_t> stop(2 * nt);
                            if (nt) {
                                rc = alga_copy_to_host(engine, left.data(), gw.d_left, nt * sizeof(uint32_t));
                                if (rc == ALGA_OK) rc = alga_copy_to_host(engine, right.data(), gw.d_right, nt * sizeof(uint32_t));
                                if (rc == ALGA_OK) rc = alga_copy_to_host(engine, voters.data(), gw.d_e_voters, 2 * nt * sizeof(uint32_t));
                                if (rc == ALGA_OK) rc = alga_copy_to_host(engine, stop.data(), gw.d_e_stop, 2 * nt);
                            }
                            FILE *f = rc == ALGA_OK ? fopen(grow_layout.c_str(), "w") : nullptr;
                            if (rc == ALGA_OK && !f) { fprintf(stderr, "alga_hip: cannot write %s\n", grow_layout.c_str()); return 1; }
                            for (size_t t = 0; f && t < nt; t++)
                                fprintf(f, "%zu\t%u\t%u\t%u\t%u\t%d\t%d\n", t, left[t], right[t], voters[2 * t], voters[2 * t + 1], (int) stop[2 * t], (int) stop[2 * t + 1]);
                            if (f && fclose(f) != 0) { fprintf(stderr, "alga_hip: cannot write %s\n", grow_layout.c_str()); return 1; }
                        }
                        if (rc == ALGA_OK && merge_ends) {                   // the grown contigs whose ends overlap become one, and the reads are placed on those
                            alga_merged mg{};
                            alga_merge_info mi;
                            rc = alga_merge_targets_device(engine, gw.d_words, gw.d_begin, gw.d_len, (int32_t) gw.n_targets, &mgp, nullptr, &mg, &mi);
                            if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot merge the contig ends: %s (status %d)\n", alga_last_error(engine), rc); return 1; }
                            fprintf(stderr, "Contig ends merged: %llu ends with an overlap, %llu ambiguous, %llu joins, %llu bases removed, N50 %llu -> %llu; %llu ends of "
                                    "%llu contigs, %llu joins dropped for cycles, %llu mismatches in the joins, longest overlap %llu, %llu merged contigs (%llu of several), "
                                    "%llu -> %llu columns; device ms: index %.3f overlap %.3f build %.3f, call %.1f ms wall\n", (unsigned long long) mi.ends_with_overlap,
                                    (unsigned long long) mi.ends_ambiguous, (unsigned long long) mi.joins, (unsigned long long) mi.bases_removed, (unsigned long long) mi.n50_before,
                                    (unsigned long long) mi.n50_after, (unsigned long long) mi.ends, (unsigned long long) mg.n_targets, (unsigned long long) mi.joins_dropped_cycle,
                                    (unsigned long long) mi.join_mismatches, (unsigned long long) mi.longest_overlap, (unsigned long long) mi.merged,
                                    (unsigned long long) mi.merged_multi, (unsigned long long) mi.columns_before, (unsigned long long) mi.columns_after, mi.ms_index, mi.ms_overlap,
                                    mi.ms_build, mi.ms_total);
                            if (!merged_path.empty()) {
                                alga_gfa_info mgi;
                                rc = alga_write_merged_fasta_device(engine, &mg, merged_path.c_str(), &mgi);
                                if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot write %s: %s (status %d)\n", merged_path.c_str(), alga_last_error(engine), rc); return 1; }
                                fprintf(stderr, "Merged contigs written -> %s: %llu records, %llu bytes\n", merged_path.c_str(), (unsigned long long) mgi.segments,
                                        (unsigned long long) mgi.bytes);
                            }
                            if (!merge_layout.empty()) {                     // not a hot path: the host formats from the arrays that came back
                                const size_t nt = (size_t) mg.n_targets, nj = (size_t) mg.n_merged, nm = (size_t) mg.n_members;
                                std::vector<uint32_t> m_off(nj + 1), start(nt);
                                std::vector<int32_t> members(nm), rank(nt), ov(nt), tlen(nt);
                                std::vector<uint8_t> orient(nt), mm(2 * nt);
                                rc = alga_copy_to_host(engine, m_off.data(), mg.d_m_off, (nj + 1) * sizeof(uint32_t));
                                if (rc == ALGA_OK && nm) rc = alga_copy_to_host(engine, members.data(), mg.d_m_members, nm * sizeof(int32_t));
                                if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, rank.data(), mg.d_rank, nt * sizeof(int32_t));
                                if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, ov.data(), mg.d_overlap_after, nt * sizeof(int32_t));
                                if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, tlen.data(), gw.d_len, nt * sizeof(int32_t));
                                if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, start.data(), mg.d_start, nt * sizeof(uint32_t));
                                if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, orient.data(), mg.d_orient, nt);
                                if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, mm.data(), mg.d_mm, 2 * nt);
                                FILE *f = rc == ALGA_OK ? fopen(merge_layout.c_str(), "w") : nullptr;
                                if (rc == ALGA_OK && !f) { fprintf(stderr, "alga_hip: cannot write %s\n", merge_layout.c_str()); return 1; }
                                for (size_t j = 0; f && j < nj; j++)
                                    for (uint32_t k = m_off[j]; k < m_off[j + 1]; k++) {
                                        const size_t c = (size_t) members[k];
                                        fprintf(f, "%zu\t%d\t%zu\t%c\t%u\t%d\t%d\t%d\n", j, rank[c], c, orient[c] ? '-' : '+', start[c], tlen[c], ov[c],
                                                ov[c] ? (int) mm[2 * c + (orient[c] ^ 1)] : 0);
                                    }
                                if (f && fclose(f) != 0) { fprintf(stderr, "alga_hip: cannot write %s\n", merge_layout.c_str()); return 1; }
                            }
                            const uint32_t *t_words = mg.d_words;
                            const uint64_t *t_begin = mg.d_begin;
                            const int32_t *t_len = mg.d_len;
                            int32_t t_n = (int32_t) mg.n_merged;
                            const char *t_what = "merged";
                            alga_kept kp{};
                            if (rc == ALGA_OK && drop_contained) {            // the merged contigs that lie inside a longer one are dropped, and the reads are placed on the kept ones
                                alga_contain_info ci;
                                rc = alga_drop_contained_device(engine, mg.d_words, mg.d_begin, mg.d_len, (int32_t) mg.n_merged, &ctp, nullptr, &kp, &ci);
                                if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot drop the contained contigs: %s (status %d)\n", alga_last_error(engine), rc); return 1; }
                                fprintf(stderr, "Contained contigs dropped: %llu queries, %llu candidates, %llu contained (%llu minus, %llu duplicates), %llu ambiguous, %llu bases "
                                        "removed, N50 %llu -> %llu; %llu kept of %llu contigs, %llu seeds (%llu over max_occ), longest contained %llu, %llu -> %llu columns; device "
                                        "ms: index %.3f contain %.3f build %.3f, call %.1f ms wall\n", (unsigned long long) ci.queries, (unsigned long long) ci.candidates,
                                        (unsigned long long) ci.contained, (unsigned long long) ci.contained_minus, (unsigned long long) ci.duplicates, (unsigned long long) ci.ambiguous,
                                        (unsigned long long) ci.bases_removed, (unsigned long long) ci.n50_before, (unsigned long long) ci.n50_after, (unsigned long long) ci.kept,
                                        (unsigned long long) kp.n_targets, (unsigned long long) ci.seeds, (unsigned long long) ci.seeds_over_max_occ,
                                        (unsigned long long) ci.longest_contained, (unsigned long long) ci.columns_before, (unsigned long long) ci.columns_after, ci.ms_index,
                                        ci.ms_contain, ci.ms_build, ci.ms_total);
                                if (!kept_path.empty()) {
                                    alga_gfa_info kgi;
                                    rc = alga_write_kept_fasta_device(engine, &kp, kept_path.c_str(), &kgi);
                                    if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot write %s: %s (status %d)\n", kept_path.c_str(), alga_last_error(engine), rc); return 1; }
                                    fprintf(stderr, "Kept contigs written -> %s: %llu records, %llu bytes\n", kept_path.c_str(), (unsigned long long) kgi.segments,
                                            (unsigned long long) kgi.bytes);
                                }
                                if (!contain_layout.empty()) {                // not a hot path: the host formats from the arrays that came back
                                    const size_t nt = (size_t) kp.n_targets;
                                    std::vector<int32_t> tlen(nt), nw(nt), host(nt), hpos(nt), root(nt), rpos(nt);
                                    std::vector<uint32_t> mm(nt);
                                    std::vector<uint8_t> state(nt), hor(nt), hits(nt), ror(nt);
                                    const struct { void *dst; const void *src; size_t bytes; } copies[] = {
                                        {tlen.data(), mg.d_len, nt * 4}, {nw.data(), kp.d_new, nt * 4}, {host.data(), kp.d_host, nt * 4}, {hpos.data(), kp.d_host_pos, nt * 4},
                                        {root.data(), kp.d_root, nt * 4}, {rpos.data(), kp.d_root_pos, nt * 4}, {mm.data(), kp.d_mm, nt * 4}, {state.data(), kp.d_state, nt},
                                        {hor.data(), kp.d_host_orient, nt}, {hits.data(), kp.d_hits, nt}, {ror.data(), kp.d_root_orient, nt}};
                                    for (const auto &cp : copies) if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, cp.dst, cp.src, cp.bytes);
                                    FILE *f = rc == ALGA_OK ? fopen(contain_layout.c_str(), "w") : nullptr;
                                    if (rc == ALGA_OK && !f) { fprintf(stderr, "alga_hip: cannot write %s\n", contain_layout.c_str()); return 1; }
                                    for (size_t c = 0; f && c < nt; c++)
                                        fprintf(f, "%zu\t%d\t%d\t%d\t%d\t%d\t%c\t%u\t%d\t%d\t%d\t%c\n", c, tlen[c], (int) state[c], nw[c], host[c], hpos[c], hor[c] ? '-' : '+', mm[c],
                                                (int) hits[c], root[c], rpos[c], ror[c] ? '-' : '+');
                                    if (f && fclose(f) != 0) { fprintf(stderr, "alga_hip: cannot write %s\n", contain_layout.c_str()); return 1; }
                                }
                                t_words = kp.d_words; t_begin = kp.d_begin; t_len = kp.d_len; t_n = (int32_t) kp.n_kept; t_what = "kept";
                            }
                            // the same reads on the merged contigs, or on the kept ones (the result keeps its own copy of the bases)
                            if (rc == ALGA_OK) rc = alga_place_reads_device(engine, &pnd, pr.paired ? (const uint8_t *) d_po : nullptr, t_words, t_begin, t_len, t_n, &pp, nullptr,
                                                                            &pl3, &pi3);
                            if (rc == ALGA_OK) {
                                fprintf(stderr, "Reads placed on the %s contigs: %llu reads, %llu placed (%llu unique, %llu multi), %llu unplaced; %llu proper pairs of %llu, "
                                        "median insert %lld; call %.1f ms wall\n", t_what, (unsigned long long) pi3.reads, (unsigned long long) pi3.placed, (unsigned long long) pi3.unique,
                                        (unsigned long long) pi3.multi, (unsigned long long) pi3.unplaced, (unsigned long long) pi3.pairs_proper, (unsigned long long) pi3.pairs,
                                        (long long) pi3.insert_median, pi3.ms_total);
                                spl = &pl3; spi = &pi3; spol = nullptr;
                            }
                        }
                    }
                    alga_placements pl4{};
                    alga_place_info pi4{};
                    if (rc == ALGA_OK && stitch) {                           // the joins of a first scaffolding whose two ends overlap become sequence, and the reads are placed on that
                        const bool have = pr.paired && spi->insert_median >= 0;
                        scp.insert = have ? (int32_t) spi->insert_median : 0;
                        scp.max_insert = pp.max_insert;
                        alga_scaffolds sc0;
                        alga_stitched sd{};
                        alga_stitch_info sti;
                        rc = alga_scaffold_placed_device(engine, &pnd, have ? (const uint8_t *) d_po : nullptr, spl, &scp, nullptr, &sc0, nullptr);
                        if (rc == ALGA_OK) rc = alga_stitch_scaffolds_device(engine, spl, &sc0, spol, &stp, nullptr, &sd, &sti);
                        if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot stitch the scaffold joins: %s (status %d)\n", alga_last_error(engine), rc); return 1; }
                        fprintf(stderr, "Scaffold joins stitched: %llu selected, %llu with an overlap, %llu ambiguous, %llu stitched, %llu bases removed, N50 %llu -> %llu; %llu "
                                "entries, %llu candidates outside the slack, %llu stitches dropped for cycles, %llu mismatches in the stitches, longest overlap %llu, %llu contigs "
                                "(%llu of several), %llu -> %llu columns; device ms: overlap %.3f build %.3f, call %.1f ms wall\n", (unsigned long long) sti.selected,
                                (unsigned long long) sti.with_overlap, (unsigned long long) sti.ambiguous, (unsigned long long) sti.stitched, (unsigned long long) sti.bases_removed,
                                (unsigned long long) sti.n50_before, (unsigned long long) sti.n50_after, (unsigned long long) sti.entries,
                                (unsigned long long) sti.candidates_outside_slack, (unsigned long long) sti.dropped_cycle, (unsigned long long) sti.join_mismatches,
                                (unsigned long long) sti.longest_overlap, (unsigned long long) sti.contigs, (unsigned long long) sti.contigs_multi,
                                (unsigned long long) sti.columns_before, (unsigned long long) sti.columns_after, sti.ms_overlap, sti.ms_build, sti.ms_total);
                        if (!stitched_path.empty()) {
                            alga_gfa_info sgi;
                            rc = alga_write_stitched_fasta_device(engine, &sd, stitched_path.c_str(), &sgi);
                            if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot write %s: %s (status %d)\n", stitched_path.c_str(), alga_last_error(engine), rc); return 1; }
                            fprintf(stderr, "Stitched contigs written -> %s: %llu records, %llu bytes\n", stitched_path.c_str(), (unsigned long long) sgi.segments,
                                    (unsigned long long) sgi.bytes);
                        }
                        if (!stitch_layout.empty()) {                        // not a hot path: the host formats from the arrays that came back
                            const size_t nt = (size_t) sd.n_targets, nj = (size_t) sd.n_stitched, nm = (size_t) sd.n_members, ne = (size_t) sd.n_entries;
                            std::vector<uint32_t> s_off(nj + 1), start(nt), off(nt + 1);
                            std::vector<int32_t> members(nm), rank(nt), ov(nt), entry(2 * nt);
                            std::vector<uint8_t> orient(nt), mm(ne);
                            rc = alga_copy_to_host(engine, s_off.data(), sd.d_s_off, (nj + 1) * sizeof(uint32_t));
                            if (rc == ALGA_OK) rc = alga_copy_to_host(engine, off.data(), spl->d_col_off, (nt + 1) * sizeof(uint32_t));
                            if (rc == ALGA_OK && nm) rc = alga_copy_to_host(engine, members.data(), sd.d_s_members, nm * sizeof(int32_t));
                            if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, rank.data(), sd.d_rank, nt * sizeof(int32_t));
                            if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, ov.data(), sd.d_overlap_after, nt * sizeof(int32_t));
                            if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, start.data(), sd.d_start, nt * sizeof(uint32_t));
                            if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, orient.data(), sd.d_orient, nt);
                            if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, entry.data(), sd.d_end_entry, 2 * nt * sizeof(int32_t));
                            if (rc == ALGA_OK && ne) rc = alga_copy_to_host(engine, mm.data(), sd.d_j_mm, ne);
                            FILE *f = rc == ALGA_OK ? fopen(stitch_layout.c_str(), "w") : nullptr;
                            if (rc == ALGA_OK && !f) { fprintf(stderr, "alga_hip: cannot write %s\n", stitch_layout.c_str()); return 1; }
                            for (size_t j = 0; f && j < nj; j++)
                                for (uint32_t k = s_off[j]; k < s_off[j + 1]; k++) {
                                    const size_t c = (size_t) members[k];
                                    fprintf(f, "%zu\t%d\t%zu\t%c\t%u\t%u\t%d\t%d\n", j, rank[c], c, orient[c] ? '-' : '+', start[c], off[c + 1] - off[c], ov[c],
                                            ov[c] ? (int) mm[(size_t) entry[2 * c + (orient[c] ^ 1)]] : 0);
                                }
                            if (f && fclose(f) != 0) { fprintf(stderr, "alga_hip: cannot write %s\n", stitch_layout.c_str()); return 1; }
                        }
                        // the same reads on the stitched contigs (the stitch result keeps its own copy of the bases)
                        if (rc == ALGA_OK) rc = alga_place_reads_device(engine, &pnd, pr.paired ? (const uint8_t *) d_po : nullptr, sd.d_words, sd.d_begin, sd.d_len,
                                                                        (int32_t) sd.n_stitched, &pp, nullptr, &pl4, &pi4);
                        if (rc == ALGA_OK) {
                            fprintf(stderr, "Reads placed on the stitched contigs: %llu reads, %llu placed (%llu unique, %llu multi), %llu unplaced; %llu proper pairs of %llu, "
                                    "median insert %lld; call %.1f ms wall\n", (unsigned long long) pi4.reads, (unsigned long long) pi4.placed, (unsigned long long) pi4.unique,
                                    (unsigned long long) pi4.multi, (unsigned long long) pi4.unplaced, (unsigned long long) pi4.pairs_proper, (unsigned long long) pi4.pairs,
                                    (long long) pi4.insert_median, pi4.ms_total);
                            spl = &pl4; spi = &pi4; spol = nullptr;
                        }
                    }
                    if (rc == ALGA_OK && !scaffolds.empty()) {
                        const alga_placements &pl = *spl;                    // (shadows: from here on the placement the scaffolds are made from)
                        const alga_place_info &pi = *spi;
                        const bool have = pr.paired && pi.insert_median >= 0;
                        if (!have) fprintf(stderr, "Scaffolding skipped: the placement saw no proper pair, so there is no insert size; every contig is its own scaffold\n");
                        scp.insert = have ? (int32_t) pi.insert_median : 0;
                        scp.max_insert = pp.max_insert;
                        alga_scaffolds sc;
                        alga_scaffold_info si;
                        alga_gfa_info sgi;
                        rc = alga_scaffold_placed_device(engine, &pnd, have ? (const uint8_t *) d_po : nullptr, &pl, &scp, nullptr, &sc, &si);
                        if (rc == ALGA_OK) rc = alga_write_scaffold_fasta_device(engine, &pl, &sc, spol, scaffolds.c_str(), &sgi);
                        if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot write %s: %s (status %d)\n", scaffolds.c_str(), alga_last_error(engine), rc); return 1; }
                        fprintf(stderr, "Scaffolds: %llu links, %llu bundles supported, %llu joins, %llu scaffolds (%llu of several contigs), N50 %llu -> %llu; insert %d, "
                                "%llu split pairs (%llu too far), %llu bundles, %llu ambiguous ends, %llu joins dropped for cycles, longest %llu; device ms: links %.3f "
                                "chain %.3f, call %.1f ms wall; -> %s: %llu bytes\n", (unsigned long long) si.links, (unsigned long long) si.bundles_supported,
                                (unsigned long long) si.joins, (unsigned long long) si.scaffolds, (unsigned long long) si.scaffolds_multi, (unsigned long long) si.n50_targets,
                                (unsigned long long) si.n50_scaffolds, scp.insert, (unsigned long long) si.pairs_split, (unsigned long long) si.links_too_far,
                                (unsigned long long) si.bundles, (unsigned long long) si.ends_ambiguous, (unsigned long long) si.joins_dropped_cycle,
                                (unsigned long long) si.longest, si.ms_links, si.ms_chain, si.ms_total, scaffolds.c_str(), (unsigned long long) sgi.bytes);
                        if (!scaffold_layout.empty()) {                      // not a hot path: the host formats from the arrays that came back
                            const size_t nt = (size_t) sc.n_targets, ns = (size_t) sc.n_scaffolds, nm = (size_t) sc.n_members;
                            std::vector<uint32_t> off(nt + 1), s_off(ns + 1), links(nt);
                            std::vector<int32_t> members(nm), rank(nt), gap(nt);
                            std::vector<uint8_t> orient(nt);
                            std::vector<uint64_t> start(nt);
                            rc = alga_copy_to_host(engine, off.data(), pl.d_col_off, (nt + 1) * sizeof(uint32_t));
                            if (rc == ALGA_OK) rc = alga_copy_to_host(engine, s_off.data(), sc.d_s_off, (ns + 1) * sizeof(uint32_t));
                            if (rc == ALGA_OK && nm) rc = alga_copy_to_host(engine, members.data(), sc.d_s_members, nm * sizeof(int32_t));
                            if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, rank.data(), sc.d_rank, nt * sizeof(int32_t));
                            if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, gap.data(), sc.d_gap_after, nt * sizeof(int32_t));
                            if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, links.data(), sc.d_join_links, nt * sizeof(uint32_t));
                            if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, orient.data(), sc.d_orient, nt);
                            if (rc == ALGA_OK && nt) rc = alga_copy_to_host(engine, start.data(), sc.d_start, nt * sizeof(uint64_t));
                            FILE *f = rc == ALGA_OK ? fopen(scaffold_layout.c_str(), "w") : nullptr;
                            if (rc == ALGA_OK && !f) { fprintf(stderr, "alga_hip: cannot write %s\n", scaffold_layout.c_str()); return 1; }
                            for (size_t j = 0; f && j < ns; j++)
                                for (uint32_t k = s_off[j]; k < s_off[j + 1]; k++) {
                                    const size_t c = (size_t) members[k];
                                    fprintf(f, "%zu\t%d\t%zu\t%c\t%llu\t%u\t%d\t%u\n", j, rank[c], c, orient[c] ? '-' : '+', (unsigned long long) start[c], off[c + 1] - off[c],
                                            gap[c], links[c]);
                                }
                            if (f && fclose(f) != 0) { fprintf(stderr, "alga_hip: cannot write %s\n", scaffold_layout.c_str()); return 1; }
                        }
                    }
                    alga_device_free(engine, d_rows); alga_device_free(engine, d_plen); alga_device_free(engine, d_po);
                    alga_free_parsed_reads(&pr);
                } else
                if (rc == ALGA_OK) rc = alga_write_final_fasta_device(engine, &cu, &cs, &fc, contigs_final.c_str(), &ffi);
                if (rc != ALGA_OK) { fprintf(stderr, "alga_amd: cannot write %s: %s (status %d)\n", contigs_final.c_str(), alga_last_error(engine), rc); return 1; }
                fprintf(stderr, "Final contigs written -> %s: %llu records of %d contigs (min length %d, new reads %d %%, trim threshold %d): %llu short, %llu rejected, "
                        "%llu trimmed away; %llu filter rounds, %llu edges in the trim's build; device ms: filter %.3f trim %.3f, call %.1f ms wall; FASTA %llu bytes, "
                        "wall %.1f ms\n", contigs_final.c_str(), (unsigned long long) ffi.segments, cu.n_pairs, min_len, contigs_new_reads_percent, contigs_trim_threshold,
                        (unsigned long long) fci.n_short, (unsigned long long) fci.rejected, (unsigned long long) fci.trimmed_away, (unsigned long long) fci.filter_rounds,
                        (unsigned long long) fci.trim_edges, fci.ms_filter, fci.ms_trim, fci.ms_total, (unsigned long long) ffi.bytes, ffi.ms_total);
            }
        }
    }
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "HIP start-up %.1f ms, parse %.1f ms, duplicate/prefix removal %.1f ms wall (device %.3f ms), overlap graph %.1f ms wall (device %.3f ms: seed %.3f probe %.3f group %.3f reduce %.3f emit %.3f)\n",
            ms(t0, t_engine), ms(t_engine, t1), ms(t1, t1b), nodes.ms_device, ms(t1b, t2), st.ms_total, st.ms_seed, st.ms_probe, st.ms_group, st.ms_reduce, st.ms_emit);
    if (serialize) {
        int rc = alga_write_graph(graph.c_str(), nodes.n, final_edges.data(), n_final);
        if (rc != ALGA_OK) { fprintf(stderr, "cannot write %s\n", graph.c_str()); return 1; }
        fprintf(stderr, "Graph serialized! -> %s\n", graph.c_str());
    }
    final_edges.clear(); final_edges.shrink_to_fit();
    creator.clear();
    if (multi) alga_multi_destroy(multi); else alga_engine_destroy(engine);     // the engines and their HBM buffers do not outlive the graph
    if (!alga_exe.empty()) {
        // argv vector, no shell: nothing in a file name is interpreted
        std::vector<std::string> args{alga_exe};
        for (const std::string &a : passthrough) args.push_back(a);
        args.push_back("--deserialize_graph=1");
        std::vector<char *> av;
        std::string shown;
        for (std::string &a : args) { av.push_back(&a[0]); shown += (shown.empty() ? "" : " ") + a; }
        av.push_back(nullptr);
        fprintf(stderr, "handing over to the unchanged simplifier / contig stages: %s\n", shown.c_str());
        pid_t pid = 0;
        extern char **environ;
        if (posix_spawn(&pid, alga_exe.c_str(), nullptr, nullptr, av.data(), environ) != 0) { fprintf(stderr, "alga_hip: cannot start %s\n", alga_exe.c_str()); return 1; }
        int status = 0;
        if (waitpid(pid, &status, 0) < 0) return 1;
        return (WIFEXITED(status) && WEXITSTATUS(status) == 0) ? 0 : 1;
    }
    return 0;
}
