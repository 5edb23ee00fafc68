#!/bin/bash
# Round 4's measurement suite on one GPU box (run through gpurun; everything lands under gpurun_out/r04_final/):
#   part A: the whole -m gpu suite; kernel trace + memory-request counters of the default bench (BASELINE configs[3]) -> traffic file -> the bench
#           line itself (with first-call legs, PCIe leg, CPU baseline); the same for configs[4]; bench lines of configs[1], configs[2]
#   part B: one rank's compute at world sizes 2 / 4 / 8 on one GPU, both forms of the N-rank build: replicated index (tools/emulate_rank.py) and
#           index sharded by seed bucket (tools/emulate_shard.py: all ranks, graph == one-GPU graph, exchange volumes); the C++ driver, both
#           forms, as 2 ranks at the north-star size against one engine
#   part C: full-size parity on THIS tree against the recorded reference dumps (sha256): 50 M reads error-free, 10 M reads with 2 % errors
# usage: tools/final_measure_r04.sh A1|A2|B|C      (A1: suite + configs[3]; A2: configs[4], configs[1], configs[2])
set -u
PART=${1:-A}
REPO=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=$REPO/gpurun_out/r04_final
mkdir -p $OUT
cd $REPO
export TMPDIR=/tmp
if [ "$PART" = A1 ] || [ "$PART" = A2 ]; then
  if [ "$PART" = A1 ]; then
    timeout -k 10 1000 python -m pytest tests -x -q -m gpu > $OUT/pytest_gpu.log 2>&1; rc=$?
    tail -3 $OUT/pytest_gpu.log
    [ $rc -ne 0 ] && exit $rc
    CFGS="cfg4_50M_150bp"
  else
    CFGS="cfg5_10M_150bp_err2"
  fi
  for CFG in $CFGS; do
    timeout -k 10 900 bash tools/profile_cmd.sh r04_final_$CFG trx bench.py --full --config $CFG --steps 5 --warmup 2 --no-cpu-baseline --no-pcie --no-first-call || exit 1
    python tools/pmc_to_traffic.py gpurun_out/prof_r04_final_$CFG $CFG > $OUT/traffic_$CFG.json || exit 1
    cp gpurun_out/prof_r04_final_$CFG/summary.txt $OUT/rocprof_$CFG.txt
    timeout -k 10 600 python bench.py --full --config $CFG > $OUT/bench_$CFG.json 2> $OUT/bench_$CFG.err || { tail -20 $OUT/bench_$CFG.err; exit 1; }
    echo "$CFG: $(python3 -c "import json,sys; d=json.loads(open('$OUT/bench_$CFG.json').read().strip().splitlines()[-1]); print(d['ms_per_step'], d['value'], d['roofline']['frac'], d['roofline']['traffic'], d.get('ms_end_to_end'))")"
  done
  cp profiles/hbm_traffic.json $OUT/hbm_traffic.json
  [ "$PART" = A1 ] && exit 0
  for CFG in cfg2_1M_150bp cfg3_5M_150bp; do
    timeout -k 10 600 python bench.py --full --config $CFG > $OUT/bench_$CFG.json 2> $OUT/bench_$CFG.err || { tail -20 $OUT/bench_$CFG.err; exit 1; }
    echo "$CFG: $(python3 -c "import json,sys; d=json.loads(open('$OUT/bench_$CFG.json').read().strip().splitlines()[-1]); print(d['ms_per_step'], d['value'])")"
  done
elif [ "$PART" = B ]; then
  : > $OUT/emulated_rank_compute.jsonl
  : > $OUT/emulated_bucket_sharded.jsonl
  for N in 2 4 8; do
    timeout -k 10 300 python tools/emulate_rank.py $N 50000000 250000000 5 1 >> $OUT/emulated_rank_compute.jsonl 2> $OUT/emulate_$N.err || { tail -5 $OUT/emulate_$N.err; exit 1; }
    timeout -k 10 400 python tools/emulate_shard.py $N 50000000 250000000 3 >> $OUT/emulated_bucket_sharded.jsonl 2> $OUT/emulate_shard_$N.err || { tail -5 $OUT/emulate_shard_$N.err; exit 1; }
  done
  cut -c1-500 $OUT/emulated_rank_compute.jsonl
  cut -c1-700 $OUT/emulated_bucket_sharded.jsonl
  for FORM in replicated bucket_sharded; do
    timeout -k 10 600 python tools/multi_cxx_check.py 2 cfg4_50M_150bp $FORM > $OUT/multi_cxx_2ranks_50M_$FORM.json 2> $OUT/multi_cxx_$FORM.err || { tail -5 $OUT/multi_cxx_$FORM.err; exit 1; }
    cut -c1-1200 $OUT/multi_cxx_2ranks_50M_$FORM.json
  done
else
  timeout -k 10 600 python tools/run_cfg4.py 50000000 250000000 2 source_side 0 a21745295ac286551ab5ce9fd8a1b9b2107f53cab6c329ed32e819deb3aed925 > $OUT/cfg4_50M_dump_vs_recorded_reference.log 2>&1 || { tail -5 $OUT/cfg4_50M_dump_vs_recorded_reference.log; exit 1; }
  tail -1 $OUT/cfg4_50M_dump_vs_recorded_reference.log | cut -c1-900
  timeout -k 10 600 python tools/cfg5_exact_dump_hash.py > $OUT/cfg5_10M_exact_path_vs_recorded_reference.json 2> $OUT/cfg5_hash.err || { tail -5 $OUT/cfg5_hash.err; exit 1; }
  cat $OUT/cfg5_10M_exact_path_vs_recorded_reference.json
fi
