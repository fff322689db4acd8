#!/bin/bash
# The measurement batch behind profiles/ (run ON THE GPU BOX, from the repo root):  bash tools/measure_round.sh <tag> [OUT]   e.g. r02
#   1. counter passes for roofline.traffic           -> OUT/pmc/pmc_linattn.json
#   2. rocprofv3 kernel stats: 13 train steps         -> OUT/<tag>_train_kernel_stats.csv, <tag>_train_under_rocprof.json
#   3. rocprofv3 kernel stats: sampling leg alone     -> OUT/<tag>_sample_kernel_stats.csv
#   4. python bench.py --full (every leg)             -> OUT/bench_<tag>.json
# OUT defaults to out.  Copy what is to be judged from OUT/ into profiles/ afterwards.
set -e -o pipefail
TAG=${1:-r02}
OUT=${2:-out}
export TMPDIR=/tmp
mkdir -p $OUT
bash tools/pmc_passes.sh $OUT/pmc
cp $OUT/pmc/pmc_linattn.json profiles/pmc_linattn.json   # bench.py quotes roofline.traffic from profiles/ when the build id matches
rm -rf $OUT/prof_train $OUT/prof_sample
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_train -- python3 bench.py --train-only --steps 10 --warmup 3 \
  > $OUT/${TAG}_train_under_rocprof.json 2> $OUT/prof_train.err
cp "$(ls $OUT/prof_train/*/*_kernel_stats.csv | head -1)" $OUT/${TAG}_train_kernel_stats.csv
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_sample -- python3 tools/prof_sample.py 512 5 \
  > $OUT/prof_sample.log 2> $OUT/prof_sample.err
cp "$(ls $OUT/prof_sample/*/*_kernel_stats.csv | head -1)" $OUT/${TAG}_sample_kernel_stats.csv
rm -rf $OUT/prof_train $OUT/prof_sample $OUT/pmc/FETCH_SIZE $OUT/pmc/WRITE_SIZE $OUT/pmc/SQ $OUT/pmc/S_FETCH_SIZE $OUT/pmc/S_WRITE_SIZE $OUT/pmc/S_SQ   # (raw traces: not merged back)
python3 bench.py --full > $OUT/bench_${TAG}.json 2> $OUT/bench_${TAG}.err
tail -c 1500 $OUT/bench_${TAG}.json
