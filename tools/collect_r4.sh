#!/bin/bash
# usage (GPU box, via gpurun, from the repo root): bash tools/collect_r4.sh   -> gpurun_out/r4_*  (copy what is to be judged into profiles/)
# Everything profiles/r4_* holds, taken at one HEAD on one box.  One pass per evidence kind; PMC passes never share a run with a trace.
#   r4_bench.json                              python bench.py --full -- the driver's command of round 4 (exact headline + configs.{simple,guided,simple_split,guided_split,train})
#   r4_kernel_stats.csv / r4_guided_*          rocprofv3 --kernel-trace --stats, exact fp32 path (configs #2 / #3), + the JSON line of the same run
#   r4_split_kernel_stats.csv / r4_split_guided_*   the same with MOLDIFF_MATRIX_PATH=split_f16
#   r4_pmc_summary.json / r4_split_pmc_summary.json / r4_guided_* / r4_split_guided_*   tools/pmc_summary.py: three separate --pmc passes each
#   r4_train_fp16_kernel_stats.csv             kernel statistics of 10 fp16 training steps
#   r4_ubench_split.txt, r4_mfma_rounding.txt, r4_split_accuracy.txt, r4_split_delta_diag.txt   the split path's micro-benchmark and accuracy evidence
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/gpurun_out
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
python $ROOT/bench.py --full > $OUT/r4_bench.json 2> $OUT/r4_bench.err
for path in exact_f32 split_f16; do
  for cfg in simple guided; do
    pre=r4_; [ $path = split_f16 ] && pre=r4_split_
    flag=""; name=${pre}kernel_stats; jn=${pre}bench_under_rocprof
    if [ $cfg = guided ]; then flag="--guided"; name=${pre}guided_kernel_stats; jn=${pre}guided_bench_under_rocprof; fi
    rm -rf /tmp/prof_$cfg
    MOLDIFF_MATRIX_PATH=$path rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$cfg -o p -- python $ROOT/bench.py --steps 95 --warmup 5 --headline-only --no-cpu-baseline $flag > $OUT/$jn.json 2> /dev/null
    find /tmp/prof_$cfg -name "*kernel_stats.csv" -exec cp {} $OUT/$name.csv \;
  done
done
python $ROOT/tools/pmc_summary.py $OUT/r4_pmc_summary.json > $OUT/r4_pmc.log 2>&1
python $ROOT/tools/pmc_summary.py $OUT/r4_guided_pmc_summary.json --guided >> $OUT/r4_pmc.log 2>&1
MOLDIFF_MATRIX_PATH=split_f16 python $ROOT/tools/pmc_summary.py $OUT/r4_split_pmc_summary.json >> $OUT/r4_pmc.log 2>&1
MOLDIFF_MATRIX_PATH=split_f16 python $ROOT/tools/pmc_summary.py $OUT/r4_split_guided_pmc_summary.json --guided >> $OUT/r4_pmc.log 2>&1
rm -rf /tmp/prof_tr
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_tr -o p -- python $ROOT/bench.py --train --precision fp16 --no-cpu-baseline --steps 10 > $OUT/r4_train_bench_fp16_under_rocprof.json 2> /dev/null
find /tmp/prof_tr -name "*kernel_stats.csv" -exec cp {} $OUT/r4_train_fp16_kernel_stats.csv \;
cd $ROOT
timeout 300 tools/ubench_split 8 > $OUT/r4_ubench_split.txt 2>&1
timeout 60 tools/mfma_rounding > $OUT/r4_mfma_rounding.txt 2>&1
python tools/split_accuracy.py > $OUT/r4_split_accuracy.txt 2>/dev/null
python tools/split_delta_diag.py > $OUT/r4_split_delta_diag.txt 2>/dev/null
ls -la $OUT | grep r4_
