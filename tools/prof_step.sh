#!/bin/bash
# rocprofv3 kernel trace of the headline bench + per-step breakdown: bash tools/prof_step.sh <tag> [extra env assignments...]
# writes <tag>_kernel_stats.csv, <tag>_step_breakdown.txt under $COUNTR_OUT (default prof_out/)
tag=$1; shift
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
out=${COUNTR_OUT:-prof_out}
mkdir -p $out
rm -rf /tmp/prof_$tag
env "$@" rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$tag -o p -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-b32 --no-other > $out/${tag}_bench.log 2>&1
f=$(find /tmp/prof_$tag -name "*kernel_trace.csv" | head -1)
s=$(find /tmp/prof_$tag -name "*kernel_stats.csv" | head -1)
cp $s $out/${tag}_kernel_stats.csv
python tools/step_breakdown.py $f 8 adamw_kernel 18 > $out/${tag}_step_breakdown.txt 2>&1
head -60 $out/${tag}_step_breakdown.txt
