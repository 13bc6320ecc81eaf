#!/bin/bash
# The first block of tools/profile_round.sh alone: the bench line, the rocprofv3 kernel-trace summary of the same command on one stream,
# the generated agreement check and the batch-4 line.   usage: tools/profile_bench_only.sh r06   -> $GLARE_OUT_DIR (default out)/<tag>_*
tag=${1:-rXX}
dir=${GLARE_OUT_DIR:-out}     # where the results go
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $dir
python bench.py --full --steps 20 --warmup 5 > $dir/${tag}_bench_line.json 2> $dir/${tag}_bench.err
rocprofv3 --kernel-trace --stats -d $dir/prof_$tag -o b -- python bench.py --full --steps 5 --warmup 2 --streams 1 --no-cpu-baseline --no-train --no-power > $dir/${tag}_bench_prof.log 2>&1
python tools/rocpd_stats.py $(ls $dir/prof_$tag/*/b_results.db $dir/prof_$tag/b_results.db 2>/dev/null | head -1) > $dir/${tag}_bench_kernel_stats.txt 2>&1
python tools/agreement_check.py $dir/${tag}_bench_line.json $dir/${tag}_bench_kernel_stats.txt > $dir/${tag}_agreement.txt 2>&1
python bench.py --full --batch 4 --steps 20 --warmup 5 --no-train --no-cpu-baseline > $dir/${tag}_bench_line_b4.json 2>> $dir/${tag}_bench.err
rm -rf $dir/prof_$tag
ls -la $dir | grep $tag
