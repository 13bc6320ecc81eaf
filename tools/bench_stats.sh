#!/bin/bash
# rocprofv3 kernel-trace summary of a short bench run -> $GLARE_OUT_DIR (default out)/<tag>_bench_kernel_stats.txt (+ the bench line)
tag=${1:-rXX}
dir=${GLARE_OUT_DIR:-out}     # where the results go
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $dir
rocprofv3 --kernel-trace --stats -d $dir/prof_$tag -o b -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $dir/${tag}_bench_prof.log 2>&1
python tools/rocpd_stats.py $(ls $dir/prof_$tag/*/b_results.db $dir/prof_$tag/b_results.db 2>/dev/null | head -1) > $dir/${tag}_bench_kernel_stats.txt 2>&1
rm -rf $dir/prof_$tag
head -16 $dir/${tag}_bench_kernel_stats.txt
grep -o '"value": [0-9.]*' $dir/${tag}_bench_prof.log
