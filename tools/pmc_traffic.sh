#!/bin/bash
# HBM traffic of the kbench kernels: FETCH_SIZE and WRITE_SIZE in SEPARATE rocprofv3 --pmc passes (TCC slots),
# counters only.  usage: tools/pmc_traffic.sh <tag> <kbench args>
tag=$1; shift
dir=${GLARE_OUT_DIR:-out}     # where the results go
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $dir
KB_REPS=2 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $dir/tr_f_$tag -o p -- python tools/kbench.py "$@" > $dir/tr_$tag.log 2>&1
KB_REPS=2 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $dir/tr_w_$tag -o p -- python tools/kbench.py "$@" >> $dir/tr_$tag.log 2>&1
python tools/rocpd_pmc.py $dir/tr_f_$tag/p_results.db $dir/tr_w_$tag/p_results.db > $dir/traffic_$tag.txt 2>&1
cat $dir/traffic_$tag.txt
