#!/bin/bash
# rocprofv3 kernel stats of a short single-stream bench run; prints the kernels matching $1 (default: all top 25)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${PROF_OUT:-$R/prof_out}/prof_s1q
rm -rf $O && mkdir -p $O
rocprofv3 --kernel-trace --stats --output-format csv -d $O -o b -- python3 $R/bench.py --streams 1 --depth 1 --match-lanes 1 --steps 30 --full --no-cpu-baseline --no-roofline > $O.json 2> $O.err </dev/null || { echo "bench failed"; tail -5 $O.err; exit 1; }
python3 $R/scripts/kstats.py "${1:-k_}" $O/b_kernel_stats.csv
