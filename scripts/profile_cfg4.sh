#!/bin/bash
# Profiles one bench workload on a GPU machine (run from the repo root; outputs under $OUT, default scratch/profile):
#   kernel trace + stats, then the two PMC passes for HBM traffic (separate runs, as the guide prescribes).
# Outputs land in $OUT/{prof_kt,pmc_fetch,pmc_write}; condense them with profiles/summarize_rocprof.py.
R=${GRAFT_REPO_ROOT:-$(pwd)}
W=${1:-cfg4}
O=${OUT:-$R/scratch/profile}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_kt $O/pmc_fetch $O/pmc_write
python3 $R/bench.py --workload $W --steps 10 --warmup 3 --full --no-secondary > $O/bench_$W.json 2> $O/bench_$W.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_kt -o run -- python3 $R/bench.py --workload $W --steps 5 --warmup 2 --no-cpu-baseline --no-secondary > $O/prof_kt.json 2> $O/prof_kt.err
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_fetch -o run -- python3 $R/bench.py --workload $W --steps 1 --warmup 0 --no-cpu-baseline --no-secondary > $O/pmc_fetch.json 2> $O/pmc_fetch.err
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_write -o run -- python3 $R/bench.py --workload $W --steps 1 --warmup 0 --no-cpu-baseline --no-secondary > $O/pmc_write.json 2> $O/pmc_write.err
ls $O/prof_kt $O/pmc_fetch $O/pmc_write
tail -c 400 $O/bench_$W.json
