#!/bin/bash
# Runs on the GPU box (via gpurun): parity tests, bench, rocprofv3 kernel stats and the FETCH_SIZE / WRITE_SIZE PMC passes.
# Usage: bash scripts/gpu_profile.sh OUT (a directory relative to the repository root; scripts/collect_profiles.py
# reads it); the summaries that are judged are copied into profiles/ afterwards.
set -x
R=$GRAFT_REPO_ROOT
cd $R
O=${1:?usage: bash scripts/gpu_profile.sh OUT}
mkdir -p $O
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $O/pytest_gpu4.log 2>&1; tail -2 $O/pytest_gpu4.log
timeout -k 10 400 python bench.py --full > $O/bench3.json 2> $O/bench3.err; echo "bench rc=$?"
cd /tmp && export TMPDIR=/tmp
rm -rf $R/$O/prof3 $R/$O/pmc_*
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/prof3 -- python3 $R/bench.py --full --no-extras --no-cpu-baseline > $R/$O/prof3.log 2>&1; echo "prof rc=$?"
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $R/$O/pmc_fetch_1e6 -- python3 $R/bench.py --full --steps 30 --warmup 5 --no-extras --no-cpu-baseline > $R/$O/pmc_fetch_1e6.log 2>&1; echo "pmc1 rc=$?"
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $R/$O/pmc_write_1e6 -- python3 $R/bench.py --full --steps 30 --warmup 5 --no-extras --no-cpu-baseline > $R/$O/pmc_write_1e6.log 2>&1; echo "pmc2 rc=$?"
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $R/$O/pmc_fetch_1e7 -- python3 $R/bench.py --full --n-molecular 10000000 --frames 2 --steps 10 --warmup 2 --no-extras --no-cpu-baseline > $R/$O/pmc_fetch_1e7.log 2>&1; echo "pmc3 rc=$?"
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $R/$O/pmc_write_1e7 -- python3 $R/bench.py --full --n-molecular 10000000 --frames 2 --steps 10 --warmup 2 --no-extras --no-cpu-baseline > $R/$O/pmc_write_1e7.log 2>&1; echo "pmc4 rc=$?"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/prof3_1e7 -- python3 $R/bench.py --full --n-molecular 10000000 --frames 2 --steps 50 --warmup 5 --no-extras --no-cpu-baseline > $R/$O/prof3_1e7.log 2>&1; echo "prof1e7 rc=$?"
cd $R
ls $O/pmc_fetch_1e6/*/ | head
cat $O/prof3/*/*kernel_stats.csv | cut -c1-120
cat $O/prof3_1e7/*/*kernel_stats.csv | cut -c1-120
