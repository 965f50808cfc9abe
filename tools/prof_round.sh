#!/bin/bash
# round-end evidence run (GPU box): bench JSON with every leg (--full), rocprofv3 kernel-trace stats of the same command,
# FETCH_SIZE counter pass of the headline, TP shard timing.  Outputs under $OUT (default out/).
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
TAG=${1:-r75}
O=${OUT:-out}
mkdir -p $O
python bench.py --full > $O/${TAG}_bench.json.log 2>&1
rm -rf $O/prof_${TAG} $O/pmc_${TAG}
rocprofv3 --kernel-trace --stats -d $O/prof_${TAG} -o bench -- python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-whole-model > $O/${TAG}_prof_bench.log 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_${TAG} -o bench -- python bench.py --steps 3 --warmup 1 > $O/${TAG}_pmc_bench.log 2>&1
python tools/bench_tp_shards.py > $O/${TAG}_tp_shards.log 2>&1
find $O/prof_${TAG} $O/pmc_${TAG} -type f | head -20
