set -x
cd "$(dirname "$0")/.."
O=${OUT:-out}
mkdir -p $O
python -m pytest tests -m gpu -q --tb=line 2>&1 | tail -5 > $O/r23_tests.log
python bench.py --full --steps 100 --warmup 10 > $O/r23_bench.log 2>&1
export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/prof_r23 -o bench -- python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline > $O/r23_prof_bench.log 2>&1
ls -R $O/prof_r23 | head -30
