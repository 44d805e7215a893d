# Round-end measurement set (GPU box): tests, bench line, rocprofv3 trace + HBM passes, SQ counters,
# phase stamps.  Usage: bash tools/gpu_round.sh <tag>
set -o pipefail
TAG=${1:-r03}
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { echo TESTS_FAILED; tail -30 $OUT/gpu_tests.log; exit 1; }
tail -2 $OUT/gpu_tests.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { echo SMOKE_FAILED; cat $OUT/smoke.log; exit 1; }
timeout -k 10 400 python -u bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { echo BENCH_FAILED; tail -20 $OUT/bench.err; exit 1; }
bash tools/profile_round.sh $TAG && bash tools/pmc_sq.sh $TAG && bash tools/stamps_all.sh $TAG && echo ROUND_OK
