# tests + fp32 tail + mc loop + full bench + kernel-trace profile + PMC passes; results under $OUT (default out/)
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/out}
cd $ROOT
export TMPDIR=/tmp
mkdir -p $OUT
bash tools/gpu_tests.sh > $OUT/tests_tail.txt 2>&1; echo "tests rc=$?"; tail -3 $OUT/tests_tail.txt
timeout -k 10 120 python tools/fp32_tail.py > $OUT/fp32_tail.txt 2>&1 && cat $OUT/fp32_tail.txt | head -14
timeout -k 10 120 python tools/mc_loop.py 5 > $OUT/mc_loop.txt 2>&1 && cat $OUT/mc_loop.txt
timeout -k 10 120 python tools/graph_probe.py > $OUT/graph_probe.txt 2>&1; cat $OUT/graph_probe.txt | tail -3
timeout -k 10 120 python -m pytest tests/test_gpu_fullsize.py -q -s -k float32_matches_float64 > $OUT/f32_vs_f64.txt 2>&1; grep "fp32 vs fp64" $OUT/f32_vs_f64.txt
timeout -k 10 300 python -u bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { echo BENCH_FAIL; tail -20 $OUT/bench.err; exit 1; }
cat $OUT/bench.json | head -c 1500; echo
rm -rf $OUT/prof
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- python3 $ROOT/bench.py --full --no-cpu-baseline > $OUT/bench_prof.json 2> $OUT/prof.err || { echo PROF_FAIL; exit 1; }
cd $ROOT && python3 profiles/summarize.py $OUT/prof > $OUT/prof_summary.json && echo PROF_OK
bash tools/gpu_pmc2.sh
