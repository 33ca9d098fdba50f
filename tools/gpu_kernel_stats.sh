set -x
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats128t -o st -- python3 $R/tools/prove_loop.py 128 6 tables=0,0 > $OUT/stats128t.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/bench -o st -- python3 $R/bench.py --full > $OUT/bench_under_rocprof.json 2> $OUT/bench.err
find $OUT/stats128t $OUT/bench -type f ! -name "*kernel_stats.csv" -delete
ls -la $OUT/stats128t $OUT/bench
tail -c 600 $OUT/bench_under_rocprof.json
