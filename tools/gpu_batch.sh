set -x
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch5 -o f -- python3 $R/bench.py --full --steps 2 --warmup 1 --tables on --no-cpu-baseline --no-e2e --legs "" > $OUT/pmc_fetch5.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_write5 -o w -- python3 $R/bench.py --full --steps 2 --warmup 1 --tables on --no-cpu-baseline --no-e2e --legs "" > $OUT/pmc_write5.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats32t -o st -- python3 $R/tools/prove_loop.py 32 11 tables=0,0 > $OUT/stats32t.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats128t -o st -- python3 $R/tools/prove_loop.py 128 6 tables=0,0 > $OUT/stats128t.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats_bencht -o st -- python3 $R/bench.py --full --steps 3 --warmup 1 --tables on --no-cpu-baseline --no-e2e --legs 46,32 > $OUT/stats_bencht.log 2>&1
rocprofv3 --kernel-trace --output-format rocpd -d $OUT/tl128t -o tl -- python3 $R/tools/prove_loop.py 128 3 tables=0,0 > $OUT/tl128t.log 2>&1
rocprofv3 --kernel-trace --output-format rocpd -d $OUT/tl32t -o tl -- python3 $R/tools/prove_loop.py 32 6 tables=0,0 > $OUT/tl32t.log 2>&1
cd $R
python tools/timeline.py $(find $OUT/tl128t -name "*.db" | head -1) 0.0 > $OUT/tl128t.txt; rm -rf $OUT/tl128t
python tools/timeline.py $(find $OUT/tl32t -name "*.db" | head -1) 0.0 > $OUT/tl32t.txt; rm -rf $OUT/tl32t
python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; echo "bench_exit=$?"
python bench.py --full --workload prime --legs "" --no-cpu-baseline > $OUT/bench_prime.json 2> $OUT/bench_prime.err; echo "prime_exit=$?"
python bench.py --full --tables off --legs "46,32" --no-cpu-baseline --no-e2e > $OUT/bench_plain.json 2> $OUT/bench_plain.err; echo "plain_exit=$?"
python tools/sweep.py matrix 7 > $OUT/sweep_matrix.csv 2> $OUT/sweep_matrix.err
python tools/sweep.py fib 31 > $OUT/sweep_fib.csv 2> $OUT/sweep_fib.err
python tools/sweep.py prime 2 > $OUT/sweep_prime.csv 2> $OUT/sweep_prime.err
