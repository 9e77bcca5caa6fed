set -u
R=$GRAFT_REPO_ROOT
cd $R
OUT=${OUT:?set OUT to the directory that collects the results}
GF_MARGINS_OUT=$OUT/r06_parity_margins_start.txt timeout 3000 python -m pytest tests -m gpu -q -x -s > $OUT/r06_gpu_suite_start.txt 2>&1
grep -E "passed|failed|error" $OUT/r06_gpu_suite_start.txt | tail -3
grep -E "cfg3 in-batch|cfg4 workload" $OUT/r06_gpu_suite_start.txt
timeout 900 python bench.py --full > $OUT/r06_bench_start.json 2> $OUT/r06_bench_start.err
tail -c 600 $OUT/r06_bench_start.json
