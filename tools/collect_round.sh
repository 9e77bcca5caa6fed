# GPU box: everything profiles/ holds for a round, in one call:  OUT=<results dir> bash tools/collect_round.sh r06
set -u
TAG=${1:-r06}
R=$GRAFT_REPO_ROOT
cd $R
OUT=${OUT:?set OUT to the directory that collects the results}
GF_MARGINS_OUT=$OUT/${TAG}_parity_margins.txt python -m pytest tests -m gpu -q -x -s > $OUT/${TAG}_gpu_suite.txt 2>&1
grep -E "passed|failed" $OUT/${TAG}_gpu_suite.txt | tail -2
grep -E "cfg3 in-batch|cfg4 workload" $OUT/${TAG}_gpu_suite.txt >> $OUT/${TAG}_parity_margins.txt
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.txt 2>&1; tail -4 $OUT/${TAG}_smoke.txt
python bench.py --full > $OUT/${TAG}_cfg3_bench.json 2> $OUT/${TAG}_bench_default.err
tail -c 300 $OUT/${TAG}_cfg3_bench.json
for wl in cfg3 cfg2 cfg5; do bash tools/profile.sh $TAG $wl > $OUT/${TAG}_profile_$wl.log 2>&1; done
bash tools/pmc_sq.sh $TAG > $OUT/${TAG}_cfg3_sq_counters.txt 2>&1
{ for a in "1 32 1024 0" "2 32 1024 0" "2 32 1024 9" "1 10 1024 0" "2 10 1024 9" "1 64 1024 0"; do python tools/physics_time.py $a 2>/dev/null | grep towers; done; } > $OUT/${TAG}_physics_times.txt
tools/micro/copy_probe > $OUT/${TAG}_copy_probe.txt 2>&1
ls $OUT | grep $TAG
