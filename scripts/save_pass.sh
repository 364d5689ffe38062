# Copy a gpu_pass.sh pass out of its output directory ($OUT) into profiles/<dir>/:
#   bash scripts/save_pass.sh profiles/r03/head_<sha> [cfg]
set -e
OUT=${OUT:-bench_out}
d=$1; c=${2:-2}
mkdir -p $d
cp $OUT/bench.json $d/c${c}_bench.json
cp $OUT/prof/run_kernel_stats.csv $d/c${c}_kernel_stats.csv
python3 scripts/pmc_summary.py $OUT/pmc > $d/c${c}_pmc.json
grep -E "PASSED|FAILED|ERROR|passed|failed" $OUT/pytest_gpu.log > $d/pytest_gpu.txt || true
cp $OUT/smoke.log $d/smoke.txt
