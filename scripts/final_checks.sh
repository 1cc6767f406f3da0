R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}; mkdir -p $OUT
cd $R
python -c "import __graft_entry__ as g; g.smoke(); print('SMOKE OK')" > $OUT/r06_smoke.txt 2>&1
python -m pytest tests -m gpu -q 2>&1 | tail -6 > $OUT/gpu_suite.txt
python3 bench.py --full --gpus 1 --steps 20 --warmup 5 --detail $OUT/r06_driver_command_bench_detail.json > $OUT/r06_driver_command_bench.json 2> $OUT/r06_bench.err
python3 bench.py --full --detail $OUT/r06_gssdpp_b32_bench_detail.json > $OUT/r06_gssdpp_b32_bench.json 2>> $OUT/r06_bench.err
cd /tmp && export TMPDIR=/tmp
for dt in f32 bf16; do
  timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r06_prof_$dt -o p -- python3 $R/bench.py --full --full-step 0 --cpu-sample 0 --no-input-stage --no-secondary --no-bf16 --steps 20 --warmup 5 --steady 0 --dtype $dt > /dev/null 2>&1
  f=$(find $OUT/r06_prof_$dt -name '*kernel_stats.csv' | head -1)
  [ -n "$f" ] && cp $f $OUT/r06_gssdpp_b32_${dt}_kernel_stats.csv
done
rm -rf $OUT/r06_prof_*
tail -3 $OUT/gpu_suite.txt; cat $OUT/r06_smoke.txt | tail -2
