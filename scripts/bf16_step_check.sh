#!/bin/bash
# The bf16 training step on the GPU box: kernel + gradient tests, the step time, and a per-kernel / critical-path profile of one step.
# usage: bash scripts/bf16_step_check.sh [tag]      -> $OUT/<tag>_* (OUT defaults to out/ in the repository)
tag=${1:-bf16_step}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}; mkdir -p $OUT
cd $R
timeout 1500 python3 -m pytest tests/test_gpu_bf16.py -x -q -m gpu -k "wgrad or backward or training or self_attn or flash or helpers" 2>&1 | tail -8
python3 bench.py --full --dtype bf16 --steps 10 --warmup 3 --steady 0 --cpu-sample 0 --no-input-stage --no-secondary --no-events --full-step 8 > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err
python3 -c "
import json
d=json.load(open('$OUT/${tag}_bench.json'))
print('bf16 fwd + loss ms', d['ms_per_step'], ' full training step ms', d['full_step']['ms_per_step'])
"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${tag}_prof -o fs -- python3 $R/bench.py --full --dtype bf16 --steps 4 --warmup 2 --steady 0 --cpu-sample 0 --no-input-stage --no-secondary --no-events --full-step 8 > $OUT/${tag}_prof.log 2>&1
cd $R
python3 scripts/critical_path.py $(ls $OUT/${tag}_prof/*kernel_trace.csv | head -1) "GSSD++ B=32 bf16 storage mode, FULL training step" 5 > $OUT/${tag}_critical_path.txt 2>&1
head -5 $OUT/${tag}_critical_path.txt
