#!/bin/bash
# One measurement cycle on the GPU box: parity tests, bench line (--full), rocprof kernel summary of a plain run.
# usage: bash tools/gpu_cycle.sh <tag> [steps]
TAG=${1:-cycle}; STEPS=${2:-4}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${LXO_OUT:-$R/measure_out}; mkdir -p $OUT
export PYTHONUNBUFFERED=1
cd $R
[ -n "$SKIPTESTS" ] || (timeout 900 python -m pytest tests -m gpu -q -x > $OUT/${TAG}_tests.log 2>&1; echo "tests rc=$?")
tail -4 $OUT/${TAG}_tests.log
(timeout 600 python bench.py --full --steps $STEPS --warmup 2 --no-cpu-baseline > $OUT/${TAG}_bench.log 2>&1; echo "bench rc=$?")
tail -2 $OUT/${TAG}_bench.log
cd /tmp && export TMPDIR=/tmp
(timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -- python $R/bench.py --steps 2 --warmup 1 > $OUT/${TAG}_prof.log 2>&1; echo "prof rc=$?")
cd $R
DB=$(ls $OUT/${TAG}_prof/*/*_results.db 2>/dev/null | head -1)
if [ -n "$DB" ]; then python tools/prof_summary.py $DB $OUT/${TAG}_kernels.csv "$TAG"; head -14 $OUT/${TAG}_kernels.csv | cut -c1-150; python tools/prof_by_grid.py $DB > $OUT/${TAG}_bygrid.txt 2>&1; python tools/prof_seq.py $DB conv_ 120 > $OUT/${TAG}_convseq.txt 2>&1; rm -rf $OUT/${TAG}_prof; fi
