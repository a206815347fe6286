#!/bin/bash
# End-of-round evidence: bench line (default steps, --full), rocprofv3 kernel summary of the same command, PMC traffic of the
# dominant conv kernel (separate passes).  usage: bash tools/gpu_final.sh <tag>
TAG=${1:-final}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${LXO_OUT:-$R/measure_out}; mkdir -p $OUT
export PYTHONUNBUFFERED=1
cd $R
(timeout 600 python bench.py --full > $OUT/${TAG}_bench.log 2>&1; echo "bench rc=$?"); tail -1 $OUT/${TAG}_bench.log | cut -c1-400
cd /tmp && export TMPDIR=/tmp
(timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -- python $R/bench.py --full --no-cpu-baseline --no-pmc > $OUT/${TAG}_prof.log 2>&1; echo "prof rc=$?")
cd $R
DB=$(ls $OUT/${TAG}_prof/*/*_results.db 2>/dev/null | head -1)
if [ -n "$DB" ]; then python tools/prof_summary.py $DB $OUT/${TAG}_kernels.csv "$TAG"; python tools/prof_by_grid.py $DB > $OUT/${TAG}_bygrid.txt 2>&1; rm -rf $OUT/${TAG}_prof; fi
tail -1 $OUT/${TAG}_prof.log > $OUT/${TAG}_bench_line_profiled.json
cd /tmp
for CNT in FETCH_SIZE WRITE_SIZE; do
  (timeout 300 rocprofv3 --pmc $CNT --kernel-trace -d $OUT/${TAG}_pmc_$CNT -- python $R/tools/pmc_conv.py > $OUT/${TAG}_pmc_$CNT.log 2>&1; echo "pmc $CNT rc=$?")
done
cd $R
F=$(ls $OUT/${TAG}_pmc_FETCH_SIZE/*/*_results.db | head -1); Wd=$(ls $OUT/${TAG}_pmc_WRITE_SIZE/*/*_results.db | head -1)
python tools/pmc_traffic.py $F $Wd $OUT/${TAG}_conv_traffic.json conv_halo2wg_kernel
rm -rf $OUT/${TAG}_pmc_FETCH_SIZE $OUT/${TAG}_pmc_WRITE_SIZE
