# Kernel trace of a short bench.py run (headline, augment and eval legs) and its idle-gap table.
# Usage: bash tools/trace_gaps.sh [output directory, default trace_out/tr]
OUT=${1:-trace_out/tr}
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/raw -o t -- python3 bench.py --full --steps 6 --warmup 3 --precision ${PREC:-f32} --no-cpu-baseline --no-roofline > $OUT/log 2>&1 || exit 1
f=$(find $OUT/raw -name '*kernel_trace.csv' | head -n 1)
python3 tools/gap_analysis.py $f 40 > $OUT/gaps.txt
cp $f $OUT/trace.csv
rm -rf $OUT/raw
