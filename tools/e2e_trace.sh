# kernel trace of the end-to-end leg (3 batches in flight) -> timeline summary of its second half
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=$(realpath -m "${OUT:-$ROOT/out}") && mkdir -p $OUT   # results folder (default: out/ in the repository)
cd /tmp && export TMPDIR=/tmp && cd $ROOT
rocprofv3 --kernel-trace --stats -d $OUT/e2etrace -o s --output-format csv -- python3 bench.py --full --no-cpu --no-streaming --steps 40 > $OUT/e2etrace_bench.json 2>$OUT/e2etrace.err
python3 tools/trace_overlap.py $OUT/e2etrace/s_kernel_trace.csv 0.75 0.98
head -20 $OUT/e2etrace/s_kernel_stats.csv
