# per-kernel durations of the image-in legs (resident uint8 images -> [Harris] -> descriptors -> matcher -> solver)
# STREAMS=1 (default): one batch in flight, durations that fit inside the step
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=$(realpath -m "${OUT:-$ROOT/out}") && mkdir -p $OUT   # results folder (default: out/ in the repository)
cd /tmp && export TMPDIR=/tmp && cd $ROOT
rocprofv3 --kernel-trace --stats -d $OUT/imgstats -o s --output-format csv -- python3 bench.py --full --streams ${STREAMS:-1} --no-cpu --no-streaming --no-e2e --steps 20 --warmup 3 > $OUT/imgstats_bench.json 2>$OUT/imgstats.err
python3 tools/kstats_table.py $OUT/imgstats/s_kernel_stats.csv 24
