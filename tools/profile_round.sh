# rocprofv3 evidence for profiles/ (run on the GPU box: gpurun -- 'bash tools/profile_round.sh [tag]'):
#   1. kernel-trace stats of the default bench run (3 batches in flight: kernels of different streams overlap)
#   2. kernel-trace stats of the same workload with ONE stream: per-kernel averages that fit inside the step
#   3./4. the two HBM-traffic counter passes (separate runs, one stream)
# then: python3 tools/pmc_to_json.py $OUT/prof_fetch $OUT/prof_write <kernel> > profiles/<round>_pmc_hbm.json
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=$(realpath -m "${OUT:-$ROOT/out}") && mkdir -p $OUT   # results folder (default: out/ in the repository)
TAG=${1:-r06}
cd /tmp && export TMPDIR=/tmp && cd $ROOT
Q="--full --no-cpu --no-e2e --no-streaming --no-images --no-i16"   # matcher step only (--no-e2e also leaves the drop-in leg out)
rocprofv3 --kernel-trace --stats -d $OUT/prof_stats -o s --output-format csv -- python3 bench.py --full --no-cpu --no-streaming --no-images --no-i16 --no-drop-in > $OUT/prof_stats_bench.json 2>$OUT/prof_stats.err &&
rocprofv3 --kernel-trace --stats -d $OUT/prof_stats1 -o s --output-format csv -- python3 bench.py --streams 1 $Q > $OUT/prof_stats1_bench.json 2>$OUT/prof_stats1.err &&
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/prof_fetch -o p --output-format csv -- python3 bench.py --streams 1 --steps 4 --warmup 1 --min-region-seconds 0 $Q > /dev/null 2>$OUT/prof_fetch.err &&
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/prof_write -o p --output-format csv -- python3 bench.py --streams 1 --steps 4 --warmup 1 --min-region-seconds 0 $Q > /dev/null 2>$OUT/prof_write.err &&
K=$(python3 -c "import json;print(json.load(open('$OUT/prof_stats1_bench.json'))['roofline']['kernel'])") &&
python3 tools/pmc_to_json.py $OUT/prof_fetch $OUT/prof_write "$K" > $OUT/${TAG}_pmc_hbm.json &&
cp $OUT/prof_stats/s_kernel_stats.csv $OUT/${TAG}_kernel_stats_3streams.csv &&
cp $OUT/prof_stats1/s_kernel_stats.csv $OUT/${TAG}_kernel_stats_1stream.csv &&
cp $OUT/prof_stats_bench.json $OUT/${TAG}_bench_under_rocprof_3streams.json &&
cp $OUT/prof_stats1_bench.json $OUT/${TAG}_bench_under_rocprof_1stream.json
