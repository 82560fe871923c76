# rocprofv3 evidence for the image-in legs: per-kernel durations with ONE batch in flight and the two
# HBM-traffic counter passes, of `python3 bench.py --no-cpu --no-streaming --no-e2e` (resident uint8 images -> [binned
# Harris] -> descriptors -> matcher -> solver; the program directly behind `--`)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=$(realpath -m "${OUT:-$ROOT/out}") && mkdir -p $OUT   # results folder (default: out/ in the repository)
TAG=${1:-r06}
cd /tmp && export TMPDIR=/tmp && cd $ROOT
Q="--full --streams 1 --e2e-streams 1 --no-cpu --no-streaming --no-e2e --no-i16 --steps 12 --warmup 2 --min-region-seconds 0"
rocprofv3 --kernel-trace --stats -d $OUT/img_stats -o s --output-format csv -- python3 bench.py $Q > $OUT/img_stats_bench.json 2>$OUT/img_stats.err &&
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/img_fetch -o p --output-format csv -- python3 bench.py $Q > /dev/null 2>$OUT/img_fetch.err &&
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/img_write -o p --output-format csv -- python3 bench.py $Q > /dev/null 2>$OUT/img_write.err &&
VISO_PMC_COMMAND="rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE --kernel-trace --output-format csv -- python3 bench.py $Q (two separate passes, tools/image_profile.sh)" \
VISO_PMC_WORKLOAD="the resident image-in legs of bench.py: 512 pairs of synthetic 1241x376 uint8 stereo images per batch, ONE batch in flight; keypoints given (2000 per image) and binned Harris on the device (1200 per image) -> descriptors -> matcher -> solver" \
python3 tools/pmc_to_json.py $OUT/img_fetch $OUT/img_write harris_detect_kernel > $OUT/${TAG}_pmc_hbm_images.json &&
cp $OUT/img_stats/s_kernel_stats.csv $OUT/${TAG}_kernel_stats_images.csv &&
cp $OUT/img_stats_bench.json $OUT/${TAG}_bench_under_rocprof_images.json
python3 tools/kstats_table.py $OUT/${TAG}_kernel_stats_images.csv 12
