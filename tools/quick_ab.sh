ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=$(realpath -m "${OUT:-$ROOT/out}") && mkdir -p $OUT   # results folder (default: out/ in the repository)
python -m pytest tests/test_gpu_parity.py tests/test_gpu_fullsize.py tests/test_gpu_fuzz.py tests/test_gpu_robustness.py -x -q -m gpu > $OUT/t1.log 2>&1; tail -3 $OUT/t1.log; python bench.py --full --steps 20 --warmup 5 --no-cpu --no-streaming --no-images > $OUT/b1.json 2> $OUT/b1.err; python - <<EOP
import json
d=json.loads(open("$OUT/b1.json").read().strip().split("\n")[-1])
print(d["value"], d["ms_per_step"], d["roofline"].get("kernel_ms"), d["end_to_end"]["fps"])
EOP
