#!/bin/bash
# tools/ab_so.sh A.so B.so ... : matcher-only bench lines of alternative builds of the library, one after the other in one call
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=$(realpath -m "${OUT:-$ROOT/out}") && mkdir -p $OUT   # results folder (default: out/ in the repository)
for so in "$@"; do
  VISO_HIP_SO=$so python bench.py --full --steps 20 --warmup 5 --no-cpu --no-streaming --no-images --no-e2e 2>/dev/null > $OUT/ab_tmp.json || true
  python - "$so" <<EOP
import json,sys
d=json.loads(open("$OUT/ab_tmp.json").read().strip().split("\n")[-1])
print(sys.argv[1], round(d["value"]), d["ms_per_step"], d["roofline"].get("kernel_ms"))
EOP
done
