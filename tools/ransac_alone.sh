# every kernel of the full pipeline ALONE (one batch, synchronize per run): durations, then SQ counters of the RANSAC stage
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=$(realpath -m "${OUT:-$ROOT/out}") && mkdir -p $OUT   # results folder (default: out/ in the repository)
cd /tmp && export TMPDIR=/tmp && cd $ROOT
export PYTHONPATH=.
rocprofv3 --kernel-trace --stats -d $OUT/alone -o s --output-format csv -- python3 tools/run_alone.py ${1:-512} 12 > $OUT/alone.txt 2>&1
tail -1 $OUT/alone.txt
python3 tools/kstats_table.py $OUT/alone/s_kernel_stats.csv 24
rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE SQ_WAIT_INST_ANY SQ_INSTS_SALU --kernel-trace -d $OUT/alonepmc -o p --output-format csv -- python3 tools/run_alone.py ${1:-512} 6 > /dev/null 2>$OUT/alonepmc.err
python3 - <<'PY'
import collections, csv, os
acc=collections.defaultdict(lambda: collections.defaultdict(list))
for r in csv.DictReader(open(os.environ["OUT"] + "/alonepmc/p_counter_collection.csv")):
    acc[r["Kernel_Name"]][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k,v in acc.items():
    if "ransac" in k or "inlier" in k or "circle" in k:
        print(k.split("(")[0], {c:round(sum(x)/len(x)) for c,x in v.items()})
PY
