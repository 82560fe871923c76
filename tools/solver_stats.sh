# per-kernel averages of one batch alone (full pipeline)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
export OUT=$(realpath -m "${OUT:-$ROOT/out}") && mkdir -p $OUT   # results folder (default: out/ in the repository)
cd /tmp && export TMPDIR=/tmp && cd $ROOT
export PYTHONPATH=.
rocprofv3 --kernel-trace --stats -d $OUT/solverstats -o s --output-format csv -- python3 tools/host_issue_cost.py ${1:-512} 0 1 > $OUT/solverstats.txt 2>&1
python3 tools/kstats_table.py $OUT/solverstats/s_kernel_stats.csv 22
