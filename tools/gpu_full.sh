# Full GPU check of the tree: parity tests, smoke, the full bench line.  Usage, on an MI355X:  bash tools/gpu_full.sh OUTDIR
set -x
O=$(realpath -m "${1:?usage: bash tools/gpu_full.sh OUTDIR}")
cd "$(dirname "$0")/.."
mkdir -p "$O"
timeout 1500 python -m pytest tests -m gpu -x -q > "$O/gputests.log" 2>&1; echo "pytest rc=$?" >> "$O/gputests.log"
tail -5 "$O/gputests.log"
timeout 200 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
timeout 600 python bench.py --full 2> "$O/bench_err.log" | tail -1 > "$O/bench_default.json"
cut -c1-600 "$O/bench_default.json"
