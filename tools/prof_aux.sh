# CTransPath bench line (every leg), and kernel traces of the MIL training step and the CTransPath forward.  Usage:  bash tools/prof_aux.sh OUTDIR
set -x
O=$(realpath -m "${1:?usage: bash tools/prof_aux.sh OUTDIR}"); mkdir -p "$O"
R=$(realpath "$(dirname "$0")/..")
cd /tmp && export TMPDIR=/tmp
timeout 400 python $R/bench.py --full --model ctranspath 2>/dev/null | tail -1 > $O/bench_ctranspath.json
timeout 300 rocprofv3 --kernel-trace -d /tmp/kt -o kt -- python $R/tools/train_only.py > /tmp/kt.log 2>&1 < /dev/null
DB=$(find /tmp/kt -name "*.db" | head -1); [ -n "$DB" ] && timeout 60 python $R/tools/rocprof_summary.py "$DB" > $O/mil_train_stats.txt
timeout 300 rocprofv3 --kernel-trace -d /tmp/ks2 -o ks2 -- python $R/tools/swin_only.py 1024 1024 2 > /tmp/ks2.log 2>&1 < /dev/null
DB=$(find /tmp/ks2 -name "*.db" | head -1); [ -n "$DB" ] && timeout 60 python $R/tools/rocprof_summary.py "$DB" > $O/ctranspath_stats.txt
cut -c1-300 $O/bench_ctranspath.json; head -5 $O/mil_train_stats.txt | cut -c1-160; head -5 $O/ctranspath_stats.txt | cut -c1-160
