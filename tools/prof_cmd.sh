# Kernel trace of a bench run with every GPU leg, and the PMC passes (FETCH_SIZE, WRITE_SIZE) over it.  Usage:  bash tools/prof_cmd.sh OUTDIR
set -x
O=$(realpath -m "${1:?usage: bash tools/prof_cmd.sh OUTDIR}"); mkdir -p "$O"
R=$(realpath "$(dirname "$0")/..")
cd /tmp && export TMPDIR=/tmp
timeout 400 rocprofv3 --kernel-trace -d /tmp/ks -o ks -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > /tmp/ks.log 2>&1 < /dev/null
tail -c 300 /tmp/ks.log
DB=$(find /tmp/ks -name "*.db" | head -1); echo "db=$DB"
[ -n "$DB" ] && timeout 60 python $R/tools/rocprof_summary.py "$DB" > $O/kernel_stats.txt
timeout 400 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d /tmp/pf -o pf -- python $R/bench.py --full --steps 1 --warmup 1 --tiles 1020 --no-cpu-baseline > /tmp/pf.log 2>&1 < /dev/null
timeout 400 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d /tmp/pw -o pw -- python $R/bench.py --full --steps 1 --warmup 1 --tiles 1020 --no-cpu-baseline > /tmp/pw.log 2>&1 < /dev/null
F=$(find /tmp/pf -name "*.db" | head -1); W=$(find /tmp/pw -name "*.db" | head -1); echo "f=$F w=$W"
[ -n "$F" ] && [ -n "$W" ] && timeout 60 python $R/tools/pmc_summary.py "$F" "$W" gemm layernorm attn > $O/pmc_summary.txt
head -30 $O/pmc_summary.txt
