#!/bin/bash
# Per-layer event table + rocprofv3 kernel-trace summary of one config (CONFIG=gen|gan|48k).
# Everything is written under $OUT_DIR (default prof_out/).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
O=${OUT_DIR:-prof_out}
mkdir -p $O
export TMPDIR=/tmp
C=${CONFIG:-gan}
timeout -k 10 300 python tools/layer_table.py --config $C > $O/layers_$C.md 2> $O/layers_$C.err || exit $?
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_$C -o run --output-format csv -- \
    python3 bench.py --full --config $C --steps 5 --warmup 2 --no-cpu-baseline > $O/prof_$C.log 2>&1 || exit $?
N=1; [ "$C" != gen ] && N=2
python tools/prof_summary.py $O/prof_$C 60 --adams-per-step $N > $O/step_kernels_$C.md
