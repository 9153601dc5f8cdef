#!/bin/bash
# Evidence pass for one config (CONFIG=gen|gan): rocprofv3 kernel-trace summary of a bench run,
# then FETCH_SIZE and WRITE_SIZE PMC passes (one counter block per run, kernel-trace only, no
# sys/runtime trace), each under its own time limit; stops at the first failure. Everything is
# written under $OUT_DIR (default prof_out/).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
O=${OUT_DIR:-prof_out}
mkdir -p $O
export TMPDIR=/tmp
C=${CONFIG:-gen}
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_$C -o run --output-format csv -- \
    python3 bench.py --full --config $C --steps 5 --warmup 2 --no-cpu-baseline > $O/prof_$C.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE -d $O/pmcF_$C -o run --output-format csv -- \
    python3 bench.py --config $C --steps 2 --warmup 1 --no-graphs > $O/pmcF_$C.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE -d $O/pmcW_$C -o run --output-format csv -- \
    python3 bench.py --config $C --steps 2 --warmup 1 --no-graphs > $O/pmcW_$C.log 2>&1 || exit $?
grep '^{' $O/prof_$C.log
