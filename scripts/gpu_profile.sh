#!/bin/bash
# rocprofv3 passes: kernel trace + stats of the bench and of the kernel
# microbenchmarks, then separate PMC passes (FETCH_SIZE, WRITE_SIZE) on the
# K1 calibration workload.  Every step is time-limited; stop at the first failure.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
o=${HHFM_OUT:-out}/prof
mkdir -p $o
timeout -k 10 500 rocprofv3 --kernel-trace --stats -d $o/trace -o bench --output-format csv -- python3 bench.py --full --steps 10 --warmup 3 --cpu-seconds 0 --no-pmc > $o/bench_under_rocprof.json 2> $o/trace.err || { echo "bench trace failed"; tail $o/trace.err; exit 1; }
timeout -k 10 500 rocprofv3 --kernel-trace --stats -d $o/mb -o mb --output-format csv -- python3 scripts/microbench.py > $o/mb.json 2> $o/mb.err || { echo "microbench trace failed"; tail $o/mb.err; exit 1; }
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE -d $o/fetch -o pmc --output-format csv -- python3 scripts/pmc_fm_rows.py > $o/fetch.log 2>&1 || { echo "fetch pmc failed"; tail $o/fetch.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE -d $o/write -o pmc --output-format csv -- python3 scripts/pmc_fm_rows.py > $o/write.log 2>&1 || { echo "write pmc failed"; tail $o/write.log; exit 1; }
cat $o/mb.json
