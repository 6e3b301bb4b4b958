#!/bin/bash
# round 6 checkpoint: the whole GPU suite, then the default bench line
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
o=${HHFM_OUT:-out}/r06
mkdir -p $o
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $o/pytest_gpu.txt 2>&1
rc=$?
grep -E 'passed|failed|error' $o/pytest_gpu.txt | tail -3
[ $rc -ne 0 ] && { tail -40 $o/pytest_gpu.txt; exit 1; }
timeout -k 10 600 python bench.py --full > $o/bench.json 2> $o/bench.err || { tail -20 $o/bench.err; exit 1; }
tail -c 3000 $o/bench.json
