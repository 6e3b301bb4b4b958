#!/bin/bash
# round 6: DeepFM wide kernel split (staged launch + overflow launch): tests, C5 legs, kernel trace
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
o=${HHFM_OUT:-out}/r06/dfm
mkdir -p $o
timeout -k 10 600 python -u -m pytest tests/test_gpu_dfm.py -m gpu -x -q --timeout 300 --timeout-method thread > $o/pytest.txt 2>&1 || { tail -40 $o/pytest.txt; exit 1; }
tail -2 $o/pytest.txt
timeout -k 10 300 python bench.py --full --legs c5 --no-pmc > $o/bench_c5.json 2> $o/bench_c5.err || { tail -20 $o/bench_c5.err; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $o/kt -o c5 -- python3 bench.py --full --legs c5 --no-check --no-pmc --steps 3 --warmup 1 > $o/kt.log 2>&1 || { tail -20 $o/kt.log; exit 1; }
python3 - $o <<'PY'
import json
import sys
d = json.loads(open(sys.argv[1] + "/bench_c5.json").read().strip().splitlines()[-1])
ex = d.get("extra", d)
for k in ("dfm_c5", "dfm_c5_f32"):
    v = ex.get(k, {})
    print(k, v.get("ms_per_pass"), v.get("kernel_ms"), (v.get("parity") or {}).get("parity"))
PY
