#!/bin/bash
REPO=$(cd "$(dirname "$0")/.." && pwd)
# round 6: the whole GPU tier + smoke + the default bench line.  usage: bash tools/gpu_r6_check.sh <tag> [pytest args]
TAG=${1:-r06a}; shift
cd "$REPO" || exit 1
mkdir -p bench_out
( timeout 3000 python -m pytest tests -m gpu -q -x "$@" 2>&1 | tail -25 ) > bench_out/${TAG}_tests.log 2>&1
tail -8 bench_out/${TAG}_tests.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
( time timeout 1200 python bench.py --full ) > bench_out/${TAG}_bench_default.json 2> bench_out/${TAG}_bench_default.err
tail -3 bench_out/${TAG}_bench_default.err
python - bench_out/${TAG}_bench_default.json <<'PY'
import json,sys
d=json.loads(open(sys.argv[1]).read().strip().split('\n')[-1])
print({k:d.get(k) for k in ("value","ms_per_step","sequential","roofline","single_scan_latency_ms","kernel_ms_per_step")})
print("q_pipe", d.get("q_pipe"))
PY
