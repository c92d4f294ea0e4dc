#!/bin/bash
# the whole GPU test-suite, then the default bench line (what the driver runs)
cd "$(dirname "$0")/.."; mkdir -p results; export TMPDIR=/tmp
TAG=${1:-full}
timeout 2400 python -m pytest tests -x -q -m gpu > results/${TAG}_gputests.log 2>&1; echo "pytest rc $?" >> results/${TAG}_gputests.log
tail -n 6 results/${TAG}_gputests.log
timeout 900 python bench.py --full > results/${TAG}_bench.json 2> results/${TAG}_bench.err; echo "bench rc $?"
python - results/${TAG}_bench.json <<'PY'
import json,sys
d=json.load(open(sys.argv[1]))
print({k: d[k] for k in ("value","ms_per_step","kernel_ms_per_step") if k in d})
print("roofline", d.get("roofline")); print("backsub", d.get("roofline_backsub")); print("traj", d.get("traj_error_vs_oracle")); print("results_check", d.get("results_check"))
PY
