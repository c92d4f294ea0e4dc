#!/bin/bash
# quick GPU check of a kernel change: the GPU tests, then the default bench workload without the CPU legs
cd "$(dirname "$0")/.."; mkdir -p results; export TMPDIR=/tmp
TAG=${1:-quick}
(timeout 1500 python -m pytest tests -m gpu -x -q 2>&1 | tail -8) > results/${TAG}_tests.log
timeout 600 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-overlap-run --no-extra-configs > results/${TAG}_bench.json 2> results/${TAG}_bench.err
cat results/${TAG}_tests.log; cut -c1-1500 results/${TAG}_bench.json
