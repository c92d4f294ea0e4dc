#!/bin/bash
# per-launch durations of the sweeps over the ten LM iterations of a bench step, with and without the kept-Jacobian replay
cd "$(dirname "$0")/.."; mkdir -p results; export TMPDIR=/tmp
TAG=${1:-keeptrace}
: > results/${TAG}.txt
for KEEP in 1 0; do
  BENCH="python bench.py --full --eager --steps 3 --warmup 0 --profile-steps 0 --keep-jacobian $KEEP ${BENCH_ARGS} --no-cpu-baseline --no-overlap-run --no-extra-configs --no-result-check"
  timeout 900 rocprofv3 --kernel-trace --stats -d results/${TAG}_kt$KEEP -o t -- $BENCH > results/${TAG}_kt$KEEP.log 2>&1
  echo "== lba_keep_jacobian $KEEP" >> results/${TAG}.txt
  python tools/rocpd_sequence.py $(ls results/${TAG}_kt$KEEP/*.db | head -1) >> results/${TAG}.txt 2>&1
  rm -rf results/${TAG}_kt$KEEP
done
cat results/${TAG}.txt
