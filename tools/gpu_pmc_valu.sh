#!/bin/bash
cd "$(dirname "$0")/.."; mkdir -p results; export TMPDIR=/tmp
C1="SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS"
timeout 600 rocprofv3 --pmc $C1 -d results/pv -o p -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-overlap-run --no-extra-configs > results/pv.log 2>&1
python tools/rocpd_pmc.py $(ls results/pv/*.db | head -1) > results/r2_pmc_valu.txt 2>&1
rm -rf results/pv
grep -A9 "k_linearise_schur\|k_backsub\|k_reduced_solve" results/r2_pmc_valu.txt
