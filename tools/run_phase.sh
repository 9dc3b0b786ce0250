#!/bin/bash
# GPU: phase-kernel parity, full gpu suite, full bench with the phase roofline leg.
LOGS=${LOGS:-logs}
mkdir -p $LOGS
export TMPDIR=/tmp
timeout -k 10 300 python -m pytest tests/test_gpu_phases.py -q -p no:cacheprovider > $LOGS/pytest_phases.log 2>&1
rc=$?; tail -30 $LOGS/pytest_phases.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 600 python -m pytest tests -m gpu -q -p no:cacheprovider > $LOGS/pytest_gpu.log 2>&1
rc2=$?; tail -5 $LOGS/pytest_gpu.log
if [ $rc2 -ne 0 ] && [ $rc2 -ne 1 ]; then exit $rc2; fi
timeout -k 10 300 python bench.py --steps 500 --warmup 50 --full --no-cpu-baseline > $LOGS/bench_phase.log 2>&1 || exit $?
tail -1 $LOGS/bench_phase.log
