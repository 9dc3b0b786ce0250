#!/bin/bash
# Default full bench (every leg, with the CPU baseline) -> $LOGS/bench_<tag>.log
LOGS=${LOGS:-logs}
mkdir -p $LOGS
export TMPDIR=/tmp
TAG=${1:-r01}
timeout -k 10 600 python bench.py --full > $LOGS/bench_$TAG.log 2>&1 || { tail -20 $LOGS/bench_$TAG.log; exit 1; }
tail -1 $LOGS/bench_$TAG.log
