#!/bin/bash
# Ant env-step throughput vs batch size (waves per SIMD) -> $LOGS/batch_scan.log
LOGS=${LOGS:-logs}
mkdir -p $LOGS
export TMPDIR=/tmp
for b in 4096 8192 16384 32768; do
  timeout -k 10 120 python bench.py --batch $b --steps 300 --warmup 30 --full --no-cpu-baseline --no-phases --no-secondary > $LOGS/scan_$b.json 2> $LOGS/scan_$b.err || { tail -5 $LOGS/scan_$b.err; exit 1; }
  python -c "import json;d=json.load(open('$LOGS/scan_$b.json'));print($b, round(d['value']/1e6,2), 'M/s kernel_ms', round(d['roofline']['kernel_ms'],4))" | tee -a $LOGS/batch_scan.log
done
