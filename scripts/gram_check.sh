#!/bin/bash
# GPU box: Gram parity tests, Gram timings, and the full bench line (every leg).
set -e
O=${OUT_DIR:-bench_out/gram}
mkdir -p $O
timeout -k 10 300 python3 -u -m pytest tests/test_gpu_parity.py -k gram -x -q --timeout 120 --timeout-method thread > $O/tests.log 2>&1
timeout -k 10 120 python3 -u scripts/gram_probe.py 100 19,64,128,256,512 > $O/probe.log 2>&1
timeout -k 10 120 python3 -u scripts/gram_probe.py 316 64,128,256 >> $O/probe.log 2>&1
timeout -k 10 600 python3 -u bench.py --full > $O/bench.log 2>&1
tail -2 $O/tests.log
cat $O/probe.log
