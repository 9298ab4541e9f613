#!/bin/bash
# GPU box: config-2 evidence after a dense-path change -- rocprof/PMC passes (tools/profile_round.sh 2), the bench
# line with the bounded CPU baseline, and the dense phase stamps; each step under its own limit.  Output under $OUT
# (LMPC_OUT, default out).
OUT=${LMPC_OUT:-out}
mkdir -p $OUT/bench $OUT/st
tools/profile_round.sh 2 > $OUT/prof_c2.log 2>&1 || { tail -20 $OUT/prof_c2.log; exit 1; }
timeout -k 10 300 python bench.py --full --config 2 --steps 20 --warmup 3 > $OUT/bench/bench_c2.json 2> $OUT/bench/bench_c2.err || exit 2
cat $OUT/bench/bench_c2.json
LMPC_STAMPS_OUT=$OUT/st/dense_stamps.npz LMPC_STAMPS_LIB=tools/build/liblmpc_stamps.so timeout -k 10 200 python -u tools/dense_check.py stamps > $OUT/st/dense_stamps.log 2>&1 || exit 3
grep -A4 "max cycles" $OUT/st/dense_stamps.log
