#!/bin/bash
# GPU box: the round's bench lines (configs 2-5 with the bounded CPU baseline, the WBC HoQp bench) into
# $OUT/bench/ (OUT: LMPC_OUT, default out), each step under its own limit, stopping at the first failure
OUT=${LMPC_OUT:-out}
mkdir -p $OUT/bench
for c in 2 3 4 5; do
  steps=20; [ $c = 4 ] && steps=5; [ $c = 3 ] && steps=10; [ $c = 5 ] && steps=10
  timeout -k 10 300 python bench.py --full --config $c --steps $steps --warmup 3 > $OUT/bench/bench_c$c.json 2> $OUT/bench/bench_c$c.err || { echo "config $c failed"; tail -n 20 $OUT/bench/bench_c$c.err; exit 1; }
  echo "config $c: $(python -c "import json; d=json.load(open('$OUT/bench/bench_c$c.json')); print(round(d['ms_per_step'],4), 'ms', '%.3e QP/s' % d['value'], 'frac', round(d['roofline']['frac'],4), d['roofline'].get('frac_source'))")"
done
timeout -k 10 300 python tools/bench_hoqp.py > $OUT/bench/bench_hoqp.json 2> $OUT/bench/bench_hoqp.err || { tail -n 20 $OUT/bench/bench_hoqp.err; exit 1; }
tail -c 600 $OUT/bench/bench_hoqp.json
