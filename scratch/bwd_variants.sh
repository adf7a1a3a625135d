#!/bin/bash
# scratch (round 6): the backward of the few-rows big shapes under each plan switch that is left (pair128; the others are retired); prints bwd_pair / splitk / step us per shape
S=${1:-256x8192,384x8192,512x8192}
for o in "" pair128=0; do
  python bench_sweep.py ${o:+--opt $o} --shapes $S 2>/dev/null | python -c "
import sys, json
for l in sys.stdin:
    try: r = json.loads(l)
    except Exception: continue
    if 'B' in r: print('${o:-default}'.ljust(16), r['B'], r['Nc'], 'bwd', r['bwd_pair']['us'], 'step', r['step']['us'])
"
done
