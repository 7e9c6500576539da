#!/bin/bash
set -o pipefail
# serial / in-flight frame times of the triangle configurations (development: tile order)
OUT=${OUT:-results/r03}
mkdir -p $OUT
for cfg in REF TRI TRI4K; do
  echo "== $cfg" >> $OUT/tri_order2.log
  timeout -k 10 300 python bench.py --full --config $cfg --no-cpu-baseline --steps 200 --warmup 10 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('in flight %.4f serial %s check %s' % (d['ms_per_step'], d.get('serial_ms_per_step'), d.get('frame_check')))" >> $OUT/tri_order2.log || exit 1
done
cat $OUT/tri_order2.log
