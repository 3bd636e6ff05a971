#!/bin/bash
# helper used during development on the GPU box: bench sweep over lambda for split/fused variants
# usage: tools/bench_sweep.sh <outdir>
out=$1
mkdir -p $out
for lam in 1e-3 1e-11; do
  timeout -k 10 100 python bench.py --full --no-cpu-baseline --lam $lam > $out/bench_split_$lam.json 2>> $out/bench.err
  python -c "import json,sys; d=json.load(open('$out/bench_split_$lam.json')); k=list(d['roofline']['kernels'].values()); print('split lam=$lam', round(d['value']), 'img/s', round(d['ms_per_step']*1000,1), 'us/step fwd', round(k[0]['avg_launch_us'],1), 'bwd', round(k[1]['avg_launch_us'],1))"
  timeout -k 10 100 python bench.py --full --no-cpu-baseline --variant fused --lam $lam > $out/bench_fused_$lam.json 2>> $out/bench.err
  python -c "import json,sys; d=json.load(open('$out/bench_fused_$lam.json')); r=d['roofline']; print('fused lam=$lam', round(d['value']), 'img/s', round(d['ms_per_step']*1000,1), 'us/step', round(r['achieved']), 'GB/s')"
done
