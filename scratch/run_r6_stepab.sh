#!/bin/bash
# round 6: the training step with the block-resident mean-field forward on / off (two interleaved runs each)
cd $GRAFT_REPO_ROOT
tag=${1:-r6stepab}
res=${OUT_ROOT:-scratch/out}/$tag      # OUT_ROOT: where the runs write, relative to the repository root
mkdir -p $res
for i in 1 2; do
for mode in off auto; do
CRFCONV_MF_BLOCK=$mode timeout -k 10 300 python3 bench.py --full --no-cpu-baseline --no-other-configs --steps 40 > $res/bench_$mode$i.json 2> $res/bench_$mode$i.err || { echo "bench $mode failed"; tail -5 $res/bench_$mode$i.err | cut -c1-300; }
python3 -c "
import json; r=json.load(open('$res/bench_$mode$i.json')); print('$mode: ms_per_step %.4f  value %.2f  mf fwd %.2f us (frac %.3f)  layer fwd %s' % (r['ms_per_step'], r['value'], r['roofline']['avg_launch_us'], r['roofline']['frac'], r.get('roofline_layer', {}).get('fwd_us')))"
done
done
