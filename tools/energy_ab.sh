#!/bin/bash
# Energy / clock A/B on the headline step: the socket sits at its power cap, so a variant that moves less data can win through the
# clock it leaves room for even when isolated kernel timings are neutral.  default | serial towers; prints ms/step, sclk, socket power, J/step per
# pass (interleaved passes).  (The banded-tile-order and 128^2-for-small-launches variants of profiles/r04_energy_ab.txt were environment knobs of the
# GEMM dispatcher, removed with the numbers kept: EXPERIMENTS.md 7c.)   usage (GPU box): bash tools/energy_ab.sh [passes]
R=$GRAFT_REPO_ROOT
P=${1:-2}
run() {  # label, env assignments...
    local label=$1; shift
    env "$@" python $R/bench.py --full --steps 20 --warmup 5 --cpu-pairs 0 --no-vendor-comparator --no-other-configs --no-roofline-events 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.read()); c = d['clock'] or {}
print('%-34s %8.3f ms/step %8.1f pairs/s  sclk %5s MHz  %7s W  %6s J/step' % ('$label', d['ms_per_step'], d['value'], c.get('sclk_mhz_under_load'), c.get('socket_power_w'), c.get('joules_per_step')))"
}
for i in $(seq $P); do
    run "default" SC_NOP=1
    run "SC_OVERLAP_VIT=0 (serial towers)" SC_OVERLAP_VIT=0
done
