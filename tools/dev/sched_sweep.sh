#!/bin/bash
# usage (GPU box, repo root): tools/dev/sched_sweep.sh [bench args]   -- the default bench line under every schedule -> gpurun_out/sched/
mkdir -p gpurun_out/sched
for s in ${SCHEDS:-channels channels2 place_bank_first small}; do
  MGNNS_SCHEDULE=$s python bench.py --no-variants --no-cpu-baseline --steps 30 "$@" > gpurun_out/sched/$s.txt 2>&1
done
