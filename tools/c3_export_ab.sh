#!/bin/bash
# Runs on the GPU box: C3 (bench.py --no-extra --no-cpu-baseline) with the regular library and any tagged library named in EXTRA="tag=path ..."
# (e.g. the parent commit's), twice each, interleaved, then once with the stamping build of tools/c3_export_build.sh; prints us per iteration,
# launch time, iteration count and the phase stamps (the st build: "allgather" / "update" are the times from the iteration's start to the export
# stores issued / to the first entry step of phase 0 multiplied, kernels_persist.h FDAPDE_STAMP_EXPORT).  Every run has a time limit of its own;
# the first failure ends the script.
set -euo pipefail
REPO=$(pwd)
V=$REPO/tools/bin/variants
run() {   # tag, lib
  FDAPDE_HIP_LIB=$2 timeout -k 10 300 python3 bench.py --steps 10 --warmup 2 --no-extra --no-cpu-baseline 2>/dev/null | tail -1 | python3 -c "
import json,sys
d=json.loads(sys.stdin.read()); c=d['config']; r=d['roofline']; s=r['phase_stamps_us_per_iteration']
print('%-9s us/iter %.2f  launch %.3f ms  iterations %d  ms/step %.3f  value %.1f  operator mean %.2f slowest %.2f  allgather %.2f  update %.2f  relres %.4e' % ('$1', c['us_per_iteration'], r['avg_launch_ms'], c['cg_iterations'], d['ms_per_step'], d['value'], s['operator_mean'], s['operator_slowest_workgroup'], s['allgather'], s['update'], c['relres']))"
}
for rep in 1 2; do
  for kv in ${EXTRA:-}; do run ${kv%%=*} ${kv#*=}; done
  run new $REPO/fdapde-core_amd/lib/libfdapde_hip.so
done
run st $V/libfdapde_hip_st.so
