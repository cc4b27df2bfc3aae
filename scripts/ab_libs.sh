#!/bin/bash
# A/B of library builds on one box, alternating, same session (run on the GPU box):
#   bash scripts/ab_libs.sh "<perf_sweeps.py arguments>" <rounds> lib1.so lib2.so ...
# prints one perf_sweeps.py line per library and round (minimum of three sweeps each).
# Libraries are builds of THIS tree (krotov_amd/_lib.py binds every symbol of include/krotov_hip.h), e.g. the q2
# kernels' two lane maps:
#   python -c "from krotov_amd import build; build.build(extra_flags=['-DKH_Q2_LDS_BROADCAST'], out='/tmp/q2_lds.so')"
#   bash scripts/ab_libs.sh "256 64 4001 1" 5 /tmp/q2_lds.so krotov_amd/libkrotov_hip.so
ARGS=${1:-"256 64 4001 1"}; ROUNDS=${2:-3}; shift 2
R=${GRAFT_REPO_ROOT:-$(pwd)}
for r in $(seq $ROUNDS); do
  for lib in "$@"; do
    case $lib in /*) path=$lib ;; *) path=$R/$lib ;; esac
    echo -n "$(basename $lib) | "
    KH_LIB=$path python $R/scripts/perf_sweeps.py $ARGS 2>&1 | grep -v amdgpu.ids | head -1
  done
done
