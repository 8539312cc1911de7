#!/bin/bash
# Builds the standalone HIP probes of tools/ (NOT part of the product) into tools/build/ (git-ignored; travels to the GPU box).
#   bash tools/build_probes.sh [skeleton_floor deferred_reset_probe ...]
cd "$(dirname "$0")/.."
mkdir -p tools/build
# the product's flags (gym.net_amd/build.py FLAGS).  PRELOAD is kept apart: launch_floor_probe compiles one of its units without it.
BASE="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize"
PRELOAD="-mllvm -amdgpu-kernarg-preload-count=14"
for P in ${@:-skeleton_floor deferred_reset_probe store_flavour_probe}; do
  [ "$P" = sc1_store_probe ] && continue
  [ "$P" = launch_floor_probe ] && continue
  /opt/rocm/bin/hipcc $BASE $PRELOAD tools/$P.hip -o tools/build/$P &
done
wait
# the shipped CartPole kernel with its non-temporal 16-byte stores as shipped / written through (profiles/store_flavour_r05.txt)
if [ $# -eq 0 ] || [[ " $* " == *" sc1_store_probe "* ]]; then
  /opt/rocm/bin/hipcc $BASE $PRELOAD tools/sc1_store_probe.hip -o tools/build/sc1_store_probe_nt &
  /opt/rocm/bin/hipcc $BASE $PRELOAD -DGYMNET_PROBE_STORE_SC1 tools/sc1_store_probe.hip -o tools/build/sc1_store_probe_sc1 &
  wait
fi
# the launch-floor probe is two units of ONE source: the main one WITHOUT the preload flag (variants a, b, d), the unit of variants (c)
# and (e) WITH it.  The preload length of every probe kernel, read from the assembly, goes to tools/build/launch_floor_probe.preload.txt.
if [[ " $* " == *" launch_floor_probe "* ]]; then
  O=tools/build/obj_launch_floor
  mkdir -p $O
  /opt/rocm/bin/hipcc $BASE -c tools/launch_floor_probe.hip -o $O/main.o &
  /opt/rocm/bin/hipcc $BASE $PRELOAD -DLAUNCH_FLOOR_PRELOAD_UNIT -c tools/launch_floor_probe.hip -o $O/preload.o &
  /opt/rocm/bin/hipcc $BASE --cuda-device-only -S tools/launch_floor_probe.hip -o $O/main.s &
  /opt/rocm/bin/hipcc $BASE $PRELOAD -DLAUNCH_FLOOR_PRELOAD_UNIT --cuda-device-only -S tools/launch_floor_probe.hip -o $O/preload.s &
  wait
  /opt/rocm/bin/hipcc --offload-arch=gfx950 $O/main.o $O/preload.o -o tools/build/launch_floor_probe
  grep -h -E "^\s*\.amdhsa_kernel |amdhsa_user_sgpr_kernarg_preload_length|amdhsa_user_sgpr_count" $O/main.s $O/preload.s \
    | sed -E 's/^\s+//' > tools/build/launch_floor_probe.preload.txt
  rm -rf $O
  cat tools/build/launch_floor_probe.preload.txt
fi
ls -la tools/build
