#!/bin/bash
# Builds a PROBE variant of the library (same sources, extra -D flags) into tools/build/libgymnet_amd_<name>.so for A/B runs on one box:
#   GYMNET_LIB_PATH=tools/build/libgymnet_amd_<name>.so python3 tools/...      (tools/build/ is git-ignored and travels to the GPU box)
#   bash tools/build_probe_lib.sh masked -DGYMNET_PROBE_RESET_MASKED
cd "$(dirname "$0")/.."
NAME=$1; shift
mkdir -p tools/build/obj_$NAME
# the product's translation units and compile flags: gym.net_amd/build.py is the one place that names them
UNITS=$(python3 -c "import sys; sys.path.insert(0, 'gym.net_amd'); import build; print(' '.join(s[:-4] for s in build.SOURCES))")
FLAGS=$(python3 -c "import sys; sys.path.insert(0, 'gym.net_amd'); import build; print(' '.join(f for f in build.FLAGS if f != '-shared'))")
for S in $UNITS; do
  /opt/rocm/bin/hipcc $FLAGS "$@" -c gym.net_amd/csrc/$S.hip -o tools/build/obj_$NAME/$S.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared tools/build/obj_$NAME/*.o -ldl -o tools/build/libgymnet_amd_$NAME.so && rm -rf tools/build/obj_$NAME
ls -la tools/build/libgymnet_amd_$NAME.so
