#!/bin/bash
# Dev tool: build a second copy of the library from the tree this script sits in, for same-box A/B runs.  The experiment lives in a
# separate working copy (e.g. `git worktree add ../exp`), never as a switch in the shipped sources:
#   ../exp/tools/dev/ab_build.sh exp        ->  ../exp/premvos_amd/csrc/libpremvos_hip_exp.so
#   PREMVOS_LIB_PATH=../exp/premvos_amd/csrc/libpremvos_hip_exp.so python tools/dev/ab_layers.py
# Further arguments go to hipcc as they are.
set -e
cd "$(dirname "$0")/../.."
TAG=$1; shift
OUT=premvos_amd/csrc/build_$TAG
mkdir -p $OUT
for f in premvos_amd/csrc/*.hip; do
  extra=$(python3 -c "import sys; sys.path.insert(0, 'premvos_amd'); import build; print(' '.join(build._file_flags(sys.argv[1])))" $f)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -Wno-unused-result $extra "$@" -c $f -o $OUT/$(basename $f).o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o premvos_amd/csrc/libpremvos_hip_$TAG.so $OUT/*.o
echo built premvos_amd/csrc/libpremvos_hip_$TAG.so
