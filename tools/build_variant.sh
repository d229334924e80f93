#!/bin/bash
# Kernel tuning aid: build the HIP library with extra -D flags into gpurun_out/variants/<name>.so
# usage: tools/build_variant.sh <name> [-DFOO=1 ...]   (run with TD_HIP_LIB=gpurun_out/variants/<name>.so)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
mkdir -p $R/variants
C=$R/tokendagger_amd/csrc
# (every source of the library, as build_hip() in __graft_entry__.py takes them: all of csrc/ but the pybind module)
srcs=$(ls $C/*.hip $C/*.cpp | grep -v '/py_binding\.cpp$')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wno-unused-function "$@" \
  $srcs -I$R/include -ldl -o $R/variants/$name.so
echo built $R/variants/$name.so
