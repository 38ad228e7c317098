#!/bin/bash
# Device assembly of one csrc file, for comparing two trees: tools/device_asm.sh FILE.hip ["-DFLAG=..."] > out.s
# build.py's flags plus --cuda-device-only -S; the lines that differ between two compiles of the same code (.file, .ident, the __hip_cuid_<hash> symbol) are dropped.
# Compare two outputs with diff or sha1sum.  Needs hipcc, no GPU.
set -e -o pipefail
FILE=$1; shift
"${HIPCC:-/opt/rocm/bin/hipcc}" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-kernarg-preload-count=8 "$@" --cuda-device-only -S "$FILE" -o - \
  | grep -v -e '^[[:space:]]*\.file[[:space:]]' -e '^[[:space:]]*\.ident[[:space:]]' -e '__hip_cuid_'
