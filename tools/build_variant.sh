#!/bin/bash
# Build an experimental kernel variant next to the default library (git-ignored):
#   tools/build_variant.sh stepprof -DMJ_STEP_PROF   -> mortal_amd/libmortal_amd_stepprof.so   (a tag + extra hipcc flags)
# A/B it with   MORTAL_AMD_LIB=mortal_amd/libmortal_amd_stepprof.so python bench.py ...   (interleave the two builds inside one run)
set -e
cd "$(dirname "$0")/.."
tag=$1
shift
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off -Wno-unused-value \
    "$@" -o mortal_amd/libmortal_amd_$tag.so mortal_amd/csrc/mj_capi.hip
ls -la mortal_amd/libmortal_amd_$tag.so
