#!/bin/bash
# Builds a variant of the library that differs in the pipelined solver only, for scans and A/B runs:
#   tools/build_pipe_variant.sh NAME [compiler flags ...]   ->  build_ab/librdis_hip_NAME.so
# e.g.  tools/build_pipe_variant.sh polls4 -DRDIS_PIPE_POLLS=4
#       tools/build_pipe_variant.sh timing -DRDIS_COOP_TIMING
# Only the two sources that include solver_pipe.hpp are compiled again; the other objects -- the kernels' translation
# units and the ABI's host-only ones (comm, plan_query) -- are those of the regular build
# (make -C rdis_amd/csrc first).  Probes pick a variant up through RDIS_PROBE_LIB.
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
name="$1"; shift
obj="$root/build_ab/obj_$name"
mkdir -p "$obj"
cd "$root/rdis_amd/csrc"
for f in rdis_hip refround_kernels; do
  "${HIPCC:-/opt/rocm/bin/hipcc}" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function "$@" -c -o "$obj/$f.o" "$f.hip" &
  pids="${pids:-} $!"
done
for p in $pids; do wait "$p"; done
others=$(ls "$root"/rdis_amd/lib/obj/*.o | grep -v -E '/(rdis_hip|refround_kernels)\.o$')
"${HIPCC:-/opt/rocm/bin/hipcc}" --offload-arch=gfx950 -shared -fPIC -o "$root/build_ab/librdis_hip_$name.so" "$obj/rdis_hip.o" "$obj/refround_kernels.o" $others
ls -la "$root/build_ab/librdis_hip_$name.so"
