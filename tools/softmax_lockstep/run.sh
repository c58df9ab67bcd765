#!/bin/bash
# tools/softmax_lockstep/run.sh -- csrc/kernels_softmax.hip executed on the host, the 64 lanes of a wavefront in lockstep,
# under AddressSanitizer and UBSan, against a serial statement of the documented order of the sums (bit for bit; forward
# out of place and in place with masked entries, backward on integers out of place, over P and over dP).  Needs no device:
# a check of the kernels' logic and bounds, not of the GPU.  The kernel file and csrc/lane_group.hpp are copied beside the
# stubs so that their #include "spmv_internal.hpp" finds the stub.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
cp -r "$here"/hip "$here"/spmv_internal.hpp "$here"/main.cpp "$work"/
cp "$here"/../../spmv-test_amd/csrc/kernels_softmax.hip "$here"/../../spmv-test_amd/csrc/lane_group.hpp "$work"/
${CXX:-clang++} -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I"$work" -x c++ "$work"/main.cpp -o "$work"/lockstep -lpthread
for layout in 0 1 2 3 4; do "$work"/lockstep $layout; done
echo "lockstep ok"
