#!/bin/bash
# tools/select_lockstep/run.sh -- csrc/kernels_select.hip executed on the host, a thread per work-item, the lanes of a
# wavefront in lockstep at every ballot and shuffle, under AddressSanitizer and UBSan: top-k and threshold selections on rows of
# 0 .. 4097 nonzeros (mixed inside a wavefront and sorted by length, plain and shuffled with repeated columns), ties (all
# equal, two values, blocks of 64 and of 65), the special scores (NaN payloads, +-Inf, +-0, subnormals, +-FLT_MAX) with and
# without SPMV_SELECT_ABS, rows of only NaNs, rows = 0 and nnz = 0, every array an exactly sized heap block, against a serial
# statement of the contract: row_ptr, col_idx, the bits of vals and the map bit for bit, then gather and scatter through the
# map (csrc/kernels_map.hip).  Needs no device: a check of the kernels' logic and bounds, not of the GPU.  The kernel files, lane_group.hpp and
# attention_args.hpp are copied beside the stubs so that their #include "spmv_internal.hpp" finds the stub.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
cp -r "$here"/hip "$here"/spmv_internal.hpp "$here"/main.cpp "$work"/
cp "$here"/../../spmv-test_amd/csrc/kernels_select.hip "$here"/../../spmv-test_amd/csrc/kernels_map.hip "$here"/../../spmv-test_amd/csrc/lane_group.hpp \
   "$here"/../../spmv-test_amd/csrc/attention_args.hpp "$work"/
${CXX:-clang++} -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I"$work" -x c++ "$work"/main.cpp -o "$work"/lockstep -lpthread
"$work"/lockstep
echo "select lockstep ok"
