#!/bin/bash
# tools/ilu0_lockstep/run.sh -- csrc/kernels_ilu0.hip executed on the host, a thread per work-item with real barriers (the HIP
# stub of tools/trsv_lockstep), under AddressSanitizer and UBSan: the generic case (257 x 257, long rows fed by short and by long
# rows), a NaN, an Inf, -0 and a subnormal in A, a diagonal matrix and a tridiagonal chain of 3000 rows (across the cap of levels
# per launch), 5000 rows behind 10, level sizes around thin_rows = 70, a 7-point stencil, an arrow, stored row lengths 1 .. 129
# and 5000 in grid launches and in one workgroup, a zero pivot, rows = 0 and 1 -- several thin thresholds, every array an exactly
# sized heap block, against a serial statement of the contract: the bits of M, the pivot word, the launches, through
# spmv_csr_ilu0's path and again through ilu0_values.  Then the refusals (an unsorted row, a repeated column, a missing
# diagonal), and operands that were never validated handed straight to the kernels (a descending row_ptr, columns out of range,
# a row_ptr beyond nnz, unsorted rows): any result, no access outside the arrays and no unbounded loop.  order, level_ptr and
# the diagonal's positions are built serially on the host.  Needs no device: a check of the kernels' logic and bounds, not of
# the GPU.  The kernel file and include/spmv_hip.h are copied beside the stubs so that #include "spmv_internal.hpp" finds the
# stub.  Takes a minute or two (3000 levels of barriers under the sanitizers).
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
cp -r "$here"/../trsv_lockstep/hip "$here"/spmv_internal.hpp "$here"/main.cpp "$work"/
cp "$here"/../../spmv-test_amd/csrc/kernels_ilu0.hip "$here"/../../include/spmv_hip.h "$work"/
${CXX:-clang++} -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I"$work" -x c++ "$work"/main.cpp -o "$work"/lockstep -lpthread
"$work"/lockstep
echo "ilu0 lockstep ok"
