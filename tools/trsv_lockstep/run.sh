#!/bin/bash
# tools/trsv_lockstep/run.sh -- csrc/kernels_trsv.hip executed on the host, a thread per work-item with real barriers, under
# AddressSanitizer and UBSan: the generic case (257 x 257 full, unsorted rows with repeated columns, long rows), NaN and Inf in
# b, a missing and a repeated diagonal, a diagonal matrix and a bidiagonal chain of 3000 rows (across the cap of levels per
# launch), a fan of 5000 rows behind 10, level sizes around thin_rows = 70, a 7-point stencil, row lengths 0 .. 129 and 5000 in
# grid launches and in one workgroup, special values, rows = 0 and 1, nnz = 0 -- both triangles, unit and non-unit, several
# thin thresholds, every array an exactly sized heap block, against a serial statement of the contract: level_ptr, order, the
# plan's counts, the launches of a solve, the bits of x, and x again in place.  Then operands that were never validated (a
# descending row_ptr, columns out of range, a row_ptr beyond nnz, a negative one): any result or refusal, no access outside the
# arrays and no unbounded loop.  Needs no device: a check of the kernels' logic and bounds, not of the GPU.  The kernel file
# and include/spmv_hip.h are copied beside the stubs so that #include "spmv_internal.hpp" finds the stub.  Takes a minute or
# two (3000 levels of barriers under the sanitizers).
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
cp -r "$here"/hip "$here"/spmv_internal.hpp "$here"/main.cpp "$work"/
cp "$here"/../../spmv-test_amd/csrc/kernels_trsv.hip "$here"/../../include/spmv_hip.h "$work"/
${CXX:-clang++} -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I"$work" -x c++ "$work"/main.cpp -o "$work"/lockstep -lpthread
"$work"/lockstep
echo "trsv lockstep ok"
