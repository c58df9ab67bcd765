#!/bin/bash
# tools/add_lockstep/run.sh -- csrc/kernels_add.hip executed on the host, a thread per work-item, under AddressSanitizer and
# UBSan: the generic case (two 257 x 193 matrices, unsorted rows with repeated columns: the route through the row-sorted view),
# sorted operands with and without repeated columns, a row block, a == b, row lengths 0 .. 129 against 0, 1, 64 and a row of
# 5000, identical / disjoint / interleaved rows, columns up to 2^31 - 2, m = 0, n = 0, nnz = 0 on either side and both, an empty
# intersection, the special values, a cancelling pair and coefficients of +0, -0, NaN and Inf -- all three ops each, every array
# an exactly sized heap block, against a serial statement of the contract: row_ptr, col_idx, the bits of vals and the plan's
# two arrays from the first call, the bits of vals again from spmv_csr_add_values after the operands' values were rewritten,
# and spmv_csr_add_gather on a poisoned target.  Then operands that were never validated (a descending row_ptr, a column out
# of range, a row_ptr beyond nnz): any result or refusal, no access outside the arrays.  Not here: the refusal at 2^31 result
# entries (16 GiB of operands).  Needs no device: a check of the kernels' logic and bounds, not of the GPU.  The kernel file and
# include/spmv_hip.h are copied beside the stubs so that #include "spmv_internal.hpp" finds the stub.  Takes some minutes (rows
# of 5000 entries under the sanitizers).
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
cp -r "$here"/hip "$here"/spmv_internal.hpp "$here"/main.cpp "$work"/
cp "$here"/../../spmv-test_amd/csrc/kernels_add.hip "$here"/../../include/spmv_hip.h "$work"/
${CXX:-clang++} -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I"$work" -x c++ "$work"/main.cpp -o "$work"/lockstep -lpthread
"$work"/lockstep
echo "add lockstep ok"
