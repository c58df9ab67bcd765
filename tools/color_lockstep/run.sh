#!/bin/bash
# tools/color_lockstep/run.sh -- csrc/kernels_color.hip and csrc/kernels_permute.hip executed on the host, a thread per work-item
# with real barriers (the HIP stub of tools/trsv_lockstep), under AddressSanitizer and UBSan.  The colouring under two seeds: a
# generic 257 x 257 pattern with long rows (unsorted with repeats, and sorted), a tridiagonal chain of 3000 rows, a 7-point
# stencil, 5000 rows behind 10, an arrow, cliques of 70 and 130 rows (the colour window slides), stars of 5000 leaves stored on
# both sides and in the centre only, rows of exactly 31, 32 and 33 neighbour entries, a strictly upper-triangular pattern, a
# diagonal matrix, nnz = 0, rows = 0 and 1 -- color, perm, color_ptr, colours, rounds and class sizes against the serial greedy
# colouring in descending key order.  The permutation through both routes, with and without its map, by rows, by columns, both
# and neither: rows of 0, 1, 7, 8, 9, 63, 64, 65, 4095, 4096 and 4097 entries, unsorted with repeats, rectangular shapes -- row_ptr,
# col_idx, the bits of vals, the map, then the companions and spmv_permute_vector.  Every array is an exactly sized heap block.
# Then the refusals of a bad permutation (the index in the message), and operands that were never validated (a descending
# row_ptr, columns out of range, a row_ptr beyond nnz; a perm with repeats and an inverse with entries out of range handed
# straight to the kernels): any result or refusal, no access outside the arrays and no unbounded loop.  Needs no device: a
# check of the kernels' logic and bounds, not of the GPU.  The kernel files and include/spmv_hip.h are copied beside the stubs
# so that #include "spmv_internal.hpp" finds the stub.  Takes a few minutes.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
cp -r "$here"/../trsv_lockstep/hip "$here"/spmv_internal.hpp "$here"/main.cpp "$work"/
cp "$here"/../../spmv-test_amd/csrc/kernels_color.hip "$here"/../../spmv-test_amd/csrc/kernels_permute.hip "$here"/../../spmv-test_amd/csrc/kernels_map.hip \
   "$here"/../../include/spmv_hip.h "$work"/
${CXX:-clang++} -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I"$work" -x c++ "$work"/main.cpp -o "$work"/lockstep -lpthread
"$work"/lockstep
echo "color lockstep ok"
