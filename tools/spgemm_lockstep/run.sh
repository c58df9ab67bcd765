#!/bin/bash
# tools/spgemm_lockstep/run.sh -- csrc/kernels_spgemm.hip executed on the host, a thread per work-item, the lanes of a
# wavefront in lockstep at every ballot, shuffle and wave barrier, under AddressSanitizer and UBSan: the generic case (257 x 193
# times 193 x 300, unsorted rows with repeated columns, values spread over 2^20), a row block, a == b, rows with T - 1, T and
# T + 1 terms and distinct columns around every class of SPMV_SPGEMM_CLASS_SLOTS (the full table among them), one result column
# under a row of 600 entries with and without repeats in B, an oversized row of 44 800 distinct columns and one of 44 800 terms
# on 192 columns, 2^31 - 1 columns, m = 0, n = 0, p = 0, nnz = 0 on either side, the special values and a cancelling pair --
# every array and the LDS of every launch an exactly sized heap block, against a serial statement of the contract: row_ptr,
# col_idx and the bits of vals from the first call, and the bits of vals again from the numeric pass alone after the operands'
# values were rewritten.  Not here: the refusal at 2^31 result entries (65 536 sorts of 32 768 words).  Needs no device: a check
# of the kernels' logic and bounds, not of the GPU.  The kernel file and include/spmv_hip.h are copied beside the stubs so that
# #include "spmv_internal.hpp" finds the stub.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
cp -r "$here"/hip "$here"/spmv_internal.hpp "$here"/main.cpp "$work"/
cp "$here"/../../spmv-test_amd/csrc/kernels_spgemm.hip "$here"/../../include/spmv_hip.h "$work"/
${CXX:-clang++} -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I"$work" -x c++ "$work"/main.cpp -o "$work"/lockstep -lpthread
"$work"/lockstep
echo "spgemm lockstep ok"
