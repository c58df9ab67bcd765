#!/bin/bash
# tools/attention_lockstep/run.sh -- csrc/kernels_attention.hip executed on the host, a thread per work-item, the lanes of a
# group in lockstep at every shuffle, under AddressSanitizer and UBSan: forward, backward_q and backward_kv at four (k, kv)
# on both load paths, rows and pieces on the pattern (a third of its rows unsorted, a fifth drawn with
# replacement so that keys repeat) and on its transpose, every array an exactly sized heap block, against
# a serial fp64 statement of attention (2e-5 of the magnitude); and csrc/kernels_sddmm.hip, built from the same
# csrc/lane_group.hpp, at the same four k on the same patterns, every out[n] bit for bit against a serial statement of the
# documented order; and three heads in one launch (the head in blockIdx.z) at the same (k, kv) and load paths, stacked and as
# column blocks, on a scratch of exactly three heads, every head bit for bit the single-head run; and four grouped-query heads
# on two K/V heads (the head within its group in blockIdx.y, the K/V head in blockIdx.z; backward_kv's sum over the heads of a
# group in k_attn_bwd_kv_rows_gqa and k_attn_add_pieces_gqa) bit for bit the single-head runs folded in head order; and the
# same four heads on 16-bit matrices (bf16 and fp16, exactly sized blocks of 2-byte elements, the 8-byte and the 2-byte load path)
# bit for bit the fp32 runs on the widened data, rounded to nearest even; and the kernels with a bias (<..., AttnBias>; fp32 and bf16, (6, 10) and
# (40, 64), both load paths, four query heads on two K/V heads, bias, bias_t and dBias exactly sized blocks, rows in pieces on
# the pattern and on its transpose) against a serial fp64 attention with bias; and the V = 32 kernels of the _wide entry points
# ((128, 128) and (65, 100), fp32 and bf16, both load paths, with and without a bias, the same four heads, rows in pieces on both
# handles, every matrix and the wide scratch of 260 floats per piece an exactly sized block) against the same serial fp64
# attention, and their zero-padding property: operands of (64, 20), (8, 40) and (16, 12) padded to (128, 128) give the narrow
# run's delta, dBias, dQ, dK and dV bit for bit and +0 in the padded columns.  Needs no device: a check of the kernels' logic, bounds and alignment, not of the GPU.  The kernel
# files, lane_group.hpp and attention_args.hpp are copied beside the stubs so that their #include "spmv_internal.hpp" finds the stub.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
cp -r "$here"/hip "$here"/spmv_internal.hpp "$here"/main.cpp "$work"/
cp "$here"/../../spmv-test_amd/csrc/kernels_attention.hip "$here"/../../spmv-test_amd/csrc/kernels_sddmm.hip \
   "$here"/../../spmv-test_amd/csrc/lane_group.hpp "$here"/../../spmv-test_amd/csrc/attention_args.hpp "$work"/
${CXX:-clang++} -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I"$work" -x c++ "$work"/main.cpp -o "$work"/lockstep -lpthread
"$work"/lockstep
echo "lockstep ok"
