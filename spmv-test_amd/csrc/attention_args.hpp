#pragma once
// attention_args.hpp -- what one fused-attention call hands from its entry point (capi.hip) to launch_attention and on to
// every kernel (kernels_attention.hip).  Needs nothing but <cstdint>: tools/attention_lockstep includes it as it stands.
#include <cstdint>

namespace spmv {

enum AttnPass { kPassForward = 0, kPassBackwardQ = 1, kPassBackwardKV = 2 };

// The element types of the matrices (Q, K, V, O, dO, dQ, dK, dV) besides float.  bf16 is its 16 bits and plain integer code
// (lane_group.hpp widens and rounds it); fp16 is the compiler's _Float16.  stats, delta and the scratch are float always.
struct bf16 {
    uint16_t bits;
};
using fp16 = _Float16;

// the operands of the three passes (a by-value kernel argument: its layout is part of the device code; a pass reads what
// it needs).  E: the element type of the matrices; every ld and every matrix stride counts elements of E.
template <typename E>
struct AttnArgsT {
    float scale;
    int k, kv;
    const E *Q;       int64_t ldq;
    const E *K;       int64_t ldk;
    const E *V;       int64_t ldv;
    const E *O;       int64_t ldo;     // backward_q
    const E *dO;      int64_t lddo;    // backward
    const float *stats_in;             // backward
    const float *delta_in;             // backward_kv
    E *out0;          int64_t ld0;     // forward O; backward_q dQ; backward_kv dK
    E *out1;          int64_t ld1;     // backward_kv dV
    float *stats;                      // forward
    float *delta;                      // backward_q
    // elements (stats, delta: floats) from head y to head y + 1 of every operand above (all 0 in a call of one head); hk, hv
    // (and in backward_kv h0, h1): from one K/V head to the next
    int64_t hq, hk, hv, ho, hdo, hstats_in, hdelta_in, h0, h1, hstats, hdelta;
};
using AttnArgs = AttnArgsT<float>;     // the nine fp32 entry points

// The additive bias of the _bias entry points: a second by-value argument of the biased kernels only, so that AttnArgsT (and
// with it the kernarg segment of every unbiased kernel) stays as it is.  Floats whatever E is, nnz of them per query head in
// the storage order of the handle the call runs on (backward_kv: the transposed handle's).
struct AttnBias {
    const float *bias;    int64_t hbias;      // floats from query head y to y + 1; 0: one bias for all heads
    float *dbias;         int64_t hdbias;     // backward_q: p (dp - delta) per nonzero and query head; null: not written
};

}  // namespace spmv
