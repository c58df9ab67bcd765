#pragma once
// attention_args.hpp -- what one fused-attention call hands from its entry point (capi.hip) to launch_attention and on to
// every kernel (kernels_attention.hip).  Needs nothing but <cstdint>: tools/attention_lockstep includes it as it stands.
#include <cstdint>

namespace spmv {

enum AttnPass { kPassForward = 0, kPassBackwardQ = 1, kPassBackwardKV = 2 };

// the operands of the three passes (a by-value kernel argument: its layout is part of the device code; a pass reads what
// it needs)
struct AttnArgs {
    float scale;
    int k, kv;
    const float *Q;   int64_t ldq;
    const float *K;   int64_t ldk;
    const float *V;   int64_t ldv;
    const float *O;   int64_t ldo;     // backward_q
    const float *dO;  int64_t lddo;    // backward
    const float *stats_in;             // backward
    const float *delta_in;             // backward_kv
    float *out0;      int64_t ld0;     // forward O; backward_q dQ; backward_kv dK
    float *out1;      int64_t ld1;     // backward_kv dV
    float *stats;                      // forward
    float *delta;                      // backward_q
    // floats from head y to head y + 1 of every operand above (all 0 in a call of one head); hk, hv (and in backward_kv h0,
    // h1): from one K/V head to the next
    int64_t hq, hk, hv, ho, hdo, hstats_in, hdelta_in, h0, h1, hstats, hdelta;
};

}  // namespace spmv
