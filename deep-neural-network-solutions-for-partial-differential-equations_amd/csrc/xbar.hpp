// Input cotangent of net_u (dbsde_net_u_xvjp):
//
//   xbar[R, D] = (Alpha[0:R, 0:K] . W)[:, 1..D],   W = the stacked input-facing
//                                                  weights [K, Dp] (K = Stot_x)
//
// the contraction that forms Z from Delta (gemm_z, phase A's "Z += delta_j V_j"
// stages) with phase C's reverse cotangents alpha_j in place of delta_j:
// d/dX [ubar u + zbar . Du] = ubar Du + H zbar, both terms inside alpha.
#pragma once
#include <hip/hip_runtime.h>

namespace dbsde {

struct XbarArgs {
  const float* Alpha;   // [>= R, lda] row-major, columns [0, K) read
  int lda;
  const float* Wt;      // W^T: [Dp, K] row-major fp32 (the BtZ pack), zero in the padding
  int K;                // multiple of 16
  int Dp;               // multiple of 16, <= 1024 (above 128: output blocks in passes of 8)
  int R, D;             // valid rows, state dimension (D + 1 <= Dp)
  float* xbar;          // [R, D] dense
};

// One launch on stream s; -1 for a geometry the kernel does not cover (launch
// errors are left for hipGetLastError).
__attribute__((visibility("hidden"))) int netu_xbar_launch(const XbarArgs& a, hipStream_t s);

}  // namespace dbsde
