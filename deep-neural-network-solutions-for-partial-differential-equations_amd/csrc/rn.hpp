// rn.hpp -- individually rounded fp32 operations for the Euler path step
// (shared by the rollout kernels of paths.hpp and the Monte-Carlo comparator
// of mc.hip).
//
// HIP contracts a*b + c into an FMA by default (-ffp-contract=fast), and its
// __fmul_rn/__fadd_rn are plain operators whose contract flag comes from the
// header that defines them, so a pragma at the call site does not stop the
// fusion.  rn_mul/rn_add/rn_sub below carry no contract flag: the reference
// (torch CPU) rounds each product and sum, and X is bit-exact against it.
#pragma once
#include <hip/hip_runtime.h>

namespace dbsde {

__device__ __forceinline__ float rn_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float rn_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float rn_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

// the reference's clamp of the Heston drift and diffusion entries
__device__ __forceinline__ float clamp100(float v) { return fminf(fmaxf(v, -100.f), 100.f); }

// One Euler step of one asset of the two-factor Heston model
// (DBSDE_PROB_HESTON2, include/dbsde.h; paths.hpp rollout_heston2_kernel and
// mc.hip), w1 / w2 the increments of W^S and W^v, rhob = fp32(sqrt(1 - rho^2)):
//   S <- (S + c(mu_a S) dt) + a,   a = c(sv S) w1
//   v <- (v + c(kappa (theta - v)) dt) + b,   b = c(rho (sig sv)) w1 + c(rhob (sig sv)) w2
// with sv = sqrt(max(v, 1e-8)) correctly rounded and every product and sum
// rounded on its own; a and b are the sigma dW entries of the S and v columns.
__device__ __forceinline__ void heston2_step(float mu_a, float kappa, float theta, float hsig, float rho, float rhob,
                                             float dt, float w1, float w2, float& S, float& v, float& a, float& b) {
  const float muS = clamp100(rn_mul(mu_a, S));
  const float muV = clamp100(rn_mul(kappa, rn_sub(theta, v)));
  const float sv = sqrtf(fmaxf(v, 1e-8f));
  const float sigV = rn_mul(hsig, sv);
  const float d00 = clamp100(rn_mul(sv, S));
  const float d10 = clamp100(rn_mul(rho, sigV)), d11 = clamp100(rn_mul(rhob, sigV));
  a = rn_mul(d00, w1);
  b = rn_add(rn_mul(d10, w1), rn_mul(d11, w2));
  S = rn_add(rn_add(S, rn_mul(muS, dt)), a);
  v = rn_add(rn_add(v, rn_mul(muV, dt)), b);
}

}  // namespace dbsde
