// act.hpp -- SiLU and Softplus (beta = 1): value, first and second derivative,
// defined once for the runtime-switched activations of kernels.hpp and the
// compile-time ones of fused.hpp.
//
// Overflow-free form: one exponential of a non-positive argument and one
// reciprocal of a number in [1, 2] per element; Softplus's value alone takes a
// logarithm more (phase C needs only the derivatives and never computes it).
//   e = exp(-|a|)   r = 1 / (1 + e)   s = a >= 0 ? r : e r   q = e r r
//   Softplus: f = max(a, 0) + log1p(e)   f' = s         f'' = q
//   SiLU:     f = a s                    f' = s + a q   f'' = q (2 + a (1 - 2 s))
// s is the logistic sigmoid and q = s (1 - s) without the cancellation of 1 - s
// (at a = 60 the subtraction gives 0 where q is 8.8e-27).  e underflows to 0
// for |a| > 104, where s, q and the products a q are 0 or 1 exactly: nothing
// overflows and no 0 * inf arises for finite a.
// torch's Softplus switches to the identity above its threshold of 20; the
// smooth form differs from it by 2.1e-9 there, below fp32 resolution, and is
// taken everywhere.
//
// Device code takes the hardware v_exp_f32 / v_rcp_f32 / v_log_f32 (1 ulp each
// on these ranges: e <= 1, 1 + e in [1, 2]); host code takes libm.  Without
// hipcc this is plain C++ (no HIP header).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
#include <math.h>
#endif
#ifndef DBSDE_HD
#ifdef __HIPCC__
#define DBSDE_HD __host__ __device__ __forceinline__
#else
#define DBSDE_HD inline
#endif
#endif

namespace dbsde {

// e = exp(-|a|), s = sigmoid(a), q = s (1 - s)
DBSDE_HD void act_esq(float a, float& e, float& s, float& q) {
#ifdef __HIP_DEVICE_COMPILE__
  e = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(a));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
#else
  e = expf(-fabsf(a));
  const float r = 1.f / (1.f + e);
#endif
  const float er = e * r;
  s = a >= 0.f ? r : er;
  q = er * r;
}
// log(1 + e) for e in [0, 1]
DBSDE_HD float act_log1p(float e) {
#ifdef __HIP_DEVICE_COMPILE__
  return 0.6931471805599453f * __builtin_amdgcn_logf(1.f + e);
#else
  return log1pf(e);
#endif
}

DBSDE_HD float softplus_f(float a) {
  float e, s, q;
  act_esq(a, e, s, q);
  return fmaxf(a, 0.f) + act_log1p(e);
}
DBSDE_HD float softplus_1(float a) {
  float e, s, q;
  act_esq(a, e, s, q);
  return s;
}
DBSDE_HD void softplus_v1(float a, float& f, float& d1) {
  float e, q;
  act_esq(a, e, d1, q);
  f = fmaxf(a, 0.f) + act_log1p(e);
}
DBSDE_HD void softplus_12(float a, float& d1, float& d2) {
  float e;
  act_esq(a, e, d1, d2);
}

DBSDE_HD float silu_f(float a) {
  float e, s, q;
  act_esq(a, e, s, q);
  return a * s;
}
DBSDE_HD float silu_1(float a) {
  float e, s, q;
  act_esq(a, e, s, q);
  return s + a * q;
}
DBSDE_HD void silu_v1(float a, float& f, float& d1) {
  float e, s, q;
  act_esq(a, e, s, q);
  f = a * s;
  d1 = s + a * q;
}
DBSDE_HD void silu_12(float a, float& d1, float& d2) {
  float e, s, q;
  act_esq(a, e, s, q);
  d1 = s + a * q;
  d2 = q * (2.f + a * (1.f - 2.f * s));
}

}  // namespace dbsde
