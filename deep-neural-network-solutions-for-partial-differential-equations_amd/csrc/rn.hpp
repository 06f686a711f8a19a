// rn.hpp -- individually rounded fp32 operations for the Euler path steps of
// sde.hpp.
//
// HIP contracts a*b + c into an FMA by default (-ffp-contract=fast), and its
// __fmul_rn/__fadd_rn are plain operators whose contract flag comes from the
// header that defines them, so a pragma at the call site does not stop the
// fusion.  rn_mul/rn_add/rn_sub below carry no contract flag: the reference
// (torch CPU) rounds each product and sum, and X is bit-exact against it.
//
// Without hipcc this is plain C++ (no HIP header; build it with
// -ffp-contract=off, the pragma is clang's).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DBSDE_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define DBSDE_HD inline
#endif

namespace dbsde {

DBSDE_HD float rn_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
DBSDE_HD float rn_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
DBSDE_HD float rn_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

// the reference's clamp of the Heston drift and diffusion entries
DBSDE_HD float clamp100(float v) { return fminf(fmaxf(v, -100.f), 100.f); }

}  // namespace dbsde
