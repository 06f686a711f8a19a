// NAIS projection at hidden widths 128 < L <= 1024 (projw.hip): R_j = W_j^T W_j,
// its Frobenius norm, and the projection adjoint Wbar_j = W_j S_j, on the
// matrix cores in K-chunked 64 x 64 tiles.  The kernels of kernels.hpp
// (rtr_params_kernel, proj_backward_kernel) keep L <= 128, where whole operand
// strips fit in LDS and the products are latency-bound.
//
// One number per block, read by everyone: |R_j|_F^2 is reduced once from the
// per-tile partial sums into sq[j]; pack_block's PK_NEGPROJ (which takes it as
// a single partial) and the adjoint both form |R_j|_F = sqrt(sq[j]) from that
// value.  <Abar_j, R_j> is reduced once from the finalize's partials into
// dot[j].  Every sum has a fixed order and nothing is accumulated with
// atomics, so a second call is bitwise equal to the first.
#pragma once
#include <hip/hip_runtime.h>

namespace dbsde {

constexpr int NAIS_WIDE_LMAX = 1024;
constexpr int PW_TILE = 64;   // output tile edge of both products

// tiles of one triangle (ti <= tj) of the L x L product
inline int projw_tri_tiles(int L) {
  const int nt = (L + PW_TILE - 1) / PW_TILE;
  return nt * (nt + 1) / 2;
}

struct ProjWideArgs {
  const float* params;        // flat parameters (forward: W_j = params + woffs[j])
  const long long* woffs;     // [K] device
  int L, K;
  float* const* rtr;          // [K] device: R_j [L, L]
  float* const* wsnap;        // [K] device: W_j as of the forward product
  float* const* abar;         // [K] device: Abar_j [L, L] (adjoint)
  float* const* sbuf;         // [K] device: S_j [L, L] (adjoint)
  double* part;               // [K, npart] per-tile sums of squares
  int npart;                  // projw_tri_tiles(L)
  double* sq;                 // [K] |R_j|_F^2
  const double* dot_part;     // [K, dot_nblk] <Abar_j, R_j> partials, dot_nused written
  int dot_nblk, dot_nused;
  double* dot;                // [K] <Abar_j, R_j>
  float* grad;                // flat gradient (adjoint: Wbar_j -> grad + woffs[j])
};

// R_j, the W_j snapshot, the partials and sq[j]; -1 for a geometry the
// kernels do not cover (launch errors are left for hipGetLastError)
__attribute__((visibility("hidden"))) int projw_forward_launch(const ProjWideArgs& a, hipStream_t s);
// dot[j], S_j = cA (Abar_j + Abar_j^T) - cR (R_j + R_j^T), grad W_j = W_j S_j
__attribute__((visibility("hidden"))) int projw_backward_launch(const ProjWideArgs& a, hipStream_t s);

}  // namespace dbsde
