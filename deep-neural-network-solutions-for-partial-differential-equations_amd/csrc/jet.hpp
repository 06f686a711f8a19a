// jet.hpp -- forward (Taylor-mode) propagation of first and second directional
// derivatives through the network, in its inputs z = (t, x):
//   d1 = grad_z net(z) . v,   d2 = v^T hess_z net(z) v
// for jet rows (point r, direction v_rj).  With B_j the packed block weight
// (the negated NAIS projection), V_j the input-skip weight and rho the
// residual flag:
//   pdot_0 = W_in v             hdot_0 = act'(p_0) pdot_0       hddot_0 = act''(p_0) pdot_0^2
//   pdot_j = B_j hdot_{j-1} + V_j v        pddot_j = B_j hddot_{j-1}
//   hdot_j  = act'(p_j) pdot_j + rho hdot_{j-1}
//   hddot_j = act''(p_j) pdot_j^2 + act'(p_j) pddot_j + rho hddot_{j-1}
//   d1 = w_out . hdot_K         d2 = w_out . hddot_K
// The pre-activations p_j depend on the point alone: a point pass of the same
// kernel family writes act'(p_j) and act''(p_j) once per point ([R, Stot]),
// the jet pass reads them by point index.  Nothing is stored per jet row.
// Both passes read the weights as split-bf16 fragments written once per call
// (jet_split_launch) from the context's fp32 copies.
#pragma once
#include <hip/hip_runtime.h>

namespace dbsde {

constexpr int JET_KMAX = 6;   // hidden blocks (ctx: K <= 6)
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

struct JetArgs {
  // weights, fp32 row-major [out][in] (ctx BtIn / Bf / beta / wout / bout)
  const float* Wx;                  // x-stack rows [Stot_x][Dp]: cols 0..D weights, col D+1 bias
  const float* Bf[JET_KMAX + 1];    // block j = 1..K: [16 tw[j]][16 tw[j-1]]
  const float* beta[JET_KMAX + 1];  // block bias (networks without the x-stack), else null
  // the same weights as split-bf16 fragments (jet.hip jet_split_kernel): the
  // image, and the first fragment of the x-stack level j / block j in it
  const uintx4* img;
  long long offX[JET_KMAX + 1], offB[JET_KMAX + 1];
  const float* wout;
  const float* bout;
  int tw[JET_KMAX + 1];             // 16-wide blocks of level j = 0..K
  int col[JET_KMAX + 1];            // level j's first column of an [., Stot] row (and x-stack row)
  int twmax, ldw;                   // max tw; LDS state row stride 16 twmax + 4
  int K, D, Dp, Stot, has_v, act;
  float rho;
  // rows of this launch
  long long nrows;                  // points (point pass) or jet rows (jet pass)
  long long g0, p0;                 // jet pass: point of row g = p0 + (g0 + g) / nd
  int nd;
  const float* t;                   // point pass: [nrows]
  const float* X;                   // point pass: [nrows, D]
  const float* V;                   // jet pass: [nrows, D + 1], column 0 = the t component
  float* A1;                        // [points, Stot] act'(p):  written by the point pass, read by the jet pass
  float* A2;                        // [points, Stot] act''(p)
  float* umask;                     // [points] 1 / 0 (u-clamp contexts) or null
  float* d1;                        // jet pass outputs [nrows], each nullable
  float* d2;
};

// point != 0: the point pass.  Returns -1 on a geometry the kernels do not cover.
int jet_launch(const JetArgs& a, int point, hipStream_t s);
long long jet_image_layout(JetArgs& a);               // fills offX / offB; the image size in 16-byte units
int jet_split_launch(const JetArgs& a, hipStream_t s);   // fp32 weights -> the image

}  // namespace dbsde
