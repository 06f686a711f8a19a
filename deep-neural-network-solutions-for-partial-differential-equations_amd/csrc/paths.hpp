// paths.hpp -- Brownian increments and the Euler-Maruyama path step (gfx950).
//
// FBSNN.fetch_minibatch (DeepBSDE.py:247-262, with_corr...py:316-353) and the
// X recursion of loss_function (DeepBSDE.py:218-222, heston_dnnpde.py:629-642)
// as HIP kernels.  mu and sigma never read Y or Z, so the whole X path is
// computed before the network runs; every kernel here writes the
// network input rows xin[r] = [t, X_1..X_D, 1, 0..] and sdw[r] = sigma(X_n) dW_n
// (the vector the Y-tilde term contracts with Z), r = m (N+1) + n.
//
// Increments come either from the caller (parity mode: W [M, N+1, nb] exactly
// as the reference builds it, dW = W1 - W0 in fp32) or from an
// in-kernel Philox4x32-10 (device mode), keyed by the GLOBAL path index so a
// rank holding paths [path0, path0 + M) draws what one device would draw.
// The device-mode time grid is the reference's: t_n = fp32(fp64 cumsum of
// T/N) (DeepBSDE.py:250-258).
//
// HIP contracts a*b + c into an FMA by default (-ffp-contract=fast), and its
// __fmul_rn/__fadd_rn are plain operators whose contract flag comes from the
// header that defines them, so a pragma at the call site does not stop the
// fusion.  Every kernel here takes its process's step from sde.hpp, where each
// formula is stated once and each operation is rounded on its own (rn.hpp): the
// reference (torch CPU) rounds each product and sum, and X is bit-exact against
// it.
#pragma once
#include "philox.hpp"
#include "sde.hpp"

namespace dbsde {

enum PathOut { PATH_ROLLOUT = 0, PATH_FETCH_W = 1, PATH_FETCH_DW = 2 };

struct RolloutArgs {
  int M, N, D, ldx;
  int nb;                // Brownian dimension (D; D/2 for Heston)
  const float* t;        // [M, N+1] or null (device grid)
  const float* W;        // [M, N+1, nb] or null (Philox)
  const float* Xi;       // [xi_rows, D]
  int xi_rows;
  float T;
  unsigned long long seed, offset;
  long long path0;
  float mu_a, sig_a, sig_b;                // diagonal problems
  float kappa, theta, hsig, rho;           // Heston
  float rhob;                              // two-factor Heston: fp32(sqrt(1 - (double)rho^2))
  const float* Lt;       // correlated device mode: L^T [nb][nb] (upper part of L^T zero)
  float* xin;            // [Rp, ldx]
  float* sdw;            // [Rp, ldx]
  int out;               // PathOut
  float* t_out;          // fetch: [M, N+1]
  float* W_out;          // fetch: [M, N+1, nb] (W) or [M, N, nb] (dW)
};

// increments of steps n0+1 .. n0+4 of coordinate d of local path m: host W
// differences (fp32, the reference's W1 - W0) or sqrt(dt) * Philox normals;
// t1[k] is the time of step n0+k+1 (clamped to N), tacc the fp64 grid sum
__device__ __forceinline__ void step_block(const RolloutArgs& p, int m, int d, int n0, float& w0, double& tacc,
                                           double dt64, float sqdt, float dw[4], float t1[4]) {
  const int N1 = p.N + 1;
  if (p.W) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int n = min(n0 + k + 1, p.N);
      const float w1 = p.W[((size_t)m * N1 + n) * p.nb + d];
      t1[k] = p.t[(size_t)m * N1 + n];
      dw[k] = rn_sub(w1, w0);
      w0 = w1;
    }
  } else {
    float z[4];
    philox_normal4(p.seed, p.offset, (uint32_t)(p.path0 + m), (uint32_t)(n0 >> 2), (uint32_t)d, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dw[k] = sqdt * z[k];
      if (n0 + k + 1 <= p.N) tacc += dt64;
      const int n = min(n0 + k + 1, p.N);
      t1[k] = p.t ? p.t[(size_t)m * N1 + n] : (float)tacc;
    }
  }
}

// fetch_minibatch output of one coordinate: t (d == 0) and W = fp32(fp64
// cumsum of dW), or the raw increments
struct FetchAcc {
  double wsum = 0.0;
  __device__ __forceinline__ void put(const RolloutArgs& p, int m, int d, int n, float tn, float dwn) {
    const int N1 = p.N + 1;
    if (n == 0) {
      if (p.out == PATH_FETCH_W) p.W_out[((size_t)m * N1) * p.nb + d] = 0.f;
      if (d == 0) p.t_out[(size_t)m * N1] = tn;
      return;
    }
    wsum += (double)dwn;
    if (p.out == PATH_FETCH_W)
      p.W_out[((size_t)m * N1 + n) * p.nb + d] = (float)wsum;
    else
      p.W_out[((size_t)m * p.N + n - 1) * p.nb + d] = dwn;
    if (d == 0) p.t_out[(size_t)m * N1 + n] = tn;
  }
};

// --------------------------------------------------------------------------
// diagonal problems (diag_step, sde.hpp)
// --------------------------------------------------------------------------
// the device fetch_minibatch of a diagonal problem: thread per (path m, dim d),
// sequential over n
__global__ void __launch_bounds__(256) fetch_diag_kernel(RolloutArgs p) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= p.M * p.D) return;
  const int m = gid / p.D, d = gid - m * p.D;
  const int N1 = p.N + 1;
  const double dt64 = (double)p.T / (double)p.N;
  const float sqdt = sqrtf(p.T / (float)p.N);
  double tacc = 0.0;
  float w0 = p.W ? p.W[(size_t)m * N1 * p.nb + d] : 0.0f;
  FetchAcc fa;
  fa.put(p, m, d, 0, p.t ? p.t[(size_t)m * N1] : 0.0f, 0.f);
  for (int n0 = 0; n0 < p.N; n0 += 4) {
    float dw[4], t1[4];
    step_block(p, m, d, n0, w0, tacc, dt64, sqdt, dw, t1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (n0 + k >= p.N) break;
      fa.put(p, m, d, n0 + k + 1, t1[k], dw[k]);
    }
  }
}

// The rollouts write whole rows, 16 bytes per lane: thread per (path m, 16-byte
// column group c of the xin / sdw rows), columns 4c .. 4c + 3 = t (column 0),
// X_d (column 1 + d), 1 (column D + 1) and zero padding.  (A thread per
// dimension leaves the padding columns and the misaligned row ends to
// partial-line writes, and the L2 then reads the rest of each line back: 23 MB
// of reads for a kernel with no inputs, profiles/r3_pmc_fetch.)  ColGroup is
// such a thread's state and its stores; what differs between the kernels that
// use it is where the increments come from.
struct ColGroup {
  int c;
  float x[4];
  bool live[4];   // the column is a state dimension
  __device__ __forceinline__ void init(const RolloutArgs& p, int m, int cg) {
    c = cg;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int d = 4 * c + k - 1;
      live[k] = d >= 0 && d < p.D;
      x[k] = live[k] ? p.Xi[(p.xi_rows == 1 ? 0 : m) * p.D + d] : 0.f;
    }
  }
  // the thread's four columns of an xin row at time t0
  __device__ __forceinline__ floatx4 xcols(const RolloutArgs& p, float t0) const {
    floatx4 xo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int col = 4 * c + k;
      xo[k] = col == 0 ? t0 : (col == p.D + 1 ? 1.f : x[k]);
    }
    return xo;
  }
  // row r = m (N + 1) + n, n < N: its xin columns, its sdw columns sigma(X_n) dW_n,
  // and x <- X_{n+1}
  __device__ __forceinline__ void put_row(const RolloutArgs& p, size_t r, float t0, float dt, floatx4 dw) {
    floatx4 xo, so;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int col = 4 * c + k;
      xo[k] = col == 0 ? t0 : (col == p.D + 1 ? 1.f : x[k]);
      so[k] = live[k] ? diag_step(p.mu_a, p.sig_a, p.sig_b, dt, dw[k], x[k]) : 0.f;
    }
    *(floatx4*)(p.xin + r * p.ldx + 4 * c) = xo;
    *(floatx4*)(p.sdw + r * p.ldx + 4 * c) = so;
  }
  // row n = N: X_N and a zero sdw row
  __device__ __forceinline__ void last_row(const RolloutArgs& p, size_t r, float t0) const {
    *(floatx4*)(p.xin + r * p.ldx + 4 * c) = xcols(p, t0);
    *(floatx4*)(p.sdw + r * p.ldx + 4 * c) = floatx4{0.f, 0.f, 0.f, 0.f};
  }
};

// One pass: the thread draws (or differences the caller's W) and steps all N
// steps in sequence.  Parity-mode batches, prefetched rollouts, DBSDE_ROLLOUT2=0.
__global__ void __launch_bounds__(256) rollout4_kernel(RolloutArgs p) {
  const int C = p.ldx >> 2;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= p.M * C) return;
  const int m = gid / C, c = gid - m * C;
  const int N1 = p.N + 1;
  ColGroup g;
  g.init(p, m, c);
  float w0[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) w0[k] = (g.live[k] && p.W) ? p.W[(size_t)m * N1 * p.nb + 4 * c + k - 1] : 0.f;
  const double dt64 = (double)p.T / (double)p.N;
  const float sqdt = sqrtf(p.T / (float)p.N);
  double tacc = 0.0;
  float t0 = p.t ? p.t[(size_t)m * N1] : 0.0f;
  size_t r = (size_t)m * N1;
  for (int n0 = 0; n0 < p.N; n0 += 4) {
    // increments of the live dimensions; every call sees the same grid sum, so
    // t1 (the times of steps n0 + 1 .. n0 + 4) is the same from each
    float dw[4][4], t1[4] = {0.f, 0.f, 0.f, 0.f};
    double tn = tacc;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int i = 0; i < 4; ++i) dw[k][i] = 0.f;
      if (g.live[k]) {
        tn = tacc;
        step_block(p, m, 4 * c + k - 1, n0, w0[k], tn, dt64, sqdt, dw[k], t1);
      }
    }
    tacc = tn;   // unchanged for a thread without live dimensions: its rows hold no t
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (n0 + i >= p.N) break;
      g.put_row(p, r, t0, rn_sub(t1[i], t0), floatx4{dw[0][i], dw[1][i], dw[2][i], dw[3][i]});
      t0 = t1[i];
      ++r;
    }
  }
  g.last_row(p, r, t0);
}

// --------------------------------------------------------------------------
// Device-mode diagonal rollout in two passes (the default for device-mode
// diagonal problems).  rollout4_kernel's 28 M threads each run Philox +
// Box-Muller + Euler for all N steps in sequence, so the draws sit on the
// chain and only M / 9 workgroups exist (33 us at M = 128 as at M = 1024).
//   pass 1 (rollout_draw_kernel): every (path, 4-step Philox block, 16-byte
//     column group) draws in parallel and writes the raw increments
//     sqrt(dt) z into the sdw rows (columns of dims outside [0, D) are 0);
//   pass 2 (rollout_chain_kernel): thread per (path, column group), 64-thread
//     workgroups (spread over every CU: the row stores are bound by each CU's
//     store issue), runs the Euler recursion reading its increments 8 steps
//     ahead and overwrites each sdw row in place with sigma(X) dW.
// Per dimension every value is rollout4_kernel's (same Philox key, same
// sqrt(dt) z, same non-contracted step, the same sequential fp64 time grid),
// so X is bit-identical; sdw is read once more and written once more (2 x
// 4 M N Dp bytes).
// --------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rollout_draw_kernel(RolloutArgs p) {
  const int C = p.ldx >> 2, nsb = (p.N + 3) >> 2;
  const long long gid = blockIdx.x * 256LL + threadIdx.x;
  if (gid >= (long long)p.M * nsb * C) return;
  const int c = (int)(gid % C);
  const long long rest = gid / C;
  const int b = (int)(rest % nsb), m = (int)(rest / nsb);
  const float sqdt = sqrtf(p.T / (float)p.N);
  float dw[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = 4 * c + k - 1;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (d >= 0 && d < p.D) philox_normal4(p.seed, p.offset, (uint32_t)(p.path0 + m), (uint32_t)b, (uint32_t)d, z);
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) dw[k][s2] = (d >= 0 && d < p.D) ? sqdt * z[s2] : 0.f;
  }
  const size_t r0 = (size_t)m * (p.N + 1) + 4 * b;
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2)
    if (4 * b + s2 < p.N)
      *(floatx4*)(p.sdw + (r0 + s2) * p.ldx + 4 * c) = floatx4{dw[0][s2], dw[1][s2], dw[2][s2], dw[3][s2]};
}

constexpr int RC_THREADS = 64;
constexpr int RC_AHEAD = 8;   // increments loaded ahead of the chain
// HOST_T: the caller's time grid p.t instead of the device grid (the wide
// correlated rollout below runs its Euler chains through this kernel too)
template <bool HOST_T = false>
__global__ void __launch_bounds__(RC_THREADS) rollout_chain_kernel(RolloutArgs p) {
  const int C = p.ldx >> 2;
  const int gid = blockIdx.x * RC_THREADS + threadIdx.x;
  if (gid >= p.M * C) return;
  const int m = gid / C, c = gid - m * C;
  const int N1 = p.N + 1;
  ColGroup g;
  g.init(p, m, c);
  const double dt64 = (double)p.T / (double)p.N;
  double tacc = 0.0;
  float t0 = 0.0f;
  if constexpr (HOST_T) t0 = p.t[(size_t)m * N1];
  const size_t r0 = (size_t)m * N1;
  for (int n0 = 0; n0 < p.N; n0 += RC_AHEAD) {
    floatx4 dw[RC_AHEAD];
#pragma unroll
    for (int i = 0; i < RC_AHEAD; ++i)
      dw[i] = n0 + i < p.N ? *(const floatx4*)(p.sdw + (r0 + n0 + i) * p.ldx + 4 * c) : floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < RC_AHEAD; ++i) {
      const int n = n0 + i;
      if (n >= p.N) break;
      tacc += dt64;
      float t1 = (float)tacc;
      if constexpr (HOST_T) t1 = p.t[(size_t)m * N1 + n + 1];
      g.put_row(p, r0 + n, t0, rn_sub(t1, t0), dw[i]);
      t0 = t1;
    }
  }
  g.last_row(p, r0 + p.N, t0);
}

// --------------------------------------------------------------------------
// Cholesky-correlated device mode (with_corr...py:339-341: dW = L (sqrt(dt) z))
// with the correlation product on the matrix cores: per step n the increments
// of a 16-path group are dW^T = L . xi^T, one v_mfma_f32_16x16x4_f32 per
// (16-dim output block o, 4-dim input step t) -- A = L (constant, held in
// registers for the whole rollout), B = xi (this step's uncorrelated
// sqrt(dt) z of the 16 paths, staged in LDS).  L is lower triangular, so block
// o stops at t < 4 o + 4.  The MFMA output layout (lane (cl, q): path cl, dims
// 16 o + 4 q + r) is the layout the Euler step and the xin / sdw rows need, so
// the step runs straight out of the accumulators.
// Workgroup = 16 paths, 8 waves (two per SIMD); wave w < nblk owns output
// block w, with its K-sum in two independent accumulation chains (the
// dependent-accumulator latency bounds a step, not the issue rate).  The
// Philox draws of the next 4-step block (4 normals per (path, dim) call) are
// made by all 512 threads into the other LDS buffer.  nb <= 128.
// LDS: xi[buf][k][q][p][t] (dim 4 t + q of path p at step 4 blk + k), t
// padded to TS = 28 (nb <= 112) or 36 floats: the 16 paths of one q read
// 16-byte slots 28 / 36 floats apart = distinct 4-bank groups (conflict-free
// ds_read_b128).
// --------------------------------------------------------------------------
// Timing-only ablations of the correlated rollout (results wrong by
// construction, never built into the library): bit 0 no row stores, bit 1 no
// draws after the first block, bit 2 no MFMA chain, bit 3 no per-step barrier.
#ifndef DBSDE_AB_CORR
#define DBSDE_AB_CORR 0
#endif
constexpr int CP_NBMAX = 128;
constexpr int CP_PATHS = 16;
constexpr int CP_THREADS = 512;                     // 8 waves: one per output block, the rest draw
// each step's xin / sdw rows are staged in LDS and written as whole float4
// rows (the MFMA layout gives each lane 4 dims of one path, one column off the
// 16-byte grid): [xin, sdw][path][SROW] (SROW = 16 nblk + 20 >= Dp).  Two
// stage buffers: step n's rows are copied out while step n + 1 is computed
// (one barrier per step; the row stores, bound by the CU's store issue, no
// longer wait for the MFMA chain and the Euler step, nor they for them).  At
// nb <= 112 the workgroup's LDS stays at 91 KB, so a phase-kernel workgroup
// (63 KB) still fits beside a prefetched rollout on a CU.
__host__ __device__ constexpr int cp_srow(int nblk) { return 16 * nblk + 20; }
template <int NBLK>
struct CPGeom {
  static constexpr int TS = NBLK <= 7 ? 28 : 36;
  static constexpr int BUF = 4 * 4 * CP_PATHS * TS;     // floats per 4-step draw buffer
  static constexpr int SROW = cp_srow(NBLK);
  static constexpr int STAGE = 2 * CP_PATHS * SROW;     // floats per stage buffer
};

typedef float cpf4 __attribute__((ext_vector_type(4)));

// the uncorrelated sqrt(dt) z of step block sb (steps 4 sb .. 4 sb + 3) of the
// workgroup's 16 paths into one LDS buffer: item (path, dim) -> 4 steps
template <int TS>
__device__ __forceinline__ void corr_draw(const RolloutArgs& p, int m0, int nt4, float sqdt, int sb, float* xb) {
  for (int it = threadIdx.x; it < CP_PATHS * 4 * nt4; it += CP_THREADS) {
    const int pp = it & (CP_PATHS - 1), d = it >> 4;
    const int m = m0 + pp;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (d < p.nb && m < p.M) philox_normal4(p.seed, p.offset, (uint32_t)(p.path0 + m), (uint32_t)sb, (uint32_t)d, z);
    const int qq = d & 3, t = d >> 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) xb[((k * 4 + qq) * CP_PATHS + pp) * TS + t] = sqdt * z[k];
  }
}

// rows of step n (stage buffer sg) -> xin / sdw: every thread of the
// workgroup, whole float4 columns
template <int SROW>
__device__ __forceinline__ void corr_rows_out(const RolloutArgs& p, const float* sg, int m0, int n, int N1) {
  if constexpr (DBSDE_AB_CORR & 1) return;
  const int c4 = p.ldx / 4;
  for (int it = threadIdx.x; it < 2 * CP_PATHS * c4; it += CP_THREADS) {
    const int c = it % c4, rest = it / c4, pp = rest % CP_PATHS, arr = rest / CP_PATHS;
    const int mm = m0 + pp;
    if (mm >= p.M) continue;
    const size_t r2 = (size_t)mm * N1 + n;
    float* dst = arr ? p.sdw : p.xin;
    *(cpf4*)(dst + r2 * p.ldx + 4 * c) = *(const cpf4*)(sg + (arr * CP_PATHS + pp) * SROW + 4 * c);
  }
}

// one wave's share: output blocks O1 and O2 (O2 < 0: none; O1 < 0: the wave
// only draws), K-steps t < 4 O + 4 (the lower triangle; L is zero-padded past
// nb), everything compile-time so the L fragments stay in registers
template <int NBLK, int O1, int O2>
__device__ __forceinline__ void corr_wave(const RolloutArgs& p, float* xs, float* stg) {
  using G = CPGeom<NBLK>;
  constexpr int NO = (O1 >= 0) + (O2 >= 0);
  constexpr int T1 = O1 >= 0 ? 4 * O1 + 4 : 0, T2 = O2 >= 0 ? 4 * O2 + 4 : 0;
  constexpr int TM = T1 > T2 ? T1 : T2;
  const int nb = p.nb, nt4 = (nb + 3) / 4;
  const int lane = threadIdx.x & 63, cl = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.x * CP_PATHS;
  const int N1 = p.N + 1, nsb = (p.N + 3) / 4;
  const float sqdt = sqrtf(p.T / (float)p.N);
  const double dt64 = (double)p.T / (double)p.N;
  const int ob[2] = {O1, O2};
  // A fragments: L[16 o + cl][4 t + q] (zero outside the lower triangle / nb)
  float la1[T1 > 0 ? T1 : 1], la2[T2 > 0 ? T2 : 1];
#pragma unroll
  for (int t = 0; t < T1; ++t) {
    const int d = 16 * O1 + cl, k = 4 * t + q;
    la1[t] = (d < nb && k <= d && k < nb) ? p.Lt[(size_t)k * nb + d] : 0.f;
  }
#pragma unroll
  for (int t = 0; t < T2; ++t) {
    const int d = 16 * O2 + cl, k = 4 * t + q;
    la2[t] = (d < nb && k <= d && k < nb) ? p.Lt[(size_t)k * nb + d] : 0.f;
  }
  const int m = m0 + cl;
  const bool ok = m < p.M;
  float x[2][4];
  FetchAcc fa[2][4];
  float t0 = (p.t && ok) ? p.t[(size_t)m * N1] : 0.f;
#pragma unroll
  for (int oc = 0; oc < NO; ++oc)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int d = 16 * ob[oc] + 4 * q + r;
      const bool own = d < nb && ok;
      x[oc][r] = own ? p.Xi[(p.xi_rows == 1 ? 0 : m) * p.D + d] : 0.f;
      if (own && p.out != PATH_ROLLOUT) fa[oc][r].put(p, m, d, 0, t0, 0.f);
    }
  const bool writes_t = O1 == 0 && q == 0 && ok;   // columns 0 (t) and D + 1 (1)
  double tacc = 0.0;
  // the K-steps past nb (t >= nt4 up to 4 O + 4) read slots no draw writes:
  // zero both buffers once (0 * stale LDS could be NaN)
  for (int i = threadIdx.x; i < 2 * G::BUF; i += CP_THREADS) xs[i] = 0.f;
  for (int i = threadIdx.x; i < 2 * G::STAGE; i += CP_THREADS) stg[i] = 0.f;   // columns never written stay 0
  __syncthreads();
  corr_draw<G::TS>(p, m0, nt4, sqdt, 0, xs);
  __syncthreads();
  for (int sb = 0; sb < nsb; ++sb) {
    if (!(DBSDE_AB_CORR & 2) && sb + 1 < nsb) corr_draw<G::TS>(p, m0, nt4, sqdt, sb + 1, xs + ((sb + 1) & 1) * G::BUF);
    const float* xb = xs + (sb & 1) * G::BUF;
    for (int k = 0; k < 4; ++k) {
      const int n = 4 * sb + k;
      if (n >= p.N) break;
      tacc += dt64;
      const float t1 = (p.t && ok) ? p.t[(size_t)m * N1 + n + 1] : (float)tacc;
      if constexpr (NO > 0) {
        const float* xr = xb + ((k * 4 + q) * CP_PATHS + cl) * G::TS;
        // two independent accumulation chains per block (even / odd K-steps):
        // the dependent-accumulator latency, not the issue rate, bounds a step
        cpf4 acc[2], acc2[2];
#pragma unroll
        for (int oc = 0; oc < 2; ++oc) acc[oc] = acc2[oc] = cpf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s4 = 0; s4 < TM / 4; ++s4) {
          const cpf4 bz = *(const cpf4*)(xr + 4 * s4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int t = 4 * s4 + j;
            cpf4& a1 = (j & 1) ? acc2[0] : acc[0];
            cpf4& a2 = (j & 1) ? acc2[1] : acc[1];
            if constexpr (DBSDE_AB_CORR & 4) {
              if (t == 0) a1[0] += bz[j];
              continue;
            }
            if (t < T1) a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(la1[t < T1 ? t : 0], bz[j], a1, 0, 0, 0);
            if (t < T2) a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(la2[t < T2 ? t : 0], bz[j], a2, 0, 0, 0);
          }
        }
#pragma unroll
        for (int oc = 0; oc < 2; ++oc) acc[oc] += acc2[oc];
        const size_t row = (size_t)m * N1 + n;
        const float dt = rn_sub(t1, t0);
#pragma unroll
        for (int oc = 0; oc < NO; ++oc)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int d = 16 * ob[oc] + 4 * q + r;
            if (d >= nb || !ok) continue;
            const float dw = acc[oc][r];
            if (p.out != PATH_ROLLOUT) {
              fa[oc][r].put(p, m, d, n + 1, t1, dw);
              continue;
            }
            float* sr = stg + (n & 1) * G::STAGE + cl * G::SROW;
            sr[1 + d] = x[oc][r];
            sr[CP_PATHS * G::SROW + 1 + d] = diag_step(p.mu_a, p.sig_a, p.sig_b, dt, dw, x[oc][r]);
          }
        if (writes_t && p.out == PATH_ROLLOUT) {
          float* sr = stg + (n & 1) * G::STAGE + cl * G::SROW;
          sr[0] = t0;
          sr[p.D + 1] = 1.0f;
        }
        (void)row;
      }
      if (p.out == PATH_ROLLOUT) {
        // the previous step's rows (its stage buffer completed before the last
        // barrier) while this step's stage fills; the barrier then orders this
        // step's stage before its copy and the copy before the buffer's reuse
        if (n > 0) corr_rows_out<G::SROW>(p, stg + ((n - 1) & 1) * G::STAGE, m0, n - 1, N1);
        if constexpr (!(DBSDE_AB_CORR & 8)) __syncthreads();
      }
      t0 = t1;
    }
    __syncthreads();
  }
  // the last step's rows
  if (p.out == PATH_ROLLOUT && p.N > 0) corr_rows_out<G::SROW>(p, stg + ((p.N - 1) & 1) * G::STAGE, m0, p.N - 1, N1);
  if constexpr (NO > 0) {
    if (p.out != PATH_ROLLOUT || !ok) return;
    const size_t row = (size_t)m * N1 + p.N;
#pragma unroll
    for (int oc = 0; oc < NO; ++oc)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 16 * ob[oc] + 4 * q + r;
        if (d >= nb) continue;
        p.xin[row * p.ldx + 1 + d] = x[oc][r];
        p.sdw[row * p.ldx + 1 + d] = 0.0f;
      }
    if (writes_t) {
      p.xin[row * p.ldx] = t0;
      p.xin[row * p.ldx + p.D + 1] = 1.0f;
    }
  }
}

// The output block of wave w (-1: it only draws).  Block o costs 4 o + 4
// MFMAs per step (the lower triangle), and waves w and w + 4 share a SIMD, so
// the blocks go in pairs (7 - s, s) of an 8-block triangle to SIMD s (the
// NBLK blocks are its last NBLK): at NBLK = 7 the SIMDs issue 28 MFMAs per
// step each instead of 24 / 32 / 40 / 16 with block w on wave w.
template <int NBLK>
constexpr int corr_block_of_wave(int w) {
  const int s = w & 3, v = (w >> 2) ? s : 7 - s, b = v - (8 - NBLK);
  return b >= 0 ? b : -1;
}
// all 8 waves draw
template <int NBLK>
__global__ void __launch_bounds__(CP_THREADS) rollout_corr_kernel(RolloutArgs p) {
  __shared__ __attribute__((aligned(16))) float xs[2 * CPGeom<NBLK>::BUF];
  __shared__ __attribute__((aligned(16))) float stg[2 * CPGeom<NBLK>::STAGE];
  switch (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) {
    case 0: corr_wave<NBLK, corr_block_of_wave<NBLK>(0), -1>(p, xs, stg); break;
    case 1: corr_wave<NBLK, corr_block_of_wave<NBLK>(1), -1>(p, xs, stg); break;
    case 2: corr_wave<NBLK, corr_block_of_wave<NBLK>(2), -1>(p, xs, stg); break;
    case 3: corr_wave<NBLK, corr_block_of_wave<NBLK>(3), -1>(p, xs, stg); break;
    case 4: corr_wave<NBLK, corr_block_of_wave<NBLK>(4), -1>(p, xs, stg); break;
    case 5: corr_wave<NBLK, corr_block_of_wave<NBLK>(5), -1>(p, xs, stg); break;
    case 6: corr_wave<NBLK, corr_block_of_wave<NBLK>(6), -1>(p, xs, stg); break;
    default: corr_wave<NBLK, corr_block_of_wave<NBLK>(7), -1>(p, xs, stg); break;
  }
}

// --------------------------------------------------------------------------
// Cholesky-correlated device mode for 128 < nb <= 1022.  L no longer fits a
// workgroup's registers and a step's rows no longer fit its LDS, so the
// correlation product leaves the Euler chain: dW = L (sqrt(dt) z) does not
// depend on X, hence every (path, step) pair is one column of a plain
// triangular GEMM, and the chain runs afterwards, as in the two-pass diagonal
// rollout.
//   pass 1 (rollout_corrw_kernel): workgroup = CW_PATHS = 16 paths x one
//     4-step Philox block = 64 columns (4 MFMA column tiles; column 4 p + k =
//     path p, step 4 sb + k), 8 waves; wave w owns the output blocks
//     o = w, w + 8, ... (16 dims each; interleaved, so the triangle's work is
//     spread evenly), at most 8, all four column tiles of each in
//     accumulators.  The K loop runs over 16-dim chunks kc = 0 .. nblk - 1: the
//     uncorrelated sqrt(dt) z of chunk kc + 1 (16 paths x 16 dims = 256 Philox
//     calls, the key of the uncorrelated rollout: seed, offset, global path,
//     step block, coordinate) are drawn into one LDS buffer while chunk kc is
//     multiplied out of the other; block o takes part while kc <= o (the
//     lower triangle).  The 16 x 16 block of L is streamed from the device
//     copy L^T (coalesced over the 16 dims of a block, L2-resident: 4 MB at
//     most) and serves the workgroup's 64 columns.
//     Summation order of dW[d]: chunks kc ascending; inside a chunk the four
//     v_mfma_f32_16x16x4_f32 i = 0..3 in order, MFMA i summing k = 16 kc + 4 q
//     + i over q = 0..3 in the matrix core's fixed order.  fp32 inputs.
//     The increments go to the sdw rows (column 1 + d), or to the fetch
//     output.
//   pass 2: rollout_chain_kernel, the diagonal rollout's Euler chains over
//     the increments in the sdw rows (whole float4 rows of xin / sdw), or, for
//     the fetch, corrw_fetch_kernel (t and the fp64 cumulative sums).
// --------------------------------------------------------------------------
constexpr int CW_PATHS = 16;
constexpr int CW_THREADS = 512;
constexpr int CW_OB = 8;        // output blocks per wave: 8 waves x 8 x 16 = 1024 dims
constexpr int CW_LS = 20;       // LDS row stride of a 16-dim chunk (16 + 4 pad)

// sqrt(dt) z of dims [16 kc, 16 kc + 16) of the 16 paths, steps 4 sb .. 4 sb + 3:
// zs[column 4 p + k][dim in chunk]
__device__ __forceinline__ void corrw_draw(const RolloutArgs& p, int m0, int sb, int kc, float sqdt, float* zs) {
  if (threadIdx.x >= CW_PATHS * 16) return;
  const int pp = threadIdx.x & (CW_PATHS - 1), dl = threadIdx.x >> 4;
  const int d = 16 * kc + dl, m = m0 + pp;
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (d < p.nb && m < p.M) philox_normal4(p.seed, p.offset, (uint32_t)(p.path0 + m), (uint32_t)sb, (uint32_t)d, z);
#pragma unroll
  for (int k = 0; k < 4; ++k) zs[(4 * pp + k) * CW_LS + dl] = (d < p.nb && m < p.M) ? sqdt * z[k] : 0.f;
}

__global__ void __launch_bounds__(CW_THREADS) rollout_corrw_kernel(RolloutArgs p) {
  __shared__ __attribute__((aligned(16))) float zs[2][4 * CW_PATHS * CW_LS];
  const int lane = threadIdx.x & 63, cl = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = blockIdx.x * CW_PATHS, sb = blockIdx.y;
  const int nb = p.nb, nblk = (nb + 15) / 16;
  const float sqdt = sqrtf(p.T / (float)p.N);
  cpf4 acc[CW_OB][4];
#pragma unroll
  for (int b = 0; b < CW_OB; ++b)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[b][t] = cpf4{0.f, 0.f, 0.f, 0.f};
  corrw_draw(p, m0, sb, 0, sqdt, zs[0]);
  __syncthreads();
  for (int kc = 0; kc < nblk; ++kc) {
    if (kc + 1 < nblk) corrw_draw(p, m0, sb, kc + 1, sqdt, zs[(kc + 1) & 1]);
    const float* zb = zs[kc & 1];
    // B operand: column 16 t + cl, dims 16 kc + 4 q + i (MFMA i takes component i)
    cpf4 bz[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) bz[t] = *(const cpf4*)(zb + (16 * t + cl) * CW_LS + 4 * q);
#pragma unroll
    for (int b = 0; b < CW_OB; ++b) {
      const int o = wave + 8 * b;
      if (o < nblk && kc <= o) {   // wave-uniform
        // A operand: L[16 o + cl][16 kc + 4 q + i] = Lt[k][d] (zero above the diagonal)
        const int d = 16 * o + cl;
        float la[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = 16 * kc + 4 * q + i;
          la[i] = (d < nb && k < nb) ? p.Lt[(size_t)k * nb + d] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[b][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(la[i], bz[t][i], acc[b][t], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // accumulator (b, t), lane (cl, q), component r: dim 16 o + 4 q + r of column 16 t + cl
  const int N1 = p.N + 1;
#pragma unroll
  for (int b = 0; b < CW_OB; ++b) {
    const int o = wave + 8 * b;
    if (o >= nblk) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int colw = 16 * t + cl, m = m0 + (colw >> 2), n = 4 * sb + (colw & 3);
      if (m >= p.M || n >= p.N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 16 * o + 4 * q + r;
        if (d >= nb) continue;
        const float dw = acc[b][t][r];
        if (p.out == PATH_ROLLOUT)
          p.sdw[((size_t)m * N1 + n) * p.ldx + 1 + d] = dw;
        else if (p.out == PATH_FETCH_DW)
          p.W_out[((size_t)m * p.N + n) * nb + d] = dw;
        else
          p.W_out[((size_t)m * N1 + n + 1) * nb + d] = dw;
      }
    }
  }
}

// the fetch outputs of the wide correlated kernel: t [M, N+1], and for
// PATH_FETCH_W the increments left in W_out[m, n + 1] summed into W = fp32(fp64
// cumulative sum) (FetchAcc's values).  Thread per (path, coordinate).
__global__ void __launch_bounds__(256) corrw_fetch_kernel(RolloutArgs p) {
  const long long gid = blockIdx.x * 256LL + threadIdx.x;
  if (gid >= (long long)p.M * p.nb) return;
  const int m = (int)(gid / p.nb), d = (int)(gid - (long long)m * p.nb);
  const int N1 = p.N + 1;
  const double dt64 = (double)p.T / (double)p.N;
  double tacc = 0.0, wsum = 0.0;
  if (d == 0) p.t_out[(size_t)m * N1] = p.t ? p.t[(size_t)m * N1] : 0.f;
  if (p.out == PATH_FETCH_W) p.W_out[((size_t)m * N1) * p.nb + d] = 0.f;
  for (int n = 1; n <= p.N; ++n) {
    tacc += dt64;
    if (d == 0) p.t_out[(size_t)m * N1 + n] = p.t ? p.t[(size_t)m * N1 + n] : (float)tacc;
    if (p.out == PATH_FETCH_W) {
      float* w = p.W_out + ((size_t)m * N1 + n) * p.nb + d;
      wsum += (double)*w;
      *w = (float)wsum;
    }
  }
}

// --------------------------------------------------------------------------
// The Heston kernels: state [S_1..S_k, v_1..v_k], thread per (path m, asset
// i), sequential over n.  AssetRows is such a thread's state and its share of
// the rows: columns 1 + i (S_i) and 1 + k + i (v_i) of xin and sdw, and for
// asset 0 also t (column 0) and the constant 1 (column D + 1).  A wave's 64
// threads store two runs of up to 256 contiguous bytes per row and array.
// --------------------------------------------------------------------------
struct AssetRows {
  int i, k;
  float S, v;
  __device__ __forceinline__ void init(const RolloutArgs& p, int m, int asset, int assets) {
    i = asset;
    k = assets;
    const float* xi = p.Xi + (size_t)(p.xi_rows == 1 ? 0 : m) * p.D;
    S = xi[i];
    v = xi[k + i];
  }
  __device__ __forceinline__ void put_x(const RolloutArgs& p, size_t r, float t0) const {
    float* xr = p.xin + r * p.ldx;
    xr[1 + i] = S;
    xr[1 + k + i] = v;
    if (i == 0) {
      xr[0] = t0;
      xr[p.D + 1] = 1.0f;
    }
  }
  __device__ __forceinline__ void put_s(const RolloutArgs& p, size_t r, float a, float b) const {
    p.sdw[r * p.ldx + 1 + i] = a;
    p.sdw[r * p.ldx + 1 + k + i] = b;
  }
  // row n = N: X_N and a zero sdw row
  __device__ __forceinline__ void last_row(const RolloutArgs& p, size_t r, float t0) const {
    put_x(p, r, t0);
    put_s(p, r, 0.0f, 0.0f);
  }
  // row n < N of the one-factor model (heston_step, sde.hpp), increment w
  __device__ __forceinline__ void heston_row(const RolloutArgs& p, size_t r, float t0, float t1, float w) {
    put_x(p, r, t0);
    float a, b;
    heston_step(heston_coef(p.mu_a, p.kappa, p.theta, p.hsig, p.rho, S, v), rn_sub(t1, t0), w, S, v, a, b);
    put_s(p, r, a, b);
  }
};

// k-asset Heston (heston_dnnpde.py), one scalar Brownian motion per asset:
// parity-mode batches (the caller's W), contexts without a factor, and their
// fetch
__global__ void __launch_bounds__(256) rollout_heston_kernel(RolloutArgs p) {
  const int k = p.nb;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= p.M * k) return;
  const int m = gid / k, i = gid - m * k;
  const int N1 = p.N + 1;
  AssetRows g;
  g.init(p, m, i, k);
  const double dt64 = (double)p.T / (double)p.N;
  const float sqdt = sqrtf(p.T / (float)p.N);
  double tacc = 0.0;
  float t0 = p.t ? p.t[(size_t)m * N1] : 0.0f;
  float w0 = p.W ? p.W[(size_t)m * N1 * p.nb + i] : 0.0f;
  size_t r = (size_t)m * N1;
  FetchAcc fa;
  if (p.out != PATH_ROLLOUT) fa.put(p, m, i, 0, t0, 0.f);
  for (int n0 = 0; n0 < p.N; n0 += 4) {
    float dw[4], t1[4];
    step_block(p, m, i, n0, w0, tacc, dt64, sqdt, dw, t1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (n0 + kk >= p.N) break;
      if (p.out != PATH_ROLLOUT) {
        fa.put(p, m, i, n0 + kk + 1, t1[kk], dw[kk]);
        continue;
      }
      g.heston_row(p, r, t0, t1[kk], dw[kk]);
      t0 = t1[kk];
      ++r;
    }
  }
  if (p.out == PATH_ROLLOUT) g.last_row(p, r, t0);
}

// --------------------------------------------------------------------------
// Correlated k-asset Heston in device mode (dbsde_set_corr on a Heston
// context: the assets' Brownian motions are dW = L (sqrt(dt) z), L [k, k]),
// two passes for every k <= 511:
//   pass 1: rollout_corrw_kernel with nb = k.  Its Philox key (seed, offset,
//     global path, step block, coordinate i) is rollout_heston_kernel's, its
//     summation order is the one documented there, and its store
//     sdw[row, 1 + i] is the S_i column of a Heston row (D = 2 k), which parks
//     asset i's increment of step n in row n.
//   pass 2 (rollout_heston_chain_kernel): thread per (path, asset) runs
//     rollout_heston_kernel's rows (AssetRows::heston_row on the same fp64 time
//     grid, so with L = I the paths are bit-identical to the uncorrelated
//     kernel's), reading its increments
//     RC_AHEAD rows ahead of the chain, and overwrites sdw[row, 1 + i] and
//     sdw[row, 1 + k + i] with the Y-tilde term.  A thread reads and writes
//     only its own asset's columns (asset 0's thread also t and the constant
//     1), so no ordering between threads is needed.
// Workgroup size HC_THREADS = 256.  rollout_chain_kernel's 64 (its float4 row
// stores are bound by each CU's store issue, so it spreads them over every CU)
// was measured here too and does not carry over: a wave's 64 threads store 256
// contiguous bytes per instruction, and at M = 1024, N = 100 the launch takes
// 41.7 / 80.2 / 251 us at k = 50 / 130 / 511 with 64 threads, 40.3 / 75.1 / 246
// with 128 and 40.2 / 75.6 / 224 with 256 (profiles/heston_corr_times.json,
// DESIGN 3.7).
// The fetch takes pass 1 into W_out and then corrw_fetch_kernel.
// --------------------------------------------------------------------------
constexpr int HC_THREADS = 256;
template <bool HOST_T = false>
__global__ void __launch_bounds__(256) rollout_heston_chain_kernel(RolloutArgs p) {
  const int k = p.nb;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= p.M * k) return;
  const int m = gid / k, i = gid - m * k;
  const int N1 = p.N + 1;
  AssetRows g;
  g.init(p, m, i, k);
  const double dt64 = (double)p.T / (double)p.N;
  double tacc = 0.0;
  float t0 = 0.0f;
  if constexpr (HOST_T) t0 = p.t[(size_t)m * N1];
  const size_t r0 = (size_t)m * N1;
  for (int n0 = 0; n0 < p.N; n0 += RC_AHEAD) {
    float dw[RC_AHEAD];
#pragma unroll
    for (int a = 0; a < RC_AHEAD; ++a) dw[a] = n0 + a < p.N ? p.sdw[(r0 + n0 + a) * p.ldx + 1 + i] : 0.f;
#pragma unroll
    for (int a = 0; a < RC_AHEAD; ++a) {
      const int n = n0 + a;
      if (n >= p.N) break;
      tacc += dt64;
      float t1 = (float)tacc;
      if constexpr (HOST_T) t1 = p.t[(size_t)m * N1 + n + 1];
      g.heston_row(p, r0 + n, t0, t1, dw[a]);
      t0 = t1;
    }
  }
  g.last_row(p, r0 + p.N, t0);
}

// --------------------------------------------------------------------------
// Two-factor Heston (DBSDE_PROB_HESTON2): the textbook model, two Brownian
// motions per asset.  State [S_1..S_k, v_1..v_k], Brownian dimension nb = 2k:
// coordinate i is W^S_i, coordinate k + i is W^v_i, all independent.  Thread
// per (path m, asset i), sequential over n; per 4-step Philox block it draws
// coordinates i and k + i with the diagonal rollout's key (seed, offset, global
// path, step block, coordinate), so the increments are those of a diagonal
// problem with D = 2k.  The step is heston2_step (sde.hpp), w1 / w2 the
// increments of W^S_i / W^v_i; rhob = fp32(sqrt(1 - (double)rho^2)) comes from
// the host.  One kernel serves the rollout (device grid or the caller's t /
// W [M, N+1, 2k]) and the two fetch outputs.
// --------------------------------------------------------------------------
constexpr int H2_THREADS = 256;
__global__ void __launch_bounds__(H2_THREADS) rollout_heston2_kernel(RolloutArgs p) {
  const int k = p.D >> 1;   // nb = D = 2k
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= p.M * k) return;
  const int m = gid / k, i = gid - m * k;
  const int N1 = p.N + 1;
  AssetRows g;
  g.init(p, m, i, k);
  const double dt64 = (double)p.T / (double)p.N;
  const float sqdt = sqrtf(p.T / (float)p.N);
  double tacc = 0.0;
  float t0 = p.t ? p.t[(size_t)m * N1] : 0.0f;
  float w0s = p.W ? p.W[(size_t)m * N1 * p.nb + i] : 0.0f;
  float w0v = p.W ? p.W[(size_t)m * N1 * p.nb + k + i] : 0.0f;
  size_t r = (size_t)m * N1;
  FetchAcc fs, fv;
  if (p.out != PATH_ROLLOUT) {
    fs.put(p, m, i, 0, t0, 0.f);
    fv.put(p, m, k + i, 0, t0, 0.f);
  }
  for (int n0 = 0; n0 < p.N; n0 += 4) {
    // both calls see the same grid sum, so t1 is the same from each
    float dws[4], dwv[4], t1[4];
    double tn = tacc;
    step_block(p, m, i, n0, w0s, tn, dt64, sqdt, dws, t1);
    step_block(p, m, k + i, n0, w0v, tacc, dt64, sqdt, dwv, t1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (n0 + kk >= p.N) break;
      if (p.out != PATH_ROLLOUT) {
        fs.put(p, m, i, n0 + kk + 1, t1[kk], dws[kk]);
        fv.put(p, m, k + i, n0 + kk + 1, t1[kk], dwv[kk]);
        continue;
      }
      g.put_x(p, r, t0);
      float a, b;
      heston2_step(p.mu_a, p.kappa, p.theta, p.hsig, p.rho, p.rhob, rn_sub(t1[kk], t0), dws[kk], dwv[kk], g.S, g.v, a, b);
      g.put_s(p, r, a, b);
      t0 = t1[kk];
      ++r;
    }
  }
  if (p.out == PATH_ROLLOUT) g.last_row(p, r, t0);
}

// --------------------------------------------------------------------------
// Arithmetic-average (Asian) problems (DBSDE_PROB_ASIAN): state [A, S_1..S_k],
// D = k + 1, Brownian dimension nb = k.  xin column 0 is t, column 1 is A,
// column 2 + i is S_i (coordinate i = column - 2), column D + 1 the constant 1.
// Two passes:
//   pass 1 (rollout_asian_chain_kernel): the S columns, in ColGroup form -- a
//     thread owns one path and one 16-byte column group and writes whole float4
//     rows of xin and sdw.  S_i is the diagonal process (diag_step) on
//     coordinate i of the diagonal rollout's Philox key, so its increments are
//     those of a diagonal problem with D = k.  WS = false: the increments are
//     drawn per 4-step Philox block or differenced from the caller's W
//     (step_block: device grid or the caller's t), as rollout4_kernel does.
//     WS = true (a factor, dbsde_set_corr): rollout_corrw_kernel ran first with
//     its sdw pointer at xin + 1, so its store "column 1 + i" parked coordinate
//     i's increment of step n in xin[row n, 2 + i] -- the S_i column itself;
//     the thread reads its own columns RC_AHEAD rows ahead of the chain and
//     overwrites them with X (no other thread touches them: no ordering between
//     threads is needed), as the correlated Heston chain does with the sdw
//     rows.  Column 1 gets A_0 in xin and 0 in sdw: the A column has no
//     diffusion, so sdw[:, 1] is exactly 0 in every row.
//   pass 2 (rollout_asian_avg_kernel): the A column.  A 16-lane group per path;
//     per row lane l sums columns 2 + l, 2 + l + 16, ... ascending and the
//     lanes meet in the xor butterfly (asian_row_sum's order, sde.hpp); A is
//     the sequential prefix over n (asian_step) with dt_n the fp32 difference
//     of the rows' own t column, which is pass 1's dt.  The row sums of
//     AA_ROWS rows are formed before their prefix steps, so their loads are in
//     flight together.  It reads the xin rows once and writes xin[:, 1].
// --------------------------------------------------------------------------
struct AsianGroup {
  int c;
  float x[4], a0;
  bool live[4];   // the column is an asset S_i
  __device__ __forceinline__ void init(const RolloutArgs& p, int m, int cg) {
    c = cg;
    const float* xi = p.Xi + (size_t)(p.xi_rows == 1 ? 0 : m) * p.D;
    a0 = xi[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = 4 * c + k - 2;
      live[k] = i >= 0 && i < p.nb;
      x[k] = live[k] ? xi[1 + i] : 0.f;
    }
  }
  __device__ __forceinline__ floatx4 xcols(const RolloutArgs& p, float t0) const {
    floatx4 xo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int col = 4 * c + k;
      xo[k] = col == 0 ? t0 : (col == 1 ? a0 : (col == p.D + 1 ? 1.f : x[k]));
    }
    return xo;
  }
  // row r = m (N + 1) + n, n < N, and x <- S_{n+1}
  __device__ __forceinline__ void put_row(const RolloutArgs& p, size_t r, float t0, float dt, floatx4 dw) {
    const floatx4 xo = xcols(p, t0);
    floatx4 so;
#pragma unroll
    for (int k = 0; k < 4; ++k) so[k] = live[k] ? diag_step(p.mu_a, p.sig_a, p.sig_b, dt, dw[k], x[k]) : 0.f;
    *(floatx4*)(p.xin + r * p.ldx + 4 * c) = xo;
    *(floatx4*)(p.sdw + r * p.ldx + 4 * c) = so;
  }
  __device__ __forceinline__ void last_row(const RolloutArgs& p, size_t r, float t0) const {
    *(floatx4*)(p.xin + r * p.ldx + 4 * c) = xcols(p, t0);
    *(floatx4*)(p.sdw + r * p.ldx + 4 * c) = floatx4{0.f, 0.f, 0.f, 0.f};
  }
};

template <bool WS>
__global__ void __launch_bounds__(WS ? RC_THREADS : 256) rollout_asian_chain_kernel(RolloutArgs p) {
  const int C = p.ldx >> 2;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= p.M * C) return;
  const int m = gid / C, c = gid - m * C;
  const int N1 = p.N + 1;
  AsianGroup g;
  g.init(p, m, c);
  const double dt64 = (double)p.T / (double)p.N;
  double tacc = 0.0;
  float t0 = p.t ? p.t[(size_t)m * N1] : 0.0f;
  const size_t r0 = (size_t)m * N1;
  if constexpr (WS) {
    for (int n0 = 0; n0 < p.N; n0 += RC_AHEAD) {
      floatx4 dw[RC_AHEAD];
#pragma unroll
      for (int i = 0; i < RC_AHEAD; ++i)
        dw[i] = n0 + i < p.N ? *(const floatx4*)(p.xin + (r0 + n0 + i) * p.ldx + 4 * c) : floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < RC_AHEAD; ++i) {
        const int n = n0 + i;
        if (n >= p.N) break;
        tacc += dt64;
        const float t1 = p.t ? p.t[(size_t)m * N1 + n + 1] : (float)tacc;
        g.put_row(p, r0 + n, t0, rn_sub(t1, t0), dw[i]);
        t0 = t1;
      }
    }
  } else {
    float w0[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w0[k] = (g.live[k] && p.W) ? p.W[(size_t)m * N1 * p.nb + 4 * c + k - 2] : 0.f;
    const float sqdt = sqrtf(p.T / (float)p.N);
    size_t r = r0;
    for (int n0 = 0; n0 < p.N; n0 += 4) {
      // every call sees the same grid sum, so t1 is the same from each
      float dw[4][4], t1[4] = {0.f, 0.f, 0.f, 0.f};
      double tn = tacc;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int i = 0; i < 4; ++i) dw[k][i] = 0.f;
        if (g.live[k]) {
          tn = tacc;
          step_block(p, m, 4 * c + k - 2, n0, w0[k], tn, dt64, sqdt, dw[k], t1);
        }
      }
      tacc = tn;   // unchanged for a thread without an asset column: its rows hold no t (column 2 is S_1)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (n0 + i >= p.N) break;
        g.put_row(p, r, t0, rn_sub(t1[i], t0), floatx4{dw[0][i], dw[1][i], dw[2][i], dw[3][i]});
        t0 = t1[i];
        ++r;
      }
    }
  }
  g.last_row(p, r0 + p.N, t0);
}

constexpr int AA_ROWS = 4;        // row sums in flight per prefix block
constexpr int AA_THREADS = 256;   // 16 paths per workgroup
constexpr int AA_TERMS = 8;       // loads of one lane sum in flight
// asian_lane_sum (sde.hpp): the same terms added in the same order, their loads
// issued AA_TERMS at a time ahead of the adds
// GEO (geo_lane_sum): the terms are lg(S_i), taken after the loads
template <bool GEO>
__device__ __forceinline__ float asian_lane_sum_ahead(const float* S, int k, int lane) {
  float p = 0.f;
  for (int i0 = lane; i0 < k; i0 += AA_TERMS * ASIAN_LANES) {
    float v[AA_TERMS];
#pragma unroll
    for (int j = 0; j < AA_TERMS; ++j) v[j] = i0 + j * ASIAN_LANES < k ? S[i0 + j * ASIAN_LANES] : 0.f;
#pragma unroll
    for (int j = 0; j < AA_TERMS; ++j)
      if (i0 + j * ASIAN_LANES < k) p = rn_add(p, GEO ? geo_lg(v[j]) : v[j]);
  }
  return p;
}
// GEO (DBSDE_PROB_GEO_ASIAN): the carried value is a = log G (a_0 = lg(G_0)), the
// row terms are lg(S_i), row 0 stores G_0 as given and row n >= 1 exp(a_n)
template <bool GEO>
__global__ void __launch_bounds__(AA_THREADS) rollout_asian_avg_kernel(RolloutArgs p) {
  const long long gid = (long long)blockIdx.x * AA_THREADS + threadIdx.x;
  const bool ok = gid / ASIAN_LANES < p.M;   // (a 16-lane group is one path: its lanes agree)
  const int m = ok ? (int)(gid / ASIAN_LANES) : 0, l = (int)(gid & (ASIAN_LANES - 1));
  const int k = p.nb, N1 = p.N + 1;
  const float* xr = p.xin + (size_t)m * N1 * p.ldx;
  float A = ok ? p.Xi[(size_t)(p.xi_rows == 1 ? 0 : m) * p.D] : 0.f;
  const float G0 = A;
  if constexpr (GEO) A = geo_lg(A);
  for (int n0 = 0; n0 <= p.N; n0 += AA_ROWS) {
    float s[AA_ROWS], dt[AA_ROWS];
#pragma unroll
    for (int j = 0; j < AA_ROWS; ++j) {
      const int n = n0 + j;
      const bool row = ok && n < p.N;
      s[j] = row ? asian_lane_sum_ahead<GEO>(xr + (size_t)n * p.ldx + 2, k, l) : 0.f;
      dt[j] = row ? rn_sub(xr[(size_t)(n + 1) * p.ldx], xr[(size_t)n * p.ldx]) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < AA_ROWS; ++j) {
#pragma unroll
      for (int o = 1; o < ASIAN_LANES; o <<= 1) s[j] = rn_add(s[j], __shfl_xor(s[j], o));
    }
#pragma unroll
    for (int j = 0; j < AA_ROWS; ++j) {
      const int n = n0 + j;
      if (!ok || n > p.N) break;
      if (l == 0) p.xin[((size_t)m * N1 + n) * p.ldx + 1] = GEO ? (n == 0 ? G0 : geo_exp(A)) : A;
      if (n < p.N) asian_step(asian_mean(s[j], k), dt[j], p.T, A);
    }
  }
}

// --------------------------------------------------------------------------
// Knock-out (barrier) problems (DBSDE_PROB_BARRIER): DIAG's rows from whichever
// rollout form ran before (one pass, draw + chain, the correlated kernels, the
// caller's t / W), then this pass stops each path at its first hit row
// (barrier_stop, sde.hpp, restated over a 16-lane group per path as
// rollout_asian_avg_kernel is).  Per row lane l sums the payoff's columns
// 1 + l, 1 + l + 16, .. ascending and the lanes meet in the xor butterfly
// (asian_row_sum's order), BS_ROWS rows' loads in flight before their
// comparisons; every lane of the group ends with the same sum, so the lanes
// agree on tau and leave the scan together.  Then the group's lanes own the
// 16-byte column groups c = l, l + 16, ..: the state columns of rows n > tau
// get row tau's, those of sdw rows tau .. N - 1 get 0 (row N is 0 already) --
// whole float4 stores where all four columns are state columns, single floats
// in the two edge groups, which hold t (column 0) and the constant 1 (column
// D + 1): neither is touched.  A path that never hits, or hits at row N, writes
// nothing.  Reads happen before the scan ends and writes only after it, to
// rows the group no longer reads, and no other group touches the path.
// --------------------------------------------------------------------------
struct BarrierArgs {
  float B, gsign;   // barrier_hit's: gsign > 0 knocks at stat <= B, gsign < 0 at stat >= B
  int cols, mean;   // the payoff's g_cols columns; mean: stat = sum / cols
};
constexpr int BS_ROWS = 4;        // row sums in flight per scan block
constexpr int BS_THREADS = 256;   // 16 paths per workgroup
__global__ void __launch_bounds__(BS_THREADS) rollout_barrier_stop_kernel(RolloutArgs p, BarrierArgs b) {
  const long long gid = (long long)blockIdx.x * BS_THREADS + threadIdx.x;
  if (gid / ASIAN_LANES >= p.M) return;   // (a 16-lane group is one path: its lanes leave together)
  const int m = (int)(gid / ASIAN_LANES), l = (int)(gid & (ASIAN_LANES - 1));
  const int N1 = p.N + 1;
  float* xr = p.xin + (size_t)m * N1 * p.ldx;
  float* sr = p.sdw + (size_t)m * N1 * p.ldx;
  int tau = N1;
  for (int n0 = 0; n0 <= p.N && tau == N1; n0 += BS_ROWS) {
    float s[BS_ROWS];
#pragma unroll
    for (int j = 0; j < BS_ROWS; ++j)
      s[j] = n0 + j <= p.N ? asian_lane_sum_ahead<false>(xr + (size_t)(n0 + j) * p.ldx + 1, b.cols, l) : 0.f;
#pragma unroll
    for (int j = 0; j < BS_ROWS; ++j) {
#pragma unroll
      for (int o = 1; o < ASIAN_LANES; o <<= 1) s[j] = rn_add(s[j], __shfl_xor(s[j], o));
    }
#pragma unroll
    for (int j = 0; j < BS_ROWS; ++j) {
      const float stat = b.mean ? asian_mean(s[j], b.cols) : s[j];
      if (tau == N1 && n0 + j <= p.N && barrier_hit(stat, b.B, b.gsign)) tau = n0 + j;
    }
  }
  if (tau >= p.N) return;
  for (int c = l; c < (p.ldx >> 2); c += ASIAN_LANES) {
    const int c0 = 4 * c;
    if (c0 > p.D) break;                         // past the last state column
    const bool whole = c0 >= 1 && c0 + 3 <= p.D;   // columns 4c .. 4c + 3 are all state columns
    if (whole) {
      const floatx4 xt = *(const floatx4*)(xr + (size_t)tau * p.ldx + c0);
      for (int n = tau + 1; n <= p.N; ++n) *(floatx4*)(xr + (size_t)n * p.ldx + c0) = xt;
      for (int n = tau; n < p.N; ++n) *(floatx4*)(sr + (size_t)n * p.ldx + c0) = floatx4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = c0 + k;
        if (col < 1 || col > p.D) continue;
        const float xt = xr[(size_t)tau * p.ldx + col];
        for (int n = tau + 1; n <= p.N; ++n) xr[(size_t)n * p.ldx + col] = xt;
        for (int n = tau; n < p.N; ++n) sr[(size_t)n * p.ldx + col] = 0.f;
      }
    }
  }
}

// Q3 (D == 1): S_n = sum over paths of sdw[m, n]   (1d_BSPDE_case.py:271-273)
__global__ void __launch_bounds__(256) q3_sum_kernel(const float* sdw, int ldx, int M, int N, float* S) {
  const int n = blockIdx.x;
  __shared__ float red[256];
  float acc = 0.f;
  for (int m = threadIdx.x; m < M; m += 256) acc += sdw[((size_t)m * (N + 1) + n) * ldx + 1];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) S[n] = red[0];
}

}  // namespace dbsde
