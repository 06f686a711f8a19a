// mc.hip -- Feynman-Kac Monte-Carlo comparator for every linear problem
// (dbsde_mc_value, include/dbsde.h).  The device counterpart of the reference
// drivers' Monte-Carlo pricers (with_corr...py:1283-1325 generate_paths /
// monte_carlo_price, basket_pricer.py, numerics/multidimensional_mc_pricer.py,
// numerics/heston_closed_form_ii.py:6-83), simulating the problem's OWN SDE.
//
// Mathematics.  A dbsde_problem with phi_zz == 0 has phi = phi_r (Y - phi_c X.Z),
// so the BSDE the step trains on is the linear PDE
//   u_t + (mu + phi_r phi_c X).Du + 1/2 tr(sigma sigma^T D^2 u) - phi_r u = 0,  u(T, .) = g,
// whose solution is  u(t, x) = E[ exp(-phi_r tau) g(X~_T) | X~_t = x ],  tau = T - t,
// X~ following the problem's Euler scheme with drift coefficient
// mu_eff = mu_a + phi_r phi_c (fp32, computed once).  Check: BSB has mu = 0,
// sigma = 0.4 X, phi = r (Y - X.Z): exp((r + sigma^2) tau) |x|^2 = DBSDE_EXACT_BSB.
// Heston has phi_c = 0 and its own drift and 2x2 blocks (heston_step, sde.hpp,
// as the rollout kernels); the two-factor Heston (DBSDE_PROB_HESTON2,
// path kind MC_HESTON2) runs heston2_step on two normals per step,
// those of coordinates d (W^S_d) and nd + d (W^v_d), nd = D / 2 -- the
// increments rollout_heston2_kernel draws.  phi_zz != 0 (HJB) is not linear:
// dbsde_hjb_mc.
// Arithmetic average (DBSDE_PROB_ASIAN, path kinds MC_ASIAN / MC_ASIAN_CORR):
// state [A, S_1..S_k], nd = k; thread (sample, asset d) runs diag_step on S_d
// and accumulates I_d = sum_n (double)fp32(S_{d,n} dt_n) (the left-point rule
// of asian_step, sde.hpp) -- no reduction per step.  A sample's payoff terms are
// its I_d: the end-of-path LDS reduction sums them in order, A_T = A_p +
// (sum_d I_d) / (k T) (T the averaging horizon, not tau_p), and mc_payoff runs
// with one column.  Delta: dA_T/dA_p = 1 (the reducing threads sum dg/dA_T),
// dA_T/dS_d = (sum_n (double)fp32(J_{d,n} dt_n)) / (k T) with DIAG's tangent J.
// Geometric average (DBSDE_PROB_GEO_ASIAN, MC_GEO_ASIAN / MC_GEO_ASIAN_CORR):
// state [G, S_1..S_k]; the same layout with I_d = sum_n (double)fp32(lg(S_{d,n})
// dt_n) (geo_lg, sde.hpp) and G_T = G_p exp((sum_d I_d) / (k T)) in fp64 after the
// end-of-path reduction -- the exponential form keeps "no reduction per step".
// Delta: dG_T/dG_p = G_T / G_p, dG_T/dS_d = G_T (sum_n (double)fp32((J_{d,n} /
// S_{d,n}) dt_n)) / (k T).
//
// Knock-out (DBSDE_PROB_BARRIER, mc_barrier_kernel): the summand is g(X_N) times
// alive = no row 0..n_steps of the sample's path was knocked.  The statistic needs a
// sum over the assets at every step, which the thread-per-(sample, coordinate) layout
// above does not have, so the kind has a kernel of its own: a 16-lane group runs one
// sample of one point, lane l the assets l, l + 16, .. (nd <= 128: eight per lane, in
// registers), and per step the lanes form barrier_stat's sum -- their ascending fp32
// partial sums met in the xor butterfly, asian_row_sum's order exactly -- and compare
// in fp32 (barrier_hit).  A knocked sample stops there (its summand is 0).  g(X_N)
// takes the fp64 sum of the lanes' ascending fp64 partial sums met in the same
// butterfly.  Workgroup = 16 groups = 16 samples side by side; grid (point, chunk);
// each group accumulates sum g and sum g^2 over its samples in fp64, the 16 groups
// are summed in order into the partials and mc_barrier_final_kernel sums the chunks:
// no atomics, bitwise repeatable, and a point's result depends on neither P nor its
// index (a workgroup serves one point; the chunking is a function of mc alone).  With
// L the unscaled L z come from the correlated Heston's increment workspace (below),
// with its bound and grouping.  No delta: the pathwise estimator is biased across
// the indicator.
//
// Draws.  The normals of sample k, step n, Brownian coordinate d are
// philox_normal4(seed, offset, k, n >> 2, d)[n & 3] -- the device-mode rollout's
// keying for global path k -- for EVERY point of a call (common random numbers).
// Point p runs the training grid with T replaced by tau_p = fp32(T) - t_p:
// t_n = fp32(fp64 cumsum of tau_p / n_steps), dt_n their fp32 differences,
// sqdt = sqrtf(tau_p / n_steps); the state is fp32 and the step is the
// reference-order, non-contracted step of sde.hpp.
//
// Layout.  A thread owns (sample k, coordinate d) and carries the state -- and
// the tangent J when delta is asked for -- of a tile of MC_PT points in
// registers: one Philox block + Box-Muller per four steps serves all of them.
// Per-point dt_n / sqdt come from a small table (mc_grid_kernel) through
// wave-uniform loads.  A 256-thread workgroup holds S = min(32, 256 / nd)
// samples side by side (nd = D, or k for Heston); it owns one chunk of the
// samples (grid.y) and one tile of points (grid.x).  After the last step each
// thread puts its payoff term (X or X^2 of the g_cols columns) into LDS, thread
// (sample, point) sums a sample's nd terms in a fixed order, forms g and
// dg/da in fp64 and accumulates sum g, sum g^2; the (k, d) threads accumulate
// dg/dX_d J_d in fp64 registers.  At the end of the chunk the S samples are
// summed in LDS in a fixed order into the partials buffer
// [P][chunks][2 (+ D)] (hipMallocAsync); mc_final_kernel sums the chunks in
// order.  No floating-point atomics: the result is bitwise repeatable, and a
// point's result depends on neither P nor its index (the chunking is a
// function of mc and nd alone, the slots of a tile run the same code).
// nd > 256 (S = 1): a thread runs its coordinates d = tid + 256 j one after
// the other; with delta it runs them a second time once dg/da is known and
// accumulates into its own partials slots.
// Correlated (DIAG, nb <= 128): the lower triangle of L sits packed in LDS
// (33 KB); per four-step block the workgroup's normals Z [nd][4 S] go through
// LDS, L . Z runs as v_mfma_f32_16x16x4_f32 tiles over the four waves (the
// lower triangle only) and returns through LDS to the (k, d) threads: one
// product per four steps, shared by the tile's points and scaled by each
// point's sqdt afterwards.
// Nothing per path goes to HBM, but for the increments of the
// correlated Heston (DBSDE_PROB_HESTON_CORR, L [k, k] between the assets'
// Brownian motions), two passes at every k <= 511, as the correlated Heston
// rollout (paths.hpp): pass 1 is that rollout's increment GEMM
// rollout_corrw_kernel over samples as paths (mc_corr_increments, rollout.hip)
// writing the UNSCALED L z [samples, n_steps, k] to a workspace -- the points of
// a call share them and scale by their own sqdt, as CORR does; pass 2 is
// mc_kernel<MC_HESTON, false, true>: kind HESTON's path with the four normals of
// a Philox block loaded from column d of the sample's workspace rows (adjacent
// d coalesce) instead of drawn.  The workspace is bounded (DBSDE_MC_WS_MB, read
// per call): the sample chunks (grid.y) run in groups whose increments fit it,
// pass 1 then pass 2 on the group's grid.y sub-range (McArgs::ch0), a chunk
// larger than the bound as a group of its own; mc_final_kernel runs once after
// the last group.  per and nch do not depend on the grouping, and a chunk's
// partials do not depend on its group, so neither do the bits of the result.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <string>

#define DBSDE_DEVICE_HELPERS_ONLY
#include "ctx.hpp"
#include "philox.hpp"
#include "sde.hpp"

// rollout.hip
int mc_corr_increments(dbsde_ctx* pc, hipStream_t s, const float* Lt, int k, int n_steps, unsigned long long seed,
                       unsigned long long offset, long long k0, long long count, float* ws);

namespace dbsde {

constexpr int MC_PT = 8;           // points per thread tile
constexpr int MC_THREADS = 256;
constexpr int MC_SMAX = MC_THREADS / MC_PT;   // samples per workgroup pass (one reducing thread per (sample, point))
constexpr int MC_CHUNKS = 256;     // sample chunks (grid.y) at most
constexpr int MC_DMAX = 4096;
constexpr int MC_NBMAX = 128;      // correlated: L in LDS
constexpr int MC_LPACK = MC_NBMAX * (MC_NBMAX + 1) / 2;
constexpr int MC_HCMAX = 511;      // correlated Heston: dbsde_set_corr's limit for Heston contexts
constexpr int MC_WS_MB = 1024;     // correlated Heston: default workspace bound (DBSDE_MC_WS_MB)
constexpr int MC_ZMAX = 2048;       // correlated: floats of the Z (and C) tile, nd x (4 S padded to 16) <= 2048
enum {
  MC_DIAG = 0, MC_CORR = 1, MC_HESTON = 2, MC_HESTON2 = 3, MC_ASIAN = 4, MC_ASIAN_CORR = 5,
  MC_GEO_ASIAN = 6, MC_GEO_ASIAN_CORR = 7
};
// the kinds whose increments go through the L . Z product, the running-average kinds (state
// [A or G, S_1..S_k], a time integral per asset), and the geometric ones among those
constexpr bool mc_geo(int kind) { return kind == MC_GEO_ASIAN || kind == MC_GEO_ASIAN_CORR; }
constexpr bool mc_corr(int kind) { return kind == MC_CORR || kind == MC_ASIAN_CORR || kind == MC_GEO_ASIAN_CORR; }
constexpr bool mc_asian(int kind) { return kind == MC_ASIAN || kind == MC_ASIAN_CORR || mc_geo(kind); }

typedef float mcf4 __attribute__((ext_vector_type(4)));

struct McArgs {
  int D, nd, P, Ppad, n_steps;
  int S, nj, nch, W;               // samples per pass, coordinate passes, chunks, partials row width
  int g_kind, gcols;
  float strike, g_alpha, phi_r, T;
  float mu, sig_a, sig_b;          // DIAG: mu = mu_eff
  float kappa, theta, hsig, rho;   // Heston (mu = mu_a)
  float rhob;                      // two-factor Heston: fp32(sqrt(1 - (double)rho^2))
  long long mc, per;               // samples, samples per chunk
  unsigned long long seed, offset;
  const float* t;                  // [P]
  const float* x;                  // [P, D]
  const float* L;                  // [nd, nd] or null
  float* dtab;                     // [n_steps, Ppad]
  float* sqdt;                     // [Ppad]
  float* Lp;                       // packed lower triangle of L^T: row j holds L[d][j], d = j .. nd - 1
  double* part;                    // [P, nch, W]
  // correlated Heston (mc_kernel WS)
  float* Lt;                       // L^T [nd][nd], zero where L's upper triangle is (rollout_corrw_kernel's operand)
  const float* ws;                 // the group's unscaled increments L z [samples, n_steps, nd]
  long long ws_k0;                 // its first sample
  int ch0;                         // its first chunk: workgroup row blockIdx.y runs chunk ch0 + blockIdx.y
  // knock-out (mc_barrier_kernel): barrier_hit's B and gsign, barrier_stat's mean
  float bar_B, bar_gsign;
  int bar_mean;
};

__device__ __forceinline__ int mc_lp_off(int j, int nd) { return j * nd - (j * (j - 1)) / 2; }

// per-point time grid (tau <= 0: a zero grid, the state stays at x) and the
// packed L
__global__ void __launch_bounds__(256) mc_grid_kernel(McArgs a) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid < a.Ppad) {
    const int pc = gid < a.P ? gid : a.P - 1;
    const float tau = rn_sub(a.T, a.t[pc]);
    const bool run = tau > 0.f;
    const double dt64 = run ? (double)tau / (double)a.n_steps : 0.0;
    a.sqdt[gid] = run ? sqrtf(tau / (float)a.n_steps) : 0.f;
    double tacc = 0.0;
    float t0 = 0.f;
    for (int n = 0; n < a.n_steps; ++n) {
      tacc += dt64;
      const float t1 = (float)tacc;
      a.dtab[(size_t)n * a.Ppad + gid] = rn_sub(t1, t0);
      t0 = t1;
    }
  }
  if (a.L)
    for (int e = gid; e < a.nd * a.nd; e += gridDim.x * 256) {
      const int d = e / a.nd, j = e - d * a.nd;
      if (a.Lp && j <= d) a.Lp[mc_lp_off(j, a.nd) + d - j] = a.L[e];
      if (a.Lt) a.Lt[(size_t)j * a.nd + d] = j <= d ? a.L[e] : 0.f;
    }
}

__device__ __forceinline__ bool mc_squares(int g_kind) { return g_kind == DBSDE_G_SUMSQ || g_kind == DBSDE_G_LOG; }

// g and dg/d(sum) from the sum of the payoff terms (X or X^2) of a sample;
// dg/dX_d = gp * (2 X_d or 1).  The call payoffs use 1/2 at a == 0, as bs_call
// (evals.hip) does.  A put is its call in -a with gp negated: -1/2 at the kink.
__device__ __forceinline__ void mc_payoff(int g_kind, double s, double cols, double K, double alpha, double& g,
                                          double& gp) {
  if (g_kind == DBSDE_G_SUMSQ) {
    g = s;
    gp = 1.0;
  } else if (g_kind == DBSDE_G_LOG) {
    const double q = 0.5 + 0.5 * s;
    g = log(q);
    gp = 0.5 / q;
  } else if (g_kind == DBSDE_G_SMOOTH_CALL || g_kind == DBSDE_G_SMOOTH_PUT) {
    const double sgn = g_kind == DBSDE_G_SMOOTH_PUT ? -1.0 : 1.0;
    const double a = sgn * (s / cols - K), sg = 1.0 / (1.0 + exp(-alpha * a));
    g = a * sg;
    gp = sgn * ((sg + a * alpha * sg * (1.0 - sg)) / cols);
  } else {
    const double sgn = g_kind >= DBSDE_G_PUT_SUM ? -1.0 : 1.0;
    const double c = (g_kind == DBSDE_G_CALL_MEAN || g_kind == DBSDE_G_PUT_MEAN) ? cols : 1.0;
    const double a = sgn * (s / c - K);
    g = a > 0.0 ? a : 0.0;
    gp = sgn * ((a > 0.0 ? 1.0 : (a == 0.0 ? 0.5 : 0.0)) / c);
  }
}

// The whole path of sample k, thread coordinate d, for the tile's MC_PT
// points.  DIAG / CORR: X the state, V the tangent J (DELTA).  HESTON / HESTON2: X = S_d,
// V = v_d.  s: the thread's sample slot, act: the thread owns a (sample,
// coordinate) pair.  Every thread of the workgroup calls this (CORR has
// barriers inside).  WS (correlated Heston): wz is column d of the sample's
// workspace rows [n_steps][nd], null for a thread without a live pair.
template <int KIND, bool DELTA, bool WS>
__device__ __forceinline__ void mc_path(const McArgs& a, uint32_t k, int d, int s, bool act, int p0,
                                        const float (&sq)[MC_PT], float (&X)[MC_PT], float (&V)[MC_PT], float* zs,
                                        const float* Ls, const float* wz, double (&AI)[MC_PT], double (&AJ)[MC_PT]) {
  for (int n0 = 0; n0 < a.n_steps; n0 += 4) {
    float z[4];
    if constexpr (WS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) z[i] = (wz && n0 + i < a.n_steps) ? wz[(size_t)(n0 + i) * a.nd] : 0.f;
    } else {
      philox_normal4(a.seed, a.offset, k, (uint32_t)(n0 >> 2), (uint32_t)d, z);
    }
    float zv[4] = {0.f, 0.f, 0.f, 0.f};   // two-factor Heston: the normals of W^v_d, coordinate nd + d
    if constexpr (KIND == MC_HESTON2) philox_normal4(a.seed, a.offset, k, (uint32_t)(n0 >> 2), (uint32_t)(a.nd + d), zv);
    if constexpr (mc_corr(KIND)) {
      // dW^T = L . Z on the matrix cores.  Z [nd][NCp]: row j = coordinate, column
      // 4 s + i = step i of sample slot s (NCp = the 4 S columns padded to 16).
      // One v_mfma_f32_16x16x4_f32 per (16-row block o of L, 16-column block cb,
      // K-step t): A = L[16 o + cl][4 t + q] from the packed triangle, B =
      // Z[4 t + q][16 cb + cl]; L is lower triangular, so block o stops at
      // t < 4 o + 4.  Tiles go round-robin over the four waves; the products
      // C [nd][NCp] return through LDS to the (sample, coordinate) threads.
      const int NC = 4 * a.S, NCp = (NC + 15) & ~15;
      float* cs = zs + MC_ZMAX;
      if (act) *(mcf4*)(zs + d * NCp + 4 * s) = mcf4{z[0], z[1], z[2], z[3]};
      __syncthreads();
      {
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int lane = threadIdx.x & 63, cl = lane & 15, q = lane >> 4;
        const int ncb = NCp >> 4, ntile = ((a.nd + 15) >> 4) * ncb, nt4 = (a.nd + 3) >> 2;
        for (int tl = wave; tl < ntile; tl += MC_THREADS / 64) {
          const int o = tl / ncb, cb = tl - o * ncb;
          const int drow = 16 * o + cl, col = 16 * cb + cl;
          const int tmax = 4 * o + 4 < nt4 ? 4 * o + 4 : nt4;
          const bool rok = drow < a.nd, cok = col < NC;
          auto la = [&](int t) {   // k <= drow < nd: inside the packed triangle
            const int k = 4 * t + q;
            return (rok && k <= drow) ? Ls[mc_lp_off(k, a.nd) + drow - k] : 0.f;
          };
          auto zb = [&](int t) {
            const int k = 4 * t + q;
            return (cok && k < a.nd) ? zs[k * NCp + col] : 0.f;
          };
          mcf4 acc0 = mcf4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;   // two chains: the accumulator latency
          int t = 0;
          for (; t + 1 < tmax; t += 2) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(la(t), zb(t), acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(la(t + 1), zb(t + 1), acc1, 0, 0, 0);
          }
          if (t < tmax) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(la(t), zb(t), acc0, 0, 0, 0);
          acc0 += acc1;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * o + 4 * q + r;
            if (row < a.nd) cs[row * NCp + col] = acc0[r];
          }
        }
      }
      __syncthreads();
      const mcf4 c = *(const mcf4*)(cs + d * NCp + 4 * s);
#pragma unroll
      for (int i = 0; i < 4; ++i) z[i] = c[i];
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (n0 + kk >= a.n_steps) break;
      const float* dtr = a.dtab + (size_t)(n0 + kk) * a.Ppad + p0;   // wave-uniform
#pragma unroll
      for (int i = 0; i < MC_PT; ++i) {
        const float dt = dtr[i];
        const float w = rn_mul(sq[i], z[kk]);
        if constexpr (KIND == MC_HESTON2) {
          float sa, sb;
          heston2_step(a.mu, a.kappa, a.theta, a.hsig, a.rho, a.rhob, dt, w, rn_mul(sq[i], zv[kk]), X[i], V[i], sa, sb);
        } else if constexpr (KIND == MC_HESTON) {
          float sa, sb;
          heston_step(heston_coef(a.mu, a.kappa, a.theta, a.hsig, a.rho, X[i], V[i]), dt, w, X[i], V[i], sa, sb);
        } else {
          if constexpr (mc_asian(KIND)) {   // the left-point rule: S (and J) at the start of the step
            if constexpr (mc_geo(KIND)) {
              AI[i] += (double)rn_mul(geo_lg(X[i]), dt);
              if constexpr (DELTA) AJ[i] += (double)rn_mul(V[i] / X[i], dt);
            } else {
              AI[i] += (double)rn_mul(X[i], dt);
              if constexpr (DELTA) AJ[i] += (double)rn_mul(V[i], dt);
            }
          }
          diag_step(a.mu, a.sig_a, a.sig_b, dt, w, X[i]);
          if constexpr (DELTA) diag_tangent_step(a.mu, a.sig_a, dt, w, V[i]);
        }
      }
    }
  }
  if constexpr (mc_corr(KIND)) __syncthreads();   // the C tile shares LDS with what the caller writes next
}

template <int KIND, bool DELTA, bool WS = false>
__global__ void __launch_bounds__(MC_THREADS) mc_kernel(McArgs a) {
  static_assert(!WS || (KIND == MC_HESTON && !DELTA), "the workspace increments are the correlated Heston's");
  __shared__ __attribute__((aligned(16))) double fred[MC_PT * MC_THREADS];
  __shared__ float gpl[MC_THREADS];
  // correlated: Z and C of mc_path share fred's 16 KB (fred is written only after a
  // path's last barrier and read before the next path's first)
  static_assert(sizeof(fred) >= 2 * MC_ZMAX * sizeof(float), "Z and C tiles must fit fred");
  float* zs = reinterpret_cast<float*>(fred);
  __shared__ float Ls[mc_corr(KIND) ? MC_LPACK : 1];
  const int tid = threadIdx.x;
  int ch = blockIdx.y;
  if constexpr (WS) ch += a.ch0;
  const int p0 = blockIdx.x * MC_PT;
  const int nd = a.nd, S = a.S, nj = a.nj;
  if constexpr (mc_corr(KIND))
    for (int e = tid; e < nd * (nd + 1) / 2; e += MC_THREADS) Ls[e] = a.Lp[e];   // read after mc_path's first barrier
  const bool act = nj > 1 || tid < S * nd;
  const int s = (act && nj == 1) ? tid / nd : 0;
  const int d0 = act ? (nj > 1 ? tid : tid - s * nd) : 0;
  const int RW = nj > 1 ? MC_THREADS : nd;            // LDS entries of one sample's payoff terms
  const int rs = tid / MC_PT, ri = tid - rs * MC_PT;  // reducing role: sample slot rs, point slot ri
  const bool reducer = rs < S;
  const bool squares = mc_squares(a.g_kind);
  const double cols = (double)a.gcols, K = (double)a.strike, alpha = (double)a.g_alpha;
  // arithmetic average: the state columns are [A, S_1..S_nd], a sample's payoff terms are the
  // time integrals I_d of its assets, and A_T = A_p + (sum_d I_d) / (nd T)
  constexpr bool ASIAN = mc_asian(KIND);
  constexpr bool GEO = mc_geo(KIND);   // [G, S_1..S_nd]: G_T = G_p exp((sum_d I_d) / (nd T)), I_d over lg(S_d)
  constexpr int XO = ASIAN ? 1 : 0;
  const double akt = (double)nd * (double)a.T;
  float sq[MC_PT];
  int pc[MC_PT];
#pragma unroll
  for (int i = 0; i < MC_PT; ++i) {
    sq[i] = a.sqdt[p0 + i];
    pc[i] = p0 + i < a.P ? p0 + i : a.P - 1;
  }
  const long long k0 = (long long)ch * a.per, k1 = k0 + a.per < a.mc ? k0 + a.per : a.mc;
  double gs = 0.0, g2 = 0.0;
  double gps = 0.0;   // ASIAN with DELTA: sum of dg/dA_T, the A column of delta
  double dacc[MC_PT];
#pragma unroll
  for (int i = 0; i < MC_PT; ++i) dacc[i] = 0.0;

  for (long long kb = k0; kb < k1; kb += S) {
    const long long kk = kb + s;
    const bool live = act && kk < k1;
    float X[MC_PT], V[MC_PT];
    double fs[MC_PT];
    double AI[MC_PT], AJ[MC_PT];   // ASIAN: sum_n fp32(S_n dt_n) and sum_n fp32(J_n dt_n) of the thread's asset
#pragma unroll
    for (int i = 0; i < MC_PT; ++i) fs[i] = 0.0;
    for (int j = 0; j < nj; ++j) {
      const int d = d0 + MC_THREADS * j;
      const bool dl = live && d < nd;
      const int dd = dl ? d : 0;
#pragma unroll
      for (int i = 0; i < MC_PT; ++i) {
        X[i] = a.x[(size_t)pc[i] * a.D + XO + dd];
        V[i] = (KIND == MC_HESTON || KIND == MC_HESTON2) ? a.x[(size_t)pc[i] * a.D + nd + dd] : 1.f;
        AI[i] = AJ[i] = 0.0;
      }
      const float* wz = nullptr;
      if constexpr (WS)
        if (dl) wz = a.ws + (size_t)(kk - a.ws_k0) * a.n_steps * nd + dd;
      mc_path<KIND, DELTA, WS>(a, (uint32_t)kk, dd, s, act, p0, sq, X, V, zs, Ls, wz, AI, AJ);
      if (dl) {
#pragma unroll
        for (int i = 0; i < MC_PT; ++i) {
          if constexpr (ASIAN) {
            fs[i] += AI[i];
            continue;
          }
          if (dd < a.gcols) fs[i] += squares ? (double)X[i] * (double)X[i] : (double)X[i];
          if ((KIND == MC_HESTON || KIND == MC_HESTON2) && nd + dd < a.gcols)
            fs[i] += squares ? (double)V[i] * (double)V[i] : (double)V[i];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < MC_PT; ++i) fred[i * MC_THREADS + tid] = fs[i];
    __syncthreads();
    if (reducer) {
      const double* fr = fred + ri * MC_THREADS + rs * RW;
      double sum = 0.0;
      for (int e = 0; e < RW; ++e) sum += fr[e];
      double gfac = 1.0;   // GEO: G_T / G_p = dG_T / dG_p
      if constexpr (GEO) {
        gfac = exp(sum / akt);
        sum = (double)a.x[(size_t)(p0 + ri < a.P ? p0 + ri : a.P - 1) * a.D] * gfac;   // G_T
      } else if constexpr (ASIAN) {
        sum = (double)a.x[(size_t)(p0 + ri < a.P ? p0 + ri : a.P - 1) * a.D] + sum / akt;   // A_T
      }
      double g, gp;
      mc_payoff(a.g_kind, sum, cols, K, alpha, g, gp);
      if (kb + rs < k1) {
        gs += g;
        g2 += g * g;
        if constexpr (ASIAN && DELTA) gps += GEO ? gp * gfac : gp;
      }
      gpl[tid] = GEO ? (float)(gp * sum) : (float)gp;   // GEO: dg/dG_T . G_T, the factor of every dS_d
    }
    __syncthreads();
    if constexpr (DELTA) {
      for (int j = 0; j < nj; ++j) {
        const int d = d0 + MC_THREADS * j;
        const bool dl = live && d < nd;
        const int dd = dl ? d : 0;
        if (nj > 1) {   // the coordinates of a long state are run again now that dg/da is known
#pragma unroll
          for (int i = 0; i < MC_PT; ++i) {
            X[i] = a.x[(size_t)pc[i] * a.D + XO + dd];
            V[i] = 1.f;
            AI[i] = AJ[i] = 0.0;
          }
          mc_path<KIND, DELTA, WS>(a, (uint32_t)kk, dd, s, act, p0, sq, X, V, zs, Ls, nullptr, AI, AJ);
        }
        if (!dl) continue;
#pragma unroll
        for (int i = 0; i < MC_PT; ++i) {
          const double fp = dd < a.gcols ? (squares ? 2.0 * (double)X[i] : 1.0) : 0.0;
          double v = (double)gpl[s * MC_PT + i] * fp * (double)V[i];
          if constexpr (ASIAN) v = (double)gpl[s * MC_PT + i] * (AJ[i] / akt);   // dA_T / dS_d = (sum_n J_n dt_n) / (nd T)
          if (nj == 1) {
            dacc[i] += v;
          } else if (p0 + i < a.P) {   // the thread's own slot: first sample stores, the others add
            double* q = a.part + ((size_t)(p0 + i) * a.nch + ch) * a.W + 2 + XO + dd;
            *q = kb == k0 ? v : *q + v;
          }
        }
      }
    }
  }

  // the chunk's sums over the S sample slots, fixed order
  if (reducer) {
    fred[tid] = gs;
    fred[MC_THREADS + tid] = g2;
    if constexpr (ASIAN && DELTA) fred[2 * MC_THREADS + tid] = gps;
  }
  __syncthreads();
  if (tid < MC_PT && p0 + tid < a.P) {
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int r = 0; r < S; ++r) {
      s1 += fred[r * MC_PT + tid];
      s2 += fred[MC_THREADS + r * MC_PT + tid];
      if constexpr (ASIAN && DELTA) s3 += fred[2 * MC_THREADS + r * MC_PT + tid];
    }
    double* q = a.part + ((size_t)(p0 + tid) * a.nch + ch) * a.W;
    q[0] = s1;
    q[1] = s2;
    if constexpr (ASIAN && DELTA) q[2] = s3;   // dA_T / dA_p = 1
  }
  if constexpr (DELTA) {
    if (nj == 1) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < MC_PT; ++i) fred[i * MC_THREADS + tid] = dacc[i];   // 0 from threads without a pair
      __syncthreads();
      for (int e = tid; e < MC_PT * nd; e += MC_THREADS) {
        const int i = e / nd, d = e - i * nd;
        if (p0 + i >= a.P) continue;
        double sum = 0.0;
        for (int r = 0; r < S; ++r) sum += fred[i * MC_THREADS + r * nd + d];
        a.part[((size_t)(p0 + i) * a.nch + ch) * a.W + 2 + XO + d] = sum;
      }
    }
  }
}

// value, standard error and delta of point p (blockIdx.x) from the chunk
// partials; column c = 0: value / standard error, c >= 1: delta[c - 1]
__global__ void __launch_bounds__(256) mc_final_kernel(McArgs a, float* value, float* stderr_, float* delta) {
  const int p = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c > (delta ? a.D : 0)) return;
  const float tau = rn_sub(a.T, a.t[p]);
  const float* xp = a.x + (size_t)p * a.D;
  const bool squares = mc_squares(a.g_kind);
  if (!(tau > 0.f)) {   // at maturity: g(x), 0, dg/dx
    double s = 0.0;
    for (int d = 0; d < a.gcols; ++d) s += squares ? (double)xp[d] * (double)xp[d] : (double)xp[d];
    double g, gp;
    mc_payoff(a.g_kind, s, (double)a.gcols, (double)a.strike, (double)a.g_alpha, g, gp);
    if (c == 0) {
      value[p] = (float)g;
      if (stderr_) stderr_[p] = 0.f;
    } else {
      delta[(size_t)p * a.D + c - 1] = c - 1 < a.gcols ? (float)(gp * (squares ? 2.0 * (double)xp[c - 1] : 1.0)) : 0.f;
    }
    return;
  }
  const double disc = exp(-(double)a.phi_r * (double)tau), n = (double)a.mc;
  const double* q = a.part + (size_t)p * a.nch * a.W;
  if (c == 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int h = 0; h < a.nch; ++h) {
      s1 += q[(size_t)h * a.W];
      s2 += q[(size_t)h * a.W + 1];
    }
    value[p] = (float)(disc * (s1 / n));
    if (stderr_) {
      double var = a.mc > 1 ? (s2 - s1 * s1 / n) / (n - 1.0) : 0.0;
      if (!(var > 0.0)) var = 0.0;
      stderr_[p] = (float)(disc * sqrt(var / n));
    }
  } else {
    double s1 = 0.0;
    for (int h = 0; h < a.nch; ++h) s1 += q[(size_t)h * a.W + 1 + c];
    delta[(size_t)p * a.D + c - 1] = (float)(disc * (s1 / n));
  }
}

// --------------------------------------------------------------------------
// Knock-out problems (the header comment has the layout)
// --------------------------------------------------------------------------
constexpr int MB_GROUPS = MC_THREADS / ASIAN_LANES;   // samples side by side in a workgroup
constexpr int MB_AMAX = MC_NBMAX / ASIAN_LANES;       // assets per lane

// barrier_stat over the lane's columns X[j] = coordinate l + 16 j (the columns below
// cols): asian_lane_sum's ascending partial, then the butterfly
__device__ __forceinline__ float mb_stat(const float (&X)[MB_AMAX], int l, int cols, bool mean) {
  float p = 0.f;
#pragma unroll
  for (int j = 0; j < MB_AMAX; ++j)
    if (l + ASIAN_LANES * j < cols) p = rn_add(p, X[j]);
#pragma unroll
  for (int o = 1; o < ASIAN_LANES; o <<= 1) p = rn_add(p, __shfl_xor(p, o));
  return mean ? asian_mean(p, cols) : p;
}

template <bool WS>
__global__ void __launch_bounds__(MC_THREADS) mc_barrier_kernel(McArgs a) {
  __shared__ double red[2][MB_GROUPS];
  const int tid = threadIdx.x, grp = tid / ASIAN_LANES, l = tid & (ASIAN_LANES - 1);
  const int p = blockIdx.x, nd = a.nd;
  int ch = blockIdx.y;
  if constexpr (WS) ch += a.ch0;
  const float sq = a.sqdt[p];
  const bool mean = a.bar_mean != 0;
  float x0[MB_AMAX];
#pragma unroll
  for (int j = 0; j < MB_AMAX; ++j) x0[j] = l + ASIAN_LANES * j < nd ? a.x[(size_t)p * a.D + l + ASIAN_LANES * j] : 0.f;
  const long long k0 = (long long)ch * a.per, k1 = k0 + a.per < a.mc ? k0 + a.per : a.mc;
  double gs = 0.0, g2 = 0.0;
  for (long long kb = k0; kb < k1; kb += MB_GROUPS) {
    const long long kk = kb + grp;
    if (kk >= k1) continue;   // (the group's 16 lanes agree)
    float X[MB_AMAX];
#pragma unroll
    for (int j = 0; j < MB_AMAX; ++j) X[j] = x0[j];
    bool alive = !barrier_hit(mb_stat(X, l, a.gcols, mean), a.bar_B, a.bar_gsign);   // row 0 counts
    for (int n0 = 0; n0 < a.n_steps && alive; n0 += 4) {
      float z[MB_AMAX][4];
#pragma unroll
      for (int j = 0; j < MB_AMAX; ++j) {
        const int d = l + ASIAN_LANES * j;
#pragma unroll
        for (int i = 0; i < 4; ++i) z[j][i] = 0.f;
        if (d >= nd) continue;
        if constexpr (WS) {
          const float* wz = a.ws + (size_t)(kk - a.ws_k0) * a.n_steps * nd + d;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (n0 + i < a.n_steps) z[j][i] = wz[(size_t)(n0 + i) * nd];
        } else {
          philox_normal4(a.seed, a.offset, (uint32_t)kk, (uint32_t)(n0 >> 2), (uint32_t)d, z[j]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (n0 + i >= a.n_steps || !alive) break;
        const float dt = a.dtab[(size_t)(n0 + i) * a.Ppad + p];
#pragma unroll
        for (int j = 0; j < MB_AMAX; ++j)
          if (l + ASIAN_LANES * j < nd) diag_step(a.mu, a.sig_a, a.sig_b, dt, rn_mul(sq, z[j][i]), X[j]);
        alive = !barrier_hit(mb_stat(X, l, a.gcols, mean), a.bar_B, a.bar_gsign);
      }
    }
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < MB_AMAX; ++j)
      if (l + ASIAN_LANES * j < a.gcols) sum += (double)X[j];
#pragma unroll
    for (int o = 1; o < ASIAN_LANES; o <<= 1) sum += __shfl_xor(sum, o);
    double g, gp;
    mc_payoff(a.g_kind, sum, (double)a.gcols, (double)a.strike, (double)a.g_alpha, g, gp);
    if (!alive) g = 0.0;
    gs += g;
    g2 += g * g;
  }
  if (l == 0) {
    red[0][grp] = gs;
    red[1][grp] = g2;
  }
  __syncthreads();
  if (tid == 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int r = 0; r < MB_GROUPS; ++r) {
      s1 += red[0][r];
      s2 += red[1][r];
    }
    double* q = a.part + ((size_t)p * a.nch + ch) * a.W;
    q[0] = s1;
    q[1] = s2;
  }
}

// value and standard error of point p (blockIdx.x) from the chunk partials, as
// mc_final_kernel forms them; a point at maturity gets g(x_p) and 0, or 0 and 0
// when x_p is beyond the barrier.  One wave per point: its first 16 lanes form
// barrier_stat, and g's fp64 sum runs in mc_barrier_kernel's order.
__global__ void __launch_bounds__(64) mc_barrier_final_kernel(McArgs a, float* value, float* stderr_) {
  const int p = blockIdx.x, l = threadIdx.x & (ASIAN_LANES - 1);
  const float tau = rn_sub(a.T, a.t[p]);
  const float* xp = a.x + (size_t)p * a.D;
  if (!(tau > 0.f)) {
    float X[MB_AMAX];
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < MB_AMAX; ++j) {
      X[j] = l + ASIAN_LANES * j < a.nd ? xp[l + ASIAN_LANES * j] : 0.f;
      if (l + ASIAN_LANES * j < a.gcols) sum += (double)X[j];
    }
    const bool hit = barrier_hit(mb_stat(X, l, a.gcols, a.bar_mean != 0), a.bar_B, a.bar_gsign);
#pragma unroll
    for (int o = 1; o < ASIAN_LANES; o <<= 1) sum += __shfl_xor(sum, o);
    double g, gp;
    mc_payoff(a.g_kind, sum, (double)a.gcols, (double)a.strike, (double)a.g_alpha, g, gp);
    if (threadIdx.x == 0) {
      value[p] = hit ? 0.f : (float)g;
      if (stderr_) stderr_[p] = 0.f;
    }
    return;
  }
  if (threadIdx.x != 0) return;
  const double disc = exp(-(double)a.phi_r * (double)tau), n = (double)a.mc;
  const double* q = a.part + (size_t)p * a.nch * a.W;
  double s1 = 0.0, s2 = 0.0;
  for (int h = 0; h < a.nch; ++h) {
    s1 += q[(size_t)h * a.W];
    s2 += q[(size_t)h * a.W + 1];
  }
  value[p] = (float)(disc * (s1 / n));
  if (stderr_) {
    double var = a.mc > 1 ? (s2 - s1 * s1 / n) / (n - 1.0) : 0.0;
    if (!(var > 0.0)) var = 0.0;
    stderr_[p] = (float)(disc * sqrt(var / n));
  }
}

}  // namespace dbsde

using namespace dbsde;

namespace {
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
}  // namespace

extern "C" int dbsde_mc_value(const dbsde_problem* prob, int D, float T, const float* L, const float* t,
                              const float* x, int P, int n_steps, long long mc, unsigned long long seed,
                              unsigned long long offset, float* value, float* stderr_, float* delta, void* stream) {
  auto bad = [](const std::string& m) { return fail(nullptr, DBSDE_EINVAL, "dbsde_mc_value: " + m); };
  if (!prob || !t || !x || !value) return bad("prob, t, x and value must not be NULL");
  if (P < 1 || D < 1 || n_steps < 1 || mc < 1) return bad("P, D, n_steps and mc must be >= 1");
  if (mc > (1LL << 32)) return bad("mc must be <= 2^32 (the sample index is a 32-bit counter word)");
  if (D > MC_DMAX) return bad("D must be <= 4096");
  if (prob->kind != DBSDE_PROB_DIAG && prob->kind != DBSDE_PROB_HESTON && prob->kind != DBSDE_PROB_HESTON2 &&
      prob->kind != DBSDE_PROB_HESTON_CORR && prob->kind != DBSDE_PROB_ASIAN && prob->kind != DBSDE_PROB_GEO_ASIAN &&
      prob->kind != DBSDE_PROB_BARRIER)
    return bad("unknown problem kind");
  if (prob->g_kind < DBSDE_G_SUMSQ || prob->g_kind > DBSDE_G_SMOOTH_PUT) return bad("unknown terminal condition g_kind");
  if (prob->phi_zz != 0.f)
    return bad("phi_zz != 0 is not a linear problem (no Feynman-Kac expectation); the HJB comparator is dbsde_hjb_mc");
  if (prob->pen != 0.f)
    return bad("pen != 0 is not a linear problem (no Feynman-Kac expectation); the arbiter of the penalised American "
               "put is dbsde_exact's DBSDE_EXACT_AMERICAN_PUT");
  const bool heston2 = prob->kind == DBSDE_PROB_HESTON2;   // the same state and the same refusals
  const bool hcorr = prob->kind == DBSDE_PROB_HESTON_CORR;   // kind HESTON's process, its assets correlated by L
  const bool heston = prob->kind == DBSDE_PROB_HESTON || heston2 || hcorr;
  if (hcorr && !L) return bad("DBSDE_PROB_HESTON_CORR needs the factor L [k, k] (independent assets: DBSDE_PROB_HESTON)");
  if (heston && (D & 1)) return bad("the Heston state [S_1..S_k, v_1..v_k] needs an even D");
  if (heston && !hcorr && L)
    return bad("L applies to DIAG problems only (correlated Heston assets: DBSDE_PROB_HESTON_CORR)");
  if (heston && delta)
    return bad("no pathwise delta for Heston (the S and v tangents couple); bump and reprice on the same draws");
  if (hcorr && D / 2 > MC_HCMAX) return bad("correlated Heston needs k = D / 2 <= 511");
  if (hcorr && (n_steps + 3) / 4 > 65535) return bad("correlated Heston needs n_steps <= 262140");
  // arithmetic average: state [A, S_1..S_k], the DIAG process on the k = D - 1 assets, payoff on A
  // geometric average: state [G, S_1..S_k], the same layout (asian is set too)
  const bool geo = prob->kind == DBSDE_PROB_GEO_ASIAN;
  const bool asian = prob->kind == DBSDE_PROB_ASIAN || geo;
  if (asian) {
    if (const char* why = geo ? geo_asian_refusal(*prob, D) : asian_refusal(*prob, D)) return bad(why);
    if (L && D - 1 > MC_NBMAX) return bad("L needs D - 1 <= 128 assets");
  }
  if (!hcorr && !asian && L && D > MC_NBMAX) return bad("L needs D <= 128");
  // knock-out: DIAG's state and step, a kernel of its own (a 16-lane group per sample)
  const bool barrier = prob->kind == DBSDE_PROB_BARRIER;
  if (barrier) {
    if (const char* why = barrier_refusal(*prob)) return bad(why);
    if (D > MC_NBMAX) return bad("the barrier problem needs D <= 128 (a 16-lane group holds a sample's assets)");
    if (delta)
      return bad("no pathwise delta for the barrier problem (the estimator is biased across the knock-out "
                 "indicator); bump and reprice on the same draws");
    if (L && (n_steps + 3) / 4 > 65535) return bad("the barrier problem with L needs n_steps <= 262140");
  }
  const bool wsinc = hcorr || (barrier && L);   // increments from the workspace the increment GEMM fills

  McArgs a{};
  a.D = D;
  a.nd = heston ? D / 2 : (asian ? D - 1 : D);
  a.P = P;
  const int tiles = (P + MC_PT - 1) / MC_PT;
  a.Ppad = tiles * MC_PT;
  a.n_steps = n_steps;
  a.nj = a.nd > MC_THREADS ? (a.nd + MC_THREADS - 1) / MC_THREADS : 1;
  a.S = a.nj > 1 ? 1 : (MC_THREADS / a.nd < MC_SMAX ? MC_THREADS / a.nd : MC_SMAX);
  if (barrier) a.S = MB_GROUPS;   // a function of nothing: the chunking depends on mc alone
  const long long per0 = (mc + MC_CHUNKS - 1) / MC_CHUNKS;
  a.per = (per0 + a.S - 1) / a.S * a.S;
  a.nch = (int)((mc + a.per - 1) / a.per);
  a.W = 2 + (delta ? D : 0);
  a.g_kind = prob->g_kind;
  a.gcols = prob->g_cols > 0 && prob->g_cols < D ? prob->g_cols : D;   // (ASIAN: 1, the A column)
  a.strike = prob->strike;
  a.g_alpha = prob->g_alpha;
  a.phi_r = prob->phi_r;
  a.T = T;
  volatile float fold = prob->phi_r * prob->phi_c;   // rounded on its own, then added
  a.mu = heston ? prob->mu_a : prob->mu_a + fold;
  a.sig_a = prob->sig_a;
  a.sig_b = prob->sig_b;
  a.kappa = prob->h_kappa;
  a.theta = prob->h_theta;
  a.hsig = prob->h_sigma;
  a.rho = prob->h_rho;
  if (heston2 && !(std::fabs((double)prob->h_rho) <= 1.0)) return bad("two-factor Heston needs |h_rho| <= 1");
  a.rhob = heston2 ? (float)std::sqrt(1.0 - (double)prob->h_rho * (double)prob->h_rho) : 0.f;
  a.mc = mc;
  a.seed = seed;
  a.offset = offset;
  a.t = t;
  a.x = x;
  a.L = L;
  a.bar_B = prob->h_kappa;
  a.bar_gsign = prob->g_kind >= DBSDE_G_PUT_SUM ? -1.f : 1.f;
  a.bar_mean = prob->g_kind == DBSDE_G_CALL_MEAN || prob->g_kind == DBSDE_G_PUT_MEAN;

  hipStream_t st = (hipStream_t)stream;
  const size_t b_part = up256((size_t)P * a.nch * a.W * sizeof(double));
  const size_t b_dtab = up256((size_t)n_steps * a.Ppad * sizeof(float));
  const size_t b_sq = up256((size_t)a.Ppad * sizeof(float));
  const size_t b_lp = wsinc ? up256((size_t)a.nd * a.nd * sizeof(float)) : L ? up256((size_t)MC_LPACK * sizeof(float)) : 0;
  // correlated Heston (and the knock-out kind with L): the chunks of a group and its workspace
  int cg = a.nch;
  size_t b_ws = 0;
  if (wsinc) {
    const char* e = getenv("DBSDE_MC_WS_MB");
    const double mb = e ? atof(e) : 0.0;   // megabytes, fractions allowed; unset or not positive: the default
    const double chunk = (double)a.per * n_steps * a.nd * sizeof(float);
    const double fit = (mb > 0.0 ? mb : (double)MC_WS_MB) * 1048576.0 / chunk;
    cg = fit < 1.0 ? 1 : (fit < (double)a.nch ? (int)fit : a.nch);
    const long long rows = std::min<long long>((long long)cg * a.per, mc);
    b_ws = up256((size_t)rows * n_steps * a.nd * sizeof(float));
  }
  char* buf = nullptr;
  if (hipMallocAsync((void**)&buf, b_part + b_dtab + b_sq + b_lp + b_ws, st) != hipSuccess)
    return fail(nullptr, DBSDE_ENOMEM, "dbsde_mc_value: hipMallocAsync failed");
  a.part = (double*)buf;
  a.dtab = (float*)(buf + b_part);
  a.sqdt = (float*)(buf + b_part + b_dtab);
  a.Lp = L && !wsinc ? (float*)(buf + b_part + b_dtab + b_sq) : nullptr;
  a.Lt = wsinc ? (float*)(buf + b_part + b_dtab + b_sq) : nullptr;

  mc_grid_kernel<<<(a.Ppad + 255) / 256, 256, 0, st>>>(a);
  const dim3 grid(tiles, a.nch);
  if (wsinc) {
    dbsde_ctx* pc = free_call_ctx();
    if (pc->prof) pc->stream = st;   // what dbsde_profile_read(NULL, ...) synchronises
    a.ws = (const float*)(buf + b_part + b_dtab + b_sq + b_lp);
    int rc = DBSDE_OK;
    for (int c0 = 0; c0 < a.nch && rc == DBSDE_OK; c0 += cg) {
      const int nc = std::min(cg, a.nch - c0);
      a.ch0 = c0;
      a.ws_k0 = (long long)c0 * a.per;
      const long long count = std::min<long long>((long long)nc * a.per, mc - a.ws_k0);
      rc = mc_corr_increments(pc, st, a.Lt, a.nd, n_steps, seed, offset, a.ws_k0, count, (float*)a.ws);
      if (rc == DBSDE_OK && barrier)
        rc = run(pc, st, "mc_barrier_paths", 0.0, 4.0 * (double)count * n_steps * a.nd * P, [&]() {
          mc_barrier_kernel<true><<<dim3(P, nc), MC_THREADS, 0, st>>>(a);
        });
      else if (rc == DBSDE_OK)
        rc = run(pc, st, "mc_heston_corr_paths", 0.0, 4.0 * (double)count * n_steps * a.nd * tiles, [&]() {
          mc_kernel<MC_HESTON, false, true><<<dim3(tiles, nc), MC_THREADS, 0, st>>>(a);
        });
    }
    if (rc != DBSDE_OK) {
      (void)hipFreeAsync(buf, st);
      return rc;
    }
  } else if (barrier)
    mc_barrier_kernel<false><<<dim3(P, a.nch), MC_THREADS, 0, st>>>(a);
  else if (heston2)
    mc_kernel<MC_HESTON2, false><<<grid, MC_THREADS, 0, st>>>(a);
  else if (heston)
    mc_kernel<MC_HESTON, false><<<grid, MC_THREADS, 0, st>>>(a);
  else if (geo && L && delta)
    mc_kernel<MC_GEO_ASIAN_CORR, true><<<grid, MC_THREADS, 0, st>>>(a);
  else if (geo && L)
    mc_kernel<MC_GEO_ASIAN_CORR, false><<<grid, MC_THREADS, 0, st>>>(a);
  else if (geo && delta)
    mc_kernel<MC_GEO_ASIAN, true><<<grid, MC_THREADS, 0, st>>>(a);
  else if (geo)
    mc_kernel<MC_GEO_ASIAN, false><<<grid, MC_THREADS, 0, st>>>(a);
  else if (asian && L && delta)
    mc_kernel<MC_ASIAN_CORR, true><<<grid, MC_THREADS, 0, st>>>(a);
  else if (asian && L)
    mc_kernel<MC_ASIAN_CORR, false><<<grid, MC_THREADS, 0, st>>>(a);
  else if (asian && delta)
    mc_kernel<MC_ASIAN, true><<<grid, MC_THREADS, 0, st>>>(a);
  else if (asian)
    mc_kernel<MC_ASIAN, false><<<grid, MC_THREADS, 0, st>>>(a);
  else if (L && delta)
    mc_kernel<MC_CORR, true><<<grid, MC_THREADS, 0, st>>>(a);
  else if (L)
    mc_kernel<MC_CORR, false><<<grid, MC_THREADS, 0, st>>>(a);
  else if (delta)
    mc_kernel<MC_DIAG, true><<<grid, MC_THREADS, 0, st>>>(a);
  else
    mc_kernel<MC_DIAG, false><<<grid, MC_THREADS, 0, st>>>(a);
  if (barrier)
    mc_barrier_final_kernel<<<P, 64, 0, st>>>(a, value, stderr_);
  else
    mc_final_kernel<<<dim3(P, ((delta ? D : 0) + 256) / 256), 256, 0, st>>>(a, value, stderr_, delta);
  const hipError_t e = hipGetLastError();
  (void)hipFreeAsync(buf, st);
  if (e != hipSuccess) return fail(nullptr, DBSDE_EHIP, std::string("dbsde_mc_value: ") + hipGetErrorString(e));
  return DBSDE_OK;
}
