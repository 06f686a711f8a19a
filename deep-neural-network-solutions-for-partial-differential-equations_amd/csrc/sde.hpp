// sde.hpp -- the one definition of each process's Euler-Maruyama step.
//
// Every path kernel (paths.hpp), the Monte-Carlo comparator (mc.hip) and the
// Heston coefficients of the PDE residual (jet.hip) take their step from here,
// so X is the numpy oracle's bit for bit (oracle/philox.py,
// tests/heston2_reference.py) and every rollout form equals every other.  Each
// product and sum is rounded on its own (rn.hpp), the square root is correctly
// rounded (hipcc's default for fp32), c = clamp100.  The header is plain C++
// without hipcc, and tests/test_sde_step_cpu.py checks these functions against
// the oracles on a CPU.
#pragma once
#include <stddef.h>

#include "rn.hpp"

namespace dbsde {

// Diagonal problems (DeepBSDE.py:218-222 with mu = mu_a X, sigma = diag(sig_a X
// + sig_b); sigma (x) dW is bit-identical to the dense bmm):
//   s = (sig_a x + sig_b) dw,   x <- (x + (mu_a x) dt) + s
// returns s, the sdw entry of the row x came from
DBSDE_HD float diag_step(float mu_a, float sig_a, float sig_b, float dt, float dw, float& x) {
  const float s = rn_mul(rn_add(rn_mul(sig_a, x), sig_b), dw);
  x = rn_add(rn_add(x, rn_mul(rn_mul(mu_a, x), dt)), s);
  return s;
}

// the tangent J = dx / dx_0 of that step (sig_b drops out)
DBSDE_HD void diag_tangent_step(float mu_a, float sig_a, float dt, float dw, float& J) {
  J = rn_add(rn_add(J, rn_mul(rn_mul(mu_a, J), dt)), rn_mul(rn_mul(sig_a, J), dw));
}

// What the two Heston models share at a state (S, v) of one asset: the drifts
//   muS = c(mu_a S),   muV = c(kappa (theta - v))
// and, with sv = sqrt(max(v, 1e-8)), sigS = sv S, sigV = sig sv (unclamped) and
// d00 = c(sigS).
DBSDE_HD float heston_mu_s(float mu_a, float S) { return clamp100(rn_mul(mu_a, S)); }
DBSDE_HD float heston_mu_v(float kappa, float theta, float v) { return clamp100(rn_mul(kappa, rn_sub(theta, v))); }
struct HestonBase {
  float muS, muV, sigS, sigV, d00;
};
DBSDE_HD HestonBase heston_base(float mu_a, float kappa, float theta, float hsig, float S, float v) {
  HestonBase b;
  b.muS = heston_mu_s(mu_a, S);
  b.muV = heston_mu_v(kappa, theta, v);
  const float sv = sqrtf(fmaxf(v, 1e-8f));
  b.sigS = rn_mul(sv, S);
  b.sigV = rn_mul(hsig, sv);
  b.d00 = clamp100(b.sigS);
  return b;
}

// k-asset Heston (heston_dnnpde.py:587-605, 629-642): one scalar Brownian
// motion per asset drives both S and v (the reference's FBSNN dimension is 1
// and einsum broadcasts dW over the two state components).
//   Sig = c([[sv S, rho sig sv], [rho sv S, sig sv]]) = [[d00, d01], [d10, d11]]
//   a = d00 w + d01 w,   b = d10 w + d11 w       (the Y-tilde term, :641-642)
//   S <- (S + muS dt) + (d00 + d01) w,   v <- (v + muV dt) + (d10 + d11) w
//                                                (einsum sums over j first)
struct HestonCoef {
  float muS, muV, d00, d01, d10, d11;
};
DBSDE_HD HestonCoef heston_coef(float mu_a, float kappa, float theta, float hsig, float rho, float S, float v) {
  const HestonBase b = heston_base(mu_a, kappa, theta, hsig, S, v);
  return HestonCoef{b.muS, b.muV, b.d00, clamp100(rn_mul(rho, b.sigV)), clamp100(rn_mul(rho, b.sigS)), clamp100(b.sigV)};
}
// a and b are the sdw entries of the S and v columns
DBSDE_HD void heston_step(const HestonCoef& c, float dt, float w, float& S, float& v, float& a, float& b) {
  a = rn_add(rn_mul(c.d00, w), rn_mul(c.d01, w));
  b = rn_add(rn_mul(c.d10, w), rn_mul(c.d11, w));
  S = rn_add(rn_add(S, rn_mul(c.muS, dt)), rn_mul(rn_add(c.d00, c.d01), w));
  v = rn_add(rn_add(v, rn_mul(c.muV, dt)), rn_mul(rn_add(c.d10, c.d11), w));
}

// Two-factor Heston (DBSDE_PROB_HESTON2, include/dbsde.h): the textbook model,
// w1 / w2 the increments of W^S and W^v, rhob = fp32(sqrt(1 - (double)rho^2)):
//   d10 = c(rho sigV),   d11 = c(rhob sigV)
//   a = d00 w1,   b = d10 w1 + d11 w2            (the sdw columns S, v)
//   S <- (S + muS dt) + a,   v <- (v + muV dt) + b
struct Heston2Coef {
  float muS, muV, d00, d10, d11;
};
DBSDE_HD Heston2Coef heston2_coef(float mu_a, float kappa, float theta, float hsig, float rho, float rhob, float S,
                                  float v) {
  const HestonBase b = heston_base(mu_a, kappa, theta, hsig, S, v);
  return Heston2Coef{b.muS, b.muV, b.d00, clamp100(rn_mul(rho, b.sigV)), clamp100(rn_mul(rhob, b.sigV))};
}
DBSDE_HD void heston2_step(float mu_a, float kappa, float theta, float hsig, float rho, float rhob, float dt, float w1,
                           float w2, float& S, float& v, float& a, float& b) {
  const Heston2Coef c = heston2_coef(mu_a, kappa, theta, hsig, rho, rhob, S, v);
  a = rn_mul(c.d00, w1);
  b = rn_add(rn_mul(c.d10, w1), rn_mul(c.d11, w2));
  S = rn_add(rn_add(S, rn_mul(c.muS, dt)), a);
  v = rn_add(rn_add(v, rn_mul(c.muV, dt)), b);
}

// Arithmetic-average (Asian) problems (DBSDE_PROB_ASIAN, include/dbsde.h):
// state [A, S_1..S_k], each S_i a diagonal process (diag_step), A the running
// average of the row mean.  The row sum runs in one fixed order over
// ASIAN_LANES = 16 partial sums: partial l adds S_l, S_{l + 16}, ... ascending
// onto 0, then the partials meet in an xor butterfly p_l <- p_l + p_{l ^ o},
// o = 1, 2, 4, 8 (fp32 addition commutes, so every partial ends as the same
// sum).  On the device a partial is a lane of a 16-lane group and the
// butterfly its shuffles (paths.hpp); asian_row_sum is the same order on one
// thread.
//   m = (sum_i S_i) / (float)k,   A <- A + (m dt) / T        (the left-point rule)
// with the division correctly rounded (hipcc's default for fp32) and the
// product and the sum rounded on their own.
constexpr int ASIAN_LANES = 16;
DBSDE_HD float asian_lane_sum(const float* S, int k, int lane) {
  float p = 0.f;
  for (int i = lane; i < k; i += ASIAN_LANES) p = rn_add(p, S[i]);
  return p;
}
DBSDE_HD float asian_row_sum(const float* S, int k) {
  float p[ASIAN_LANES];
  for (int l = 0; l < ASIAN_LANES; ++l) p[l] = asian_lane_sum(S, k, l);
  for (int o = 1; o < ASIAN_LANES; o <<= 1) {
    float q[ASIAN_LANES];
    for (int l = 0; l < ASIAN_LANES; ++l) q[l] = rn_add(p[l], p[l ^ o]);
    for (int l = 0; l < ASIAN_LANES; ++l) p[l] = q[l];
  }
  return p[0];
}
DBSDE_HD float asian_mean(float sum, int k) { return sum / (float)k; }
// A_{n+1} from A_n, the row mean m_n of S_n and dt_n
DBSDE_HD void asian_step(float m, float dt, float T, float& A) { A = rn_add(A, rn_mul(m, dt) / T); }

// Geometric-average problems (DBSDE_PROB_GEO_ASIAN): state [G, S_1..S_k], G
// the running geometric average exp((1/T) int mean_i log S_i dt).  The
// arithmetic machinery above runs on lg(S_i) and carries a = log G; the stored
// column is exp(a):
//   lg_i = (float)log((double)max(S_i, FLT_MIN))     (fp64 log, rounded to fp32 once)
//   m    = (sum_i lg_i) / (float)k                   (asian_lane_sum / asian_row_sum's order on lg)
//   a'   = a + (m dt) / T                            (asian_step on a),  a_0 = lg(G_0)
//   G_n  = (float)exp((double)a_n), n >= 1;  row 0 holds G_0 as given
// so G_N = G_0 exp((1/T) sum_n m_n dt_n).
DBSDE_HD float geo_lg(float S) { return (float)log((double)fmaxf(S, 1.17549435e-38f)); }   // FLT_MIN
DBSDE_HD float geo_exp(float a) { return (float)exp((double)a); }
DBSDE_HD float geo_lane_sum(const float* S, int k, int lane) {
  float p = 0.f;
  for (int i = lane; i < k; i += ASIAN_LANES) p = rn_add(p, geo_lg(S[i]));
  return p;
}
DBSDE_HD float geo_row_sum(const float* S, int k) {
  float p[ASIAN_LANES];
  for (int l = 0; l < ASIAN_LANES; ++l) p[l] = geo_lane_sum(S, k, l);
  for (int o = 1; o < ASIAN_LANES; o <<= 1) {
    float q[ASIAN_LANES];
    for (int l = 0; l < ASIAN_LANES; ++l) q[l] = rn_add(p[l], p[l ^ o]);
    for (int l = 0; l < ASIAN_LANES; ++l) p[l] = q[l];
  }
  return p[0];
}

// Knock-out (barrier) problems (DBSDE_PROB_BARRIER): the DIAG process stopped
// at the first monitored row whose payoff statistic is beyond the barrier B.
// The statistic is the payoff's own over its `cols` leading state columns, in
// asian_row_sum's order; every comparison is fp32.  gsign > 0 (the calls):
// down-and-out, hit when stat <= B; gsign < 0 (the puts): up-and-out, hit when
// stat >= B.  A NaN statistic never hits.
DBSDE_HD float barrier_stat(const float* X, int cols, bool mean) {
  const float s = asian_row_sum(X, cols);
  return mean ? asian_mean(s, cols) : s;
}
DBSDE_HD bool barrier_hit(float stat, float B, float gsign) { return gsign > 0.f ? stat <= B : stat >= B; }
// One path's rows: X and S point at the first state column of row 0 of the
// path's xin and sdw rows (row stride ld, rows 0..N, D state columns).  tau is
// the first row n in 0..N that hits; rows n > tau of X get row tau's state
// columns, rows n >= tau of S get 0; nothing else is touched (t keeps
// running).  Returns tau, N + 1 for a path that never hits (it is left as it
// is).  The device pass (rollout_barrier_stop_kernel, paths.hpp) restates this
// rule over a 16-lane group.
DBSDE_HD int barrier_stop(float* X, float* S, int ld, int N, int D, int cols, bool mean, float B, float gsign) {
  int tau = N + 1;
  for (int n = 0; n <= N && tau > N; ++n)
    if (barrier_hit(barrier_stat(X + (size_t)n * ld, cols, mean), B, gsign)) tau = n;
  for (int n = tau + 1; n <= N; ++n)
    for (int d = 0; d < D; ++d) X[(size_t)n * ld + d] = X[(size_t)tau * ld + d];
  for (int n = tau; n <= N; ++n)
    for (int d = 0; d < D; ++d) S[(size_t)n * ld + d] = 0.f;
  return tau;
}

}  // namespace dbsde
