// evals.hip -- the references' exact / comparator solutions on the device:
// the closed forms the drivers compare the learned Y against
// (DeepBSDE.py:345-349, nd_BSPDE_case.py:587-658, with_corr...py:621-700) and
// the HJB Monte-Carlo value (hjb_implement.py:1088-1095), and the Heston
// characteristic-function price of the two-factor model.  Exported through
// include/dbsde.h (dbsde_exact, dbsde_hjb_mc); no context needed.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/dbsde.h"
#include "philox.hpp"

int fail(dbsde_ctx* c, int code, const std::string& msg);   // net.hip: the message dbsde_last_error(NULL) returns

namespace dbsde {

__device__ __forceinline__ double ncdf(double x) { return 0.5 * erfc(-x * 0.70710678118654752440); }

// Black-Scholes call (q = 0) at time-to-maturity tau; the payoff and its
// 1 / 1/2 / 0 delta at tau <= 0 (nd_BSPDE_case.py:590-618)
__device__ __forceinline__ void bs_call(double S, double K, double tau, double r, double sig, double& price,
                                        double& delta) {
  if (tau > 0.0) {
    const double st = sig * sqrt(tau);
    const double d1 = (log(S / K) + (r + 0.5 * sig * sig) * tau) / st;
    const double d2 = d1 - st;
    price = S * ncdf(d1) - K * exp(-r * tau) * ncdf(d2);
    delta = ncdf(d1);
  } else {
    price = S - K > 0.0 ? S - K : 0.0;
    delta = S > K ? 1.0 : (S == K ? 0.5 : 0.0);
  }
}

// Black-Scholes put, computed directly (never as call minus parity, which
// loses a deep out-of-the-money put to cancellation): K e^{-r tau} N(-d2) -
// S N(-d1), delta -N(-d1); the payoff and its -1 / -1/2 / 0 delta at tau <= 0
__device__ __forceinline__ void bs_put(double S, double K, double tau, double r, double sig, double& price,
                                       double& delta) {
  if (tau > 0.0) {
    const double st = sig * sqrt(tau);
    const double d1 = (log(S / K) + (r + 0.5 * sig * sig) * tau) / st;
    const double d2 = d1 - st;
    price = K * exp(-r * tau) * ncdf(-d2) - S * ncdf(-d1);
    delta = -ncdf(-d1);
  } else {
    price = K - S > 0.0 ? K - S : 0.0;
    delta = S < K ? -1.0 : (S == K ? -0.5 : 0.0);
  }
}
template <bool PUT>
__device__ __forceinline__ void bs_price(double S, double K, double tau, double r, double sig, double& price,
                                         double& delta) {
  if constexpr (PUT)
    bs_put(S, K, tau, r, sig, price, delta);
  else
    bs_call(S, K, tau, r, sig, price, delta);
}

struct ExactArgs {
  int kind, D;
  long long R;
  double T, p0, p1, p2, p3, p4, p5;
  const float* t;
  const float* x;
  float* price;
  float* delta;
};

// PUT: a.kind holds the call kind, the option prices are the puts'
template <bool PUT>
__global__ void __launch_bounds__(256) exact_kernel(ExactArgs a) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  const long long n = a.kind == DBSDE_EXACT_BS_CALL ? a.R * a.D : a.R;
  if (i >= n) return;
  const long long r = a.kind == DBSDE_EXACT_BS_CALL ? i / a.D : i;
  const double tau = a.T - (double)a.t[r];
  const float* xr = a.x + r * a.D;
  double price = 0.0, delta = 0.0;
  if (a.kind == DBSDE_EXACT_BSB) {            // exp((r + s^2)(T - t)) |x|^2
    double s2 = 0.0;
    for (int d = 0; d < a.D; ++d) s2 += (double)xr[d] * (double)xr[d];
    price = exp((a.p0 + a.p1 * a.p1) * tau) * s2;
  } else if (a.kind == DBSDE_EXACT_BS_CALL) {
    bs_price<PUT>((double)a.x[i], a.p2, tau, a.p0, a.p1, price, delta);
  } else if (a.kind == DBSDE_EXACT_BASKET_AVG) {   // call on mean(x), sigma / sqrt(D)
    double sm = 0.0;
    for (int d = 0; d < a.D; ++d) sm += (double)xr[d];
    bs_price<PUT>(sm / a.D, a.p2, tau, a.p0, a.p1 / sqrt((double)a.D), price, delta);
  } else {                                     // mean of the per-asset calls
    double ps = 0.0, ds = 0.0;
    for (int d = 0; d < a.D; ++d) {
      double pc, dc;
      bs_price<PUT>((double)xr[d], a.p2, tau, a.p0, a.p1, pc, dc);
      ps += pc;
      ds += dc;
    }
    price = ps / a.D;
    delta = ds / a.D;
  }
  a.price[i] = (float)price;
  if (a.delta) a.delta[i] = (float)delta;
}

// DBSDE_EXACT_GEO_ASIAN / _PUT: the option on the geometric average G_T = G exp((1/T)
// int_t^T mean_i log S_i ds) of k correlated GBM assets (dS_i = mu S_i dt + sigma S_i
// (L dW)_i), x = [G, S_1..S_k].  log G_T is normal with
//   M = ln G + [tau mean_i ln S_i + (mu - sigma^2 cbar / 2) tau^2 / 2] / T,
//   V = sigma^2 vbar tau^3 / (3 T^2),
// cbar = mean_i (L L^T)_ii, vbar = 1^T L L^T 1 / k^2.  One thread per point; the put
// is computed directly.  tau <= 0: the payoff and its 1 / 1/2 / 0 derivative in G.
template <bool PUT>
__global__ void __launch_bounds__(256) geo_asian_exact_kernel(ExactArgs a) {
  const long long r = blockIdx.x * 256LL + threadIdx.x;
  if (r >= a.R) return;
  const double tau = a.T - (double)a.t[r];
  const float* xr = a.x + r * a.D;
  const int k = a.D - 1;
  const double mu = a.p0, rr = a.p1, sig = a.p2, K = a.p3, cbar = a.p4, vbar = a.p5;
  const double G = (double)xr[0];
  double price, fwd;   // fwd: e^{-r tau} e^{M + V/2} N(+-d1) with the option's sign, the factor of every delta
  if (tau > 0.0) {
    double ml = 0.0;
    for (int d = 1; d < a.D; ++d) ml += log((double)xr[d]);
    ml /= (double)k;
    const double M = log(G) + (tau * ml + (mu - 0.5 * sig * sig * cbar) * tau * tau * 0.5) / a.T;
    const double V = sig * sig * vbar * tau * tau * tau / (3.0 * a.T * a.T);
    const double sv = sqrt(V);
    const double d2 = (M - log(K)) / sv, d1 = d2 + sv;
    const double df = exp(-rr * tau), F = exp(M + 0.5 * V);
    if constexpr (PUT) {
      price = df * (K * ncdf(-d2) - F * ncdf(-d1));
      fwd = -df * F * ncdf(-d1);
    } else {
      price = df * (F * ncdf(d1) - K * ncdf(d2));
      fwd = df * F * ncdf(d1);
    }
  } else {
    const double s = PUT ? K - G : G - K;
    price = s > 0.0 ? s : 0.0;
    fwd = (PUT ? -1.0 : 1.0) * (s > 0.0 ? 1.0 : (s == 0.0 ? 0.5 : 0.0)) * G;
  }
  a.price[r] = (float)price;
  if (a.delta) {
    float* dr = a.delta + r * a.D;
    dr[0] = (float)(fwd / G);
    for (int d = 1; d < a.D; ++d) dr[d] = tau > 0.0 ? (float)(fwd * tau / ((double)k * a.T * (double)xr[d])) : 0.f;
  }
}

// DBSDE_EXACT_BARRIER_CALL / _PUT: the down-and-out call (B <= K) and the up-and-out
// put (B >= K) without rebate on one GBM asset with cost of carry b (Reiner and
// Rubinstein 1991; include/dbsde.h has the terms): A - C, f = +1 / -1.  n_mon > 0
// first moves B away from S by exp(-+0.5826 sigma sqrt(tau / n_mon)) (Broadie,
// Glasserman and Kou 1997), the continuity correction for n_mon monitoring dates.
// The S-derivatives of the normal densities cancel inside A and inside C (S e^{(b - r)
// tau} n(x1) = K e^{-r tau} n(x1 - s), and the same with the (B / S) powers at y1), so
//   delta = f e^{(b - r) tau} N(f x1) + f e^{(b - r) tau} (2 lambda + 1) (B / S)^{2 lambda + 2} N(f y1)
//           - 2 lambda f K e^{-r tau} (B / S)^{2 lambda} N(f y1 - f s) / S.
// Thread per (point, coordinate); p = {r, sigma, K, b, B, n_mon}.
template <bool PUT>
__global__ void __launch_bounds__(256) barrier_exact_kernel(ExactArgs a) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= a.R * a.D) return;
  const double tau = a.T - (double)a.t[i / a.D];
  const double S = (double)a.x[i];
  const double r = a.p0, sig = a.p1, K = a.p2, b = a.p3, nm = a.p5;
  const double f = PUT ? -1.0 : 1.0;
  double B = a.p4, price = 0.0, delta = 0.0;
  if (tau > 0.0) {
    if (nm > 0.0) B *= exp(-f * 0.5826 * sig * sqrt(tau / nm));
    if (PUT ? S < B : S > B) {
      const double s = sig * sqrt(tau), lam = (b - 0.5 * sig * sig) / (sig * sig);
      const double x1 = log(S / K) / s + (1.0 + lam) * s;
      const double y1 = log(B * B / (S * K)) / s + (1.0 + lam) * s;
      const double cf = exp((b - r) * tau), df = exp(-r * tau);
      const double pw0 = pow(B / S, 2.0 * lam), pw1 = pw0 * (B / S) * (B / S);
      const double Nx1 = ncdf(f * x1), Nx2 = ncdf(f * (x1 - s)), Ny1 = ncdf(f * y1), Ny2 = ncdf(f * (y1 - s));
      const double A = f * S * cf * Nx1 - f * K * df * Nx2;
      const double C = f * S * cf * pw1 * Ny1 - f * K * df * pw0 * Ny2;
      price = A - C;
      delta = f * cf * Nx1 + f * cf * (2.0 * lam + 1.0) * pw1 * Ny1 - 2.0 * lam * f * K * df * pw0 * Ny2 / S;
    }
  } else if (PUT ? S < B : S > B) {
    bs_price<PUT>(S, K, tau, r, sig, price, delta);   // the payoff and its kink delta
  }
  a.price[i] = (float)price;
  if (a.delta) a.delta[i] = (float)delta;
}

// --------------------------------------------------------------------------
// DBSDE_EXACT_AMERICAN_PUT: the put with early exercise on a Cox-Ross-Rubinstein
// tree in fp64 (include/dbsde.h): the arbiter of the penalised
// problem, which no Feynman-Kac expectation prices.  One workgroup per (point,
// coordinate); the level sits in LDS as doubles, node j of level i at
// s u^{2j - i}.  Thread t owns the nodes j = t + 256 k, k < C = ceil((n + 1) /
// 256) <= 17, so the 64 lanes of a wave touch 64 consecutive doubles (no bank
// conflict), and keeps their prices and their own values in registers (one
// multiplication by u per level).  A level step: every thread reads the upper
// neighbour v[j + 1] of each of its nodes, barrier, writes its nodes' new
// values, barrier.  No atomics, a fixed order: bitwise repeatable.
//   pen = +inf:  v = max(c, g)                                  (American)
//   pen finite:  v = g > c ? (c + pen Delta g) / (1 + pen Delta) : c
// the implicit step of u' = .. + pen (g - u)^+ on the node, i.e. the value of
// the penalised problem (pen = 0: the European tree).  A point whose
// risk-neutral probability p = (e^{b Delta} - d) / (u - d) is not in [0, 1]
// (a coarse tree: |b| sqrt(Delta) > sigma) has no tree value: price and delta
// are NaN.
// --------------------------------------------------------------------------
constexpr int TREE_NMAX = 4096;
constexpr int TREE_THREADS = 256;
constexpr int TREE_CMAX = (TREE_NMAX + 1 + TREE_THREADS - 1) / TREE_THREADS;

struct TreeArgs {
  int D, n;
  double T, r, sig, K, b, pen;
  const float* t;
  const float* x;
  float* price;
  float* delta;
};

__global__ void __launch_bounds__(TREE_THREADS) american_put_tree_kernel(TreeArgs a) {
  __shared__ double v[TREE_NMAX + 1];
  const long long i = blockIdx.x;   // (point, coordinate)
  const int tid = threadIdx.x;
  const double tau = a.T - (double)a.t[i / a.D];
  const double S = (double)a.x[i], K = a.K;
  if (tau <= 0.0) {   // the whole workgroup leaves together
    if (tid == 0) {
      a.price[i] = (float)(K - S > 0.0 ? K - S : 0.0);
      if (a.delta) a.delta[i] = (float)(S < K ? -1.0 : (S == K ? -0.5 : 0.0));
    }
    return;
  }
  const int n = a.n;
  const double dl = tau / (double)n, h = a.sig * sqrt(dl);
  const double up = exp(h), dn = 1.0 / up;
  const double p = (exp(a.b * dl) - dn) / (up - dn), q = 1.0 - p, disc = exp(-a.r * dl);
  if (!(p >= 0.0 && p <= 1.0)) {   // (uniform over the workgroup, before any barrier)
    if (tid == 0) {
      a.price[i] = __builtin_nanf("");
      if (a.delta) a.delta[i] = __builtin_nanf("");
    }
    return;
  }
  const bool amer = isinf(a.pen);
  const double pd = amer ? 0.0 : a.pen * dl;
  const int C = (n + TREE_THREADS) / TREE_THREADS;
  double s[TREE_CMAX], w[TREE_CMAX];   // price and value of node tid + 256 k
#pragma unroll
  for (int k = 0; k < TREE_CMAX; ++k) {
    const int j = tid + TREE_THREADS * k;
    s[k] = w[k] = 0.0;
    if (k < C && j <= n) {
      s[k] = S * exp((double)(2 * j - n) * h);
      w[k] = K - s[k] > 0.0 ? K - s[k] : 0.0;
      v[j] = w[k];
    }
  }
  __syncthreads();
  double v10 = 0.0, v11 = 0.0;
  for (int lv = n - 1; lv >= 0; --lv) {
    double hi[TREE_CMAX];
#pragma unroll
    for (int k = 0; k < TREE_CMAX; ++k) {
      const int j = tid + TREE_THREADS * k;
      hi[k] = (k < C && j <= lv) ? v[j + 1] : 0.0;   // j + 1 <= lv + 1 <= n
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TREE_CMAX; ++k) {
      const int j = tid + TREE_THREADS * k;
      if (k < C && j <= lv) {
        s[k] *= up;
        const double c = disc * (p * hi[k] + q * w[k]);
        const double g = K - s[k] > 0.0 ? K - s[k] : 0.0;
        w[k] = amer ? (c > g ? c : g) : (g > c ? (c + pd * g) / (1.0 + pd) : c);
        v[j] = w[k];
      }
    }
    __syncthreads();
    if (lv == 1 && tid == 0) {
      v10 = v[0];
      v11 = v[1];
    }
  }
  if (tid == 0) {
    a.price[i] = (float)v[0];
    if (a.delta) a.delta[i] = (float)((v11 - v10) / (S * up - S * dn));
  }
}

// --------------------------------------------------------------------------
// DBSDE_EXACT_HESTON: the European call under the two-factor Heston model
//   dS = r S dt + sqrt(v) S dW^S,  dv = kappa (theta - v) dt + sigma sqrt(v) dW^v,
//   d<W^S, W^v> = rho dt        (DBSDE_PROB_HESTON2 with k = 1, mu_a = phi_r = r)
// C = S P1 - K exp(-r tau) P2, delta = P1 (Heston 1993),
//   P_j = 1/2 + 1/pi int_0^inf Re[exp(-i phi ln K) f_j(phi) / (i phi)] dphi,
// f_j = exp(C_j + D_j v + i phi ln S) in the branch-stable form (Albrecher,
// Mayer, Schoutens, Tistaert, "The little Heston trap", 2007): with u_1 = 1/2,
// u_2 = -1/2, b_1 = kappa - rho sigma, b_2 = kappa, beta = b_j - rho sigma i phi,
//   d = sqrt(beta^2 + sigma^2 (phi^2 - 2 u_j i phi))     (principal root, Re d >= 0)
//   g = (beta - d) / (beta + d),  e = exp(-d tau)
//   D = (beta - d) / sigma^2 (1 - e) / (1 - g e)
//   C = r i phi tau + kappa theta / sigma^2 [(beta - d) tau - 2 (log(1 - g e) - log(1 - g))]
// |g| < 1 and |e| <= 1, so both logarithms stay on the principal branch for
// every phi and tau.  With E = C + D v + i phi ln(S / K) the integrand is
// exp(Re E) sin(Im E) / phi.  fp64 throughout, own complex arithmetic.
// Quadrature (include/dbsde.h): [0, U] in 64 equal panels, 8-point
// Gauss-Legendre on each.  One wavefront per point, lane l owns panel l and
// adds its 8 nodes in order; the 64 panel sums are added by a fixed xor
// butterfly, so the result is bitwise repeatable.  U = 8 / sqrt(Vbar) times
// the first power of sqrt(2) (at most 2^8) with exp(Re E_j(U)) <= 1e-10 U for
// j = 1, 2: every lane runs that search on the same numbers.
// --------------------------------------------------------------------------
struct cplx {
  double re, im;
};
__device__ __forceinline__ cplx operator+(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx operator-(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx operator*(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cplx operator*(double s, cplx a) { return {s * a.re, s * a.im}; }
__device__ __forceinline__ cplx operator/(cplx a, cplx b) {
  const double q = 1.0 / (b.re * b.re + b.im * b.im);
  return {(a.re * b.re + a.im * b.im) * q, (a.im * b.re - a.re * b.im) * q};
}
__device__ __forceinline__ cplx c_exp(cplx a) {
  const double m = exp(a.re);
  double sn, cs;
  sincos(a.im, &sn, &cs);
  return {m * cs, m * sn};
}
__device__ __forceinline__ cplx c_log(cplx a) { return {log(hypot(a.re, a.im)), atan2(a.im, a.re)}; }
// principal square root (Re >= 0)
__device__ __forceinline__ cplx c_sqrt(cplx a) {
  const double m = hypot(a.re, a.im);
  if (m == 0.0) return {0.0, 0.0};
  if (a.re >= 0.0) {
    const double t = sqrt(0.5 * (m + a.re));
    return {t, 0.5 * a.im / t};
  }
  const double t = sqrt(0.5 * (m - a.re));
  return {0.5 * fabs(a.im) / t, a.im >= 0.0 ? t : -t};
}

struct HestonCf {
  double r, kappa, theta, sigma, rho, tau, v, x;   // x = ln(S / K)
};
// E_j(phi) = C_j + D_j v + i phi x
__device__ __forceinline__ cplx heston_exponent(const HestonCf& h, int j, double phi) {
  const double u = j == 1 ? 0.5 : -0.5;
  const double b = j == 1 ? h.kappa - h.rho * h.sigma : h.kappa;
  const double s2 = h.sigma * h.sigma;
  const cplx one = {1.0, 0.0};
  const cplx beta = {b, -h.rho * h.sigma * phi};
  const cplx d = c_sqrt(beta * beta + cplx{s2 * phi * phi, -2.0 * u * s2 * phi});
  const cplx bmd = beta - d;
  const cplx g = bmd / (beta + d);
  const cplx e = c_exp(-h.tau * d);
  const cplx ge = one - g * e;
  const cplx Dv = (1.0 / s2) * (bmd * ((one - e) / ge));
  const cplx Cv = (h.kappa * h.theta / s2) * (h.tau * bmd - 2.0 * (c_log(ge) - c_log(one - g)));
  const cplx E = Cv + h.v * Dv;
  return {E.re, E.im + phi * (h.r * h.tau + h.x)};
}

constexpr int HQ_PANELS = 64;   // one per lane
constexpr int HQ_GL = 8;
__constant__ double HQ_X[HQ_GL] = {-0.9602898564975363, -0.7966664774136267, -0.5255324099163290, -0.1834346424956498,
                                   0.1834346424956498,  0.5255324099163290,  0.7966664774136267,  0.9602898564975363};
__constant__ double HQ_W[HQ_GL] = {0.1012285362903763, 0.2223810344533745, 0.3137066458778873, 0.3626837833783620,
                                   0.3626837833783620, 0.3137066458778873, 0.2223810344533745, 0.1012285362903763};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// p0..p5 = r, K, kappa, theta, sigma, rho; x [R, 2] = (S, v).  PUT: the same
// quadrature sums I_j = pi (P_j - 1/2) enter K e^{-r tau} (1/2 - I_2 / pi) -
// S (1/2 - I_1 / pi), delta -(1/2 - I_1 / pi): the put's own probabilities,
// not the call minus parity.  The call instance is the code it was.
template <bool PUT>
__device__ __forceinline__ void heston_price(const ExactArgs& a) {
  const int lane = threadIdx.x & 63;
  const long long r = blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (r >= a.R) return;   // whole waves leave together
  const double S = (double)a.x[2 * r], v = (double)a.x[2 * r + 1], K = a.p1;
  const double tau = a.T - (double)a.t[r];
  double price, delta;
  if (tau > 0.0) {
    HestonCf h;
    h.r = a.p0;
    h.kappa = a.p2;
    h.theta = a.p3;
    h.sigma = a.p4;
    h.rho = a.p5;
    h.tau = tau;
    h.v = v;
    h.x = log(S / K);
    // expected integrated variance: the scale of the integrand's decay
    double vbar = h.theta * tau + (v - h.theta) * (1.0 - exp(-h.kappa * tau)) / h.kappa;
    vbar = vbar > 1e-12 ? vbar : 1e-12;
    double U = 8.0 / sqrt(vbar);
    for (int it = 0; it < 16; ++it) {
      const double m1 = exp(heston_exponent(h, 1, U).re), m2 = exp(heston_exponent(h, 2, U).re);
      if ((m1 > m2 ? m1 : m2) <= 1e-10 * U) break;
      U *= 1.4142135623730951;
    }
    const double hw = U / HQ_PANELS, mid = (lane + 0.5) * hw;
    double s1 = 0.0, s2 = 0.0;
    // not unrolled: sixteen inlined fp64 complex exponents at once take every
    // register of the wave (256 VGPRs + 234 AGPRs, spilled SGPRs)
#pragma unroll 1
    for (int q = 0; q < HQ_GL; ++q) {
      const double phi = mid + 0.5 * hw * HQ_X[q];
      const cplx e1 = heston_exponent(h, 1, phi), e2 = heston_exponent(h, 2, phi);
      s1 += HQ_W[q] * (exp(e1.re) * sin(e1.im) / phi);
      s2 += HQ_W[q] * (exp(e2.re) * sin(e2.im) / phi);
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    if constexpr (PUT) {
      const double Q1 = 0.5 - 0.5 * hw * s1 * 0.31830988618379067154;
      const double Q2 = 0.5 - 0.5 * hw * s2 * 0.31830988618379067154;
      price = K * exp(-h.r * tau) * Q2 - S * Q1;
      delta = -Q1;
    } else {
      const double P1 = 0.5 + 0.5 * hw * s1 * 0.31830988618379067154;
      const double P2 = 0.5 + 0.5 * hw * s2 * 0.31830988618379067154;
      price = S * P1 - K * exp(-h.r * tau) * P2;
      delta = P1;
    }
  } else if constexpr (PUT) {
    price = K - S > 0.0 ? K - S : 0.0;
    delta = S < K ? -1.0 : (S == K ? -0.5 : 0.0);
  } else {
    price = S - K > 0.0 ? S - K : 0.0;
    delta = S > K ? 1.0 : (S == K ? 0.5 : 0.0);
  }
  if (lane != 0) return;
  a.price[r] = (float)price;
  if (a.delta) a.delta[r] = (float)delta;
}
__global__ void __launch_bounds__(256) heston_call_kernel(ExactArgs a) { heston_price<false>(a); }
__global__ void __launch_bounds__(256) heston_put_kernel(ExactArgs a) { heston_price<true>(a); }

// HJB Monte-Carlo: block (p, c) sums exp(-g(x_p + s_p z_k)) = 1 / (1/2 + |y|^2/2)
// over its share of the samples k; normals z_k[4 q + j] = normal4 of counter
// (q, HJB_TAG, k, p) (oracle/philox.py hjb_value)
constexpr uint32_t HJB_TAG = 0x484A42u;
constexpr int HJB_CHUNKS = 64;
constexpr int HJB_DMAX = 4096;

__global__ void __launch_bounds__(256) hjb_mc_kernel(const float* t, const float* x, int D, float T, long long mc,
                                                     unsigned long long seed, double* part) {
  __shared__ float xs[HJB_DMAX];
  __shared__ double red[256];
  const int p = blockIdx.x;
  for (int d = threadIdx.x; d < D; d += 256) xs[d] = x[(size_t)p * D + d];
  __syncthreads();
  const double s = sqrt(2.0 * fabs((double)T - (double)t[p]));
  const long long per = (mc + HJB_CHUNKS - 1) / HJB_CHUNKS;
  const long long k0 = (long long)blockIdx.y * per, k1 = k0 + per < mc ? k0 + per : mc;
  double acc = 0.0;
  for (long long k = k0 + threadIdx.x; k < k1; k += 256) {
    double ss = 0.0;
    for (int q = 0; q < (D + 3) / 4; ++q) {
      float z[4];
      philox_normal4(seed, (unsigned long long)p, (uint32_t)k, HJB_TAG, (uint32_t)q, z);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = 4 * q + j;
        if (d < D) {
          const double y = (double)xs[d] + s * (double)z[j];
          ss += y * y;
        }
      }
    }
    acc += 1.0 / (0.5 + 0.5 * ss);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)p * HJB_CHUNKS + blockIdx.y] = red[0];
}

__global__ void hjb_final_kernel(const double* part, int P, long long mc, float* u) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  double s = 0.0;
  for (int c = 0; c < HJB_CHUNKS; ++c) s += part[(size_t)p * HJB_CHUNKS + c];
  u[p] = (float)(-log(s / (double)mc));
}

}  // namespace dbsde

using namespace dbsde;

extern "C" {

int dbsde_exact(int kind, const float* t, const float* x, long long R, int D, float T, const double* params,
                float* price, float* delta, void* stream) {
  const bool geo = kind == DBSDE_EXACT_GEO_ASIAN || kind == DBSDE_EXACT_GEO_ASIAN_PUT;
  const bool tree = kind == DBSDE_EXACT_AMERICAN_PUT;
  const bool bar = kind == DBSDE_EXACT_BARRIER_CALL || kind == DBSDE_EXACT_BARRIER_PUT;
  if (kind < DBSDE_EXACT_BSB || (kind > DBSDE_EXACT_HESTON_PUT && !geo && !tree && !bar) || !t || !x || !params || !price ||
      R < 1 || D < 1)
    return DBSDE_EINVAL;
  if (geo && D < 2) return DBSDE_EINVAL;   // x = [G, S_1..S_k]
  // the kernels read and write whole floats: an address that is no multiple of
  // sizeof(float) (sizeof(double) for params) cannot be such a buffer, and is
  // refused here rather than handed to a launch
  auto misaligned = [](const void* q, size_t a) { return ((uintptr_t)q & (a - 1)) != 0; };
  if (misaligned(t, sizeof(float)) || misaligned(x, sizeof(float)) || misaligned(price, sizeof(float)) ||
      misaligned(delta, sizeof(float)) || misaligned(params, sizeof(double)))
    return DBSDE_EINVAL;
  if (tree) {   // params = {r, sigma, K, b, n_tree, pen}; price and delta [R, D]
    auto bad = [](const std::string& m) { return fail(nullptr, DBSDE_EINVAL, "dbsde_exact(DBSDE_EXACT_AMERICAN_PUT): " + m); };
    const double nt = params[4], pen = params[5];
    if (!(params[1] > 0.0) || !std::isfinite(params[1])) return bad("sigma must be > 0");
    if (!(params[2] > 0.0) || !std::isfinite(params[2])) return bad("K must be > 0");
    if (!std::isfinite(params[0]) || !std::isfinite(params[3])) return bad("r and b must be finite");
    if (!(nt >= 2.0 && nt <= (double)TREE_NMAX) || nt != std::floor(nt))
      return bad("n_tree must be an integer in [2, 4096]");
    if (!(pen >= 0.0)) return bad("pen must be >= 0 (+inf: the American value), not negative or NaN");
    if (R > 0x7fffffffLL / D) return bad("R * D must be below 2^31 (one workgroup per point and coordinate)");
    TreeArgs g{};
    g.D = D;
    g.n = (int)nt;
    g.T = T;
    g.r = params[0];
    g.sig = params[1];
    g.K = params[2];
    g.b = params[3];
    g.pen = pen;
    g.t = t;
    g.x = x;
    g.price = price;
    g.delta = delta;
    american_put_tree_kernel<<<(unsigned)(R * D), TREE_THREADS, 0, (hipStream_t)stream>>>(g);
    return hipGetLastError() == hipSuccess ? DBSDE_OK : DBSDE_EHIP;
  }
  if (bar) {   // params = {r, sigma, K, b, B, n_mon}; price and delta [R, D]
    const bool put = kind == DBSDE_EXACT_BARRIER_PUT;
    auto bad = [](const std::string& m) { return fail(nullptr, DBSDE_EINVAL, "dbsde_exact(DBSDE_EXACT_BARRIER_*): " + m); };
    if (!std::isfinite(params[0]) || !std::isfinite(params[3])) return bad("r and b must be finite");
    if (!(params[1] > 0.0) || !std::isfinite(params[1])) return bad("sigma must be > 0");
    if (!(params[2] > 0.0) || !std::isfinite(params[2])) return bad("K must be > 0");
    if (!(params[4] > 0.0) || !std::isfinite(params[4])) return bad("B must be > 0");
    if (!put && params[4] > params[2]) return bad("the down-and-out call needs B <= K");
    if (put && params[4] < params[2]) return bad("the up-and-out put needs B >= K");
    if (!(params[5] >= 0.0) || !std::isfinite(params[5])) return bad("n_mon must be >= 0 (0: continuous monitoring)");
    if (R > 0x7fffffffLL * 256 / D) return bad("R * D is too large for one launch");
    ExactArgs g{};
    g.kind = kind;
    g.D = D;
    g.R = R;
    g.T = T;
    g.p0 = params[0];
    g.p1 = params[1];
    g.p2 = params[2];
    g.p3 = params[3];
    g.p4 = params[4];
    g.p5 = params[5];
    g.t = t;
    g.x = x;
    g.price = price;
    g.delta = delta;
    const unsigned nblk = (unsigned)((R * D + 255) / 256);
    if (put)
      barrier_exact_kernel<true><<<nblk, 256, 0, (hipStream_t)stream>>>(g);
    else
      barrier_exact_kernel<false><<<nblk, 256, 0, (hipStream_t)stream>>>(g);
    return hipGetLastError() == hipSuccess ? DBSDE_OK : DBSDE_EHIP;
  }
  if (geo) {   // params = {mu, r, sigma, K, cbar, vbar}; delta [R, D]
    if ((R + 255) / 256 > 0x7fffffffLL) return DBSDE_EINVAL;
    ExactArgs g{};
    g.kind = kind;
    g.D = D;
    g.R = R;
    g.T = T;
    g.p0 = params[0];
    g.p1 = params[1];
    g.p2 = params[2];
    g.p3 = params[3];
    g.p4 = params[4];
    g.p5 = params[5];
    g.t = t;
    g.x = x;
    g.price = price;
    g.delta = delta;
    if (kind == DBSDE_EXACT_GEO_ASIAN_PUT)
      geo_asian_exact_kernel<true><<<(unsigned)((R + 255) / 256), 256, 0, (hipStream_t)stream>>>(g);
    else
      geo_asian_exact_kernel<false><<<(unsigned)((R + 255) / 256), 256, 0, (hipStream_t)stream>>>(g);
    return hipGetLastError() == hipSuccess ? DBSDE_OK : DBSDE_EHIP;
  }
  // a put runs its call counterpart's shapes and parameters
  const bool put = kind >= DBSDE_EXACT_BS_PUT;
  if (put) kind -= DBSDE_EXACT_BS_PUT - DBSDE_EXACT_BS_CALL;
  if (kind == DBSDE_EXACT_HESTON && D != 2) return DBSDE_EINVAL;   // x = (S, v): one asset
  ExactArgs a{};
  a.kind = kind;
  a.D = D;
  a.R = R;
  a.T = T;
  a.p0 = params[0];
  a.p1 = params[1];
  a.p2 = kind == DBSDE_EXACT_BSB ? 0.0 : params[2];
  a.t = t;
  a.x = x;
  a.price = price;
  a.delta = delta;
  if (kind == DBSDE_EXACT_HESTON) {   // params = {r, K, kappa, theta, sigma, rho}; one wavefront per point
    a.p3 = params[3];
    a.p4 = params[4];
    a.p5 = params[5];
    if ((R + 3) / 4 > 0x7fffffffLL) return DBSDE_EINVAL;
    if (put)
      heston_put_kernel<<<(unsigned)((R + 3) / 4), 256, 0, (hipStream_t)stream>>>(a);
    else
      heston_call_kernel<<<(unsigned)((R + 3) / 4), 256, 0, (hipStream_t)stream>>>(a);
    return hipGetLastError() == hipSuccess ? DBSDE_OK : DBSDE_EHIP;
  }
  const long long n = kind == DBSDE_EXACT_BS_CALL ? R * D : R;
  if (put)
    exact_kernel<true><<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(a);
  else
    exact_kernel<false><<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? DBSDE_OK : DBSDE_EHIP;
}

int dbsde_hjb_mc(const float* t, const float* x, int P, int D, float T, long long mc, unsigned long long seed,
                 float* u, void* stream) {
  if (!t || !x || !u || P < 1 || D < 1 || D > HJB_DMAX || mc < 1) return DBSDE_EINVAL;
  double* part = nullptr;
  if (hipMallocAsync((void**)&part, (size_t)P * HJB_CHUNKS * sizeof(double), (hipStream_t)stream) != hipSuccess)
    return DBSDE_ENOMEM;
  hjb_mc_kernel<<<dim3(P, HJB_CHUNKS), 256, 0, (hipStream_t)stream>>>(t, x, D, T, mc, seed, part);
  hjb_final_kernel<<<(P + 63) / 64, 64, 0, (hipStream_t)stream>>>(part, P, mc, u);
  const hipError_t e = hipGetLastError();
  (void)hipFreeAsync(part, (hipStream_t)stream);
  return e == hipSuccess ? DBSDE_OK : DBSDE_EHIP;
}

}  // extern "C"
