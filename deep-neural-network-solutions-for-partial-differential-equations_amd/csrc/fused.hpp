// fused.hpp -- shared pieces of the fused phase kernels (phase.hpp): their
// argument block, register tiles, compile-time activations, and the closed-form
// residual / cotangent of one row (DeepBSDE.py:223-240 restated).
#pragma once
#include <type_traits>

#include "kernels.hpp"

namespace dbsde {

// residual / cotangent inputs, shared by phase C (fused) and the forward-only
// loss kernel
struct CotanParams {
  int R, Rp, N1, D, Dp, gcols;
  const float* xin;         // [Rp, Dp]  [t, X, 1, 0..]
  const float* sdw;         // [Rp, Dp]  sigma dW (cols 1..D)
  const float* zfull;       // [Rp, Dp]  Z (cols 1..D)
  const float* u;           // [Rp]      Y
  const float* rowsum;      // [Rp, 8]   [s_zs, s_xz, s_zz, s_x, s_xx, z_1, u-mask, 0]
  const float* q3S;         // [N] or null
  float phi_r, phi_c, phi_zz, strike, g_alpha;
  float gsign;              // -1: put (g_kind holds the call kind, terminal_kind)
  int g_kind;
  float pen;                // dbsde_problem.pen: phi -= pen max(g(X) - Y, 0) (kernels.hpp penalty_phi)
  // net_u VJP (dbsde_net_u_vjp): caller cotangents instead of the BSDE
  // residual ones -- ubar from ext_ub [Rp], zbar from the sdw rows
  int ext;
  const float* ext_ub;
};

struct FusedArgs {
  int R, N1, D, Dp, W, S;   // rows, N+1, D, padded D, padded level width, level stride
  int has_v, act;
  int tile0;                // first 64-row tile of this launch (path-chunked pipeline)
  int gcols;                // leading state columns entering g (row sums s_x, s_xx)
  int u_clamp;              // u = max(net, 0) (heston_dnnpde.py:568)
  float rho;
  const float* xin;         // [Rp, Dp]
  const float* beta[7];     // FC/Resnet level-j bias
  const float* wout;
  const float* bout;
  // phase A outputs
  float *Abuf, *H, *G, *Delta, *u, *zfull, *rowsum;  // rowsum [Rp, 8]
  const float* sdw;         // [Rp, Dp]
  // phase C: cotangents (computed in its prologue) and outputs
  CotanParams cp;
  float* zbar;              // [Rp, Dp] (written for the weight-gradient kernel)
  float* ubar;              // [Rp]
  float* u16;               // [Rp, 16] col 0 = ubar (split-K weight-gradient path) or null
  double* loss_part;        // [Rp / 64] per-workgroup loss sums
  float *Hdot, *Alpha;
  float* Adot;              // phase2 ADOT kernels: adot_j between the tangent and the reverse (tile order)
  // fragment images of the stage sequence of each pass (phase.hpp)
  // (fp32 images: two pieces per stage; split-bf16 images: one piece per
  // 32-wide input block, phase.hpp)
  const float* simgA[64];
  int snfA[64];
  int nA;
  const float* simgC[64];
  int snfC[64];
  int nC;
};

template <int TT>
struct Mat {
  floatx4 v[TT];
};

// SiLU / Softplus are straight-line code, and left alone the compiler moves it
// to where it costs registers.  Phase A: it sinks the derivative's half
// (reciprocal, select, multiplies) from the forward to its use in the
// backward, so that s1 holds e and 1 + e per element instead of act'(a), twice
// the registers (the width-112 phase A spilled 136..255 of them).  Phase C's
// tangent: SiLU's act'(a) = s + a q spilled 16 registers at width 112 however
// the prefetch was set.  The empty statement makes its operand a value that
// exists at that point: act'(a) where phase A stores it, a where SiLU's act_1
// starts.  For the other activations it is nothing, and they compile to the
// code they compiled to without it.
template <int ACT>
__device__ __forceinline__ void act_pin(float& v) {
  if constexpr (ACT == ACT_SILU || ACT == ACT_SOFTPLUS) asm volatile("" : "+v"(v));
}

// activation with compile-time kind: value + first derivative, and first +
// second derivative (one sincos / tanh / exponential per element; SiLU and
// Softplus: act.hpp)
template <int ACT>
__device__ __forceinline__ void act_v1(float a, float& f, float& d1) {
  if constexpr (ACT == ACT_SINE) {
    fast_sincosf(a, f, d1);
  } else if constexpr (ACT == ACT_TANH) {
    f = tanhf(a);
    d1 = 1.f - f * f;
  } else if constexpr (ACT == ACT_SILU) {
    silu_v1(a, f, d1);
  } else if constexpr (ACT == ACT_SOFTPLUS) {
    softplus_v1(a, f, d1);
  } else {
    static_assert(ACT == ACT_RELU, "unknown activation");
    f = a > 0.f ? a : 0.f;
    d1 = a > 0.f ? 1.f : 0.f;
  }
}
template <int ACT>
__device__ __forceinline__ float act_1(float a) {
  if constexpr (ACT == ACT_SINE) {
    float sv, cv;
    fast_sincosf(a, sv, cv);
    return cv;
  } else if constexpr (ACT == ACT_TANH) {
    const float f = tanhf(a);
    return 1.f - f * f;
  } else if constexpr (ACT == ACT_SILU) {
    act_pin<ACT>(a);
    return silu_1(a);
  } else if constexpr (ACT == ACT_SOFTPLUS) {
    return softplus_1(a);
  } else {
    static_assert(ACT == ACT_RELU, "unknown activation");
    return a > 0.f ? 1.f : 0.f;
  }
}
template <int ACT>
__device__ __forceinline__ void act_12(float a, float& d1, float& d2) {
  if constexpr (ACT == ACT_SINE) {
    float sv;
    fast_sincosf(a, sv, d1);
    d2 = -sv;
  } else if constexpr (ACT == ACT_TANH) {
    const float f = tanhf(a);
    d1 = 1.f - f * f;
    d2 = -2.f * f * d1;
  } else if constexpr (ACT == ACT_SILU) {
    silu_12(a, d1, d2);
  } else if constexpr (ACT == ACT_SOFTPLUS) {
    softplus_12(a, d1, d2);   // no logarithm: phase C needs the derivatives only
  } else {
    static_assert(ACT == ACT_RELU, "unknown activation");
    d1 = a > 0.f ? 1.f : 0.f;
    d2 = 0.f;
  }
}

// compile-time loop: f(std::integral_constant<int, I>) for I = B .. E-1, so
// that per-level register arrays are indexed by constants (no scratch)
template <int B, int E>
struct SFor {
  template <class F>
  __device__ __forceinline__ static void run(F&& f) {
    if constexpr (B < E) {
      f(std::integral_constant<int, B>{});
      SFor<B + 1, E>::run(f);
    }
  }
};

template <int TT>
__device__ __forceinline__ void zero(Mat<TT>& m) {
#pragma unroll
  for (int t = 0; t < TT; ++t) m.v[t] = floatx4{0.f, 0.f, 0.f, 0.f};
}

// residual of a non-terminal row from its row sums rs, Y = y, Y_next = yn,
// dt and the Q3 sum: Y_{n+1} - Ytilde_{n+1} (DeepBSDE.py:223-228); dphidy
// receives the row's d phi / d Y (phi_r, plus the penalty's indicator: g from
// the row's own s_x, s_xx)
__device__ __forceinline__ float step_residual(const CotanParams& p, floatx4 rs0, floatx4 rs1, float y, float yn,
                                               float dt, float q3, float& dphidy) {
  const float zs = p.q3S ? rs1[1] * q3 : rs0[0];
  float phi = p.phi_r * (y - p.phi_c * rs0[1]) + p.phi_zz * rs0[2];
  dphidy = p.phi_r;
  if (p.pen != 0.f) {
    float gs, dy;
    phi += penalty_phi(p.pen, terminal_g(p.g_kind, rs0[3], rs1[0], p.gcols, p.strike, p.g_alpha, p.gsign, gs), y, dy);
    dphidy = p.phi_r + dy;
  }
  return yn - (y + phi * dt + zs);
}

// cotangents of row r: ubar (d loss / d Y_r) and the per-row scalars the zbar
// entries need.  The loss of the row is res^2 + |Z - grad g|^2 (terminal).
// Every load is issued up front from clamped indices (one memory latency, not
// a chain of dependent ones).
struct RowCotan {
  bool valid, term;
  int n;
  float res, ub, coefY, dt, gsc, mask, q3s;
  float gA, gB;   // terminal: d g / d x_col = gA x_col + gB (terminal_dg as an affine map)
};
__device__ __forceinline__ RowCotan row_cotan(const CotanParams& p, int r) {
  RowCotan c{};
  c.valid = r < p.R;
  const int rr = c.valid ? r : 0;
  const int n = rr % p.N1;
  const bool term = n == p.N1 - 1;
  const int rn = term ? rr : rr + 1, rp = n >= 1 ? rr - 1 : rr;
  const floatx4 a0 = *(const floatx4*)(p.rowsum + (size_t)rr * 8), a1 = *(const floatx4*)(p.rowsum + (size_t)rr * 8 + 4);
  const floatx4 b0 = *(const floatx4*)(p.rowsum + (size_t)rp * 8), b1 = *(const floatx4*)(p.rowsum + (size_t)rp * 8 + 4);
  const float y = p.u[rr], yn = p.u[rn], yp = p.u[rp];
  const float t = p.xin[(size_t)rr * p.Dp], tn = p.xin[(size_t)rn * p.Dp], tp = p.xin[(size_t)rp * p.Dp];
  const float q = p.q3S ? p.q3S[term ? 0 : n] : 0.f, qp = p.q3S ? p.q3S[n >= 1 ? n - 1 : 0] : 0.f;
  c.n = n;
  c.term = term;
  c.mask = a1[2];
  if (term) {
    c.res = y - terminal_g(p.g_kind, a0[3], a1[0], p.gcols, p.strike, p.g_alpha, p.gsign, c.gsc);
    c.ub = 2.f * c.res;
    c.gA = p.g_kind == 0 ? 2.f : (p.g_kind == 3 ? c.gsc : 0.f);
    c.gB = (p.g_kind == 0 || p.g_kind == 3) ? 0.f : c.gsc;
  } else {
    c.dt = tn - t;
    float dy;
    c.res = step_residual(p, a0, a1, y, yn, c.dt, q, dy);
    c.ub = -2.f * c.res * (1.f + dy * c.dt);
    c.q3s = q;
  }
  float dyp;   // (the previous row's own factor is that row's business)
  if (n >= 1) c.ub += 2.f * step_residual(p, b0, b1, yp, y, t - tp, qp, dyp);
  c.ub *= c.mask;
  c.coefY = -2.f * c.res;
  if (!c.valid) c.res = c.ub = c.coefY = 0.f;   // padding rows carry no cotangent
  return c;
}
// zbar of column col (1 <= col <= D) from x, z, (sigma dW) of that column;
// tz accumulates the terminal |Z - grad g|^2 over the g columns
// Branch-free (both row kinds evaluated, then selected): straight-line code
// per element, no divergence between terminal and interior rows of a wave.
__device__ __forceinline__ float col_zbar(const CotanParams& p, const RowCotan& c, int col, float xv, float zv,
                                          float sv, float& tz) {
  const float dphidz = -p.phi_r * p.phi_c * xv + 2.f * p.phi_zz * zv;
  const float sd = p.q3S ? c.q3s : sv;
  const float vn = c.mask * (c.coefY * (dphidz * c.dt + sd));
  const float e = zv - (c.gA * xv + c.gB);
  const bool ing = col <= p.gcols;
  tz += (c.term && ing) ? e * e : 0.f;
  const float vt = ing ? c.mask * (2.f * e) : 0.f;
  return c.term ? vt : vn;
}

// Forward-only loss (predict / loss_function without backward): per-block
// partial sums of the row losses; 16 threads per row, 16 rows per block.
#ifndef DBSDE_DEVICE_HELPERS_ONLY
__global__ void __launch_bounds__(256) cotan_kernel(CotanParams p, double* loss_part) {
  const int sub = threadIdx.x & 15;
  const int r = blockIdx.x * 16 + (threadIdx.x >> 4);
  double lv = 0.0;
  const RowCotan c = row_cotan(p, r);
  if (c.valid) {
    float tz = 0.f;
    if (c.term) {
      const float* xr = p.xin + (size_t)r * p.Dp;
      const float* zr = p.zfull + (size_t)r * p.Dp;
      const float* sr = p.sdw + (size_t)r * p.Dp;
      for (int col = 1 + sub; col <= p.D; col += 16) (void)col_zbar(p, c, col, xr[col], zr[col], sr[col], tz);
    }
    tz = red16(tz);
    if (sub == 0) lv = (double)(c.res * c.res + tz);
  }
  __shared__ double red[256];
  red[threadIdx.x] = lv;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_part[blockIdx.x] = red[0];
}

// Wide contexts (Dp > 128): the Z GEMM runs over column tiles, so no epilogue
// holds a whole Z row.  This kernel does for such a row what the EPI_COTAN
// epilogue does inside the GEMM: the u-clamp mask on Z, the residual row sums,
// the residual (interior rows) or terminal mismatch, zbar, rres and lossrow;
// ubar_kernel follows as in the narrow chain.  One 16-lane group per row:
// lane l visits columns l, l + 16, ... in ascending order and the 16 partial
// sums meet in red16's xor butterfly, so the order of every sum is fixed.
// grid Rp / 16; rows in [R, Rp) write zeros.
struct ZRowArgs {
  CotanParams p;        // rowsum / ext unused
  const float* umask;   // [Rp] u-clamp gradient mask or null
  float* zfull;         // [Rp, Dp] Z as the GEMM stored it; masked in place
  float* zbar;          // [Rp, Dp]
  float* rres;          // [Rp]
  float* lossrow;       // [Rp]
  float* dphidy;        // [Rp] pen != 0: the row's d phi / d Y, for ubar_kernel
};
__global__ void __launch_bounds__(256) zrow_cotan_kernel(ZRowArgs a) {
  const CotanParams& p = a.p;
  const int sub = threadIdx.x & 15;
  const int r = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (r >= p.Rp) return;
  RowCotan c{};
  c.valid = r < p.R;
  c.n = c.valid ? r % p.N1 : 0;
  c.term = c.n == p.N1 - 1;
  c.mask = a.umask ? a.umask[r] : 1.f;
  const size_t ro = (size_t)r * p.Dp;
  const float* xr = p.xin + ro;
  const float* sr = p.sdw + ro;
  float* zr = a.zfull + ro;
  float s_zs = 0.f, s_xz = 0.f, s_zz = 0.f, s_x = 0.f, s_xx = 0.f, z1 = 0.f;
  for (int col = sub; col < p.Dp; col += 16) {
    const float z = zr[col] * c.mask;
    if (a.umask) zr[col] = z;
    if (col >= 1 && col <= p.D) {
      const float xv = xr[col];
      s_zs += z * sr[col];
      s_xz += xv * z;
      s_zz += z * z;
      if (col <= p.gcols) {
        s_x += xv;
        s_xx += xv * xv;
      }
      if (col == 1) z1 = z;
    }
  }
  const floatx4 rs0 = {red16(s_zs), red16(s_xz), red16(s_zz), red16(s_x)};
  const floatx4 rs1 = {red16(s_xx), red16(z1), c.mask, 0.f};
  if (c.valid) {
    const float y = p.u[r];
    if (!c.term) {
      c.dt = xr[p.Dp] - xr[0];
      c.q3s = p.q3S ? p.q3S[c.n] : 0.f;
      float dy;
      c.res = step_residual(p, rs0, rs1, y, p.u[r + 1], c.dt, c.q3s, dy);
      if (p.pen != 0.f && sub == 0) a.dphidy[r] = dy;
      c.coefY = -2.f * c.res;
    } else {
      c.res = y - terminal_g(p.g_kind, rs0[3], rs1[0], p.gcols, p.strike, p.g_alpha, p.gsign, c.gsc);
      c.gA = p.g_kind == 0 ? 2.f : (p.g_kind == 3 ? c.gsc : 0.f);
      c.gB = (p.g_kind == 0 || p.g_kind == 3) ? 0.f : c.gsc;
    }
  }
  float tz = 0.f;
  float* zb = a.zbar + ro;
  for (int col = sub; col < p.Dp; col += 16) {
    float v = 0.f;
    if (c.valid && col >= 1 && col <= p.D) v = col_zbar(p, c, col, xr[col], zr[col], sr[col], tz);
    zb[col] = v;
  }
  tz = red16(tz);
  if (sub == 0) {
    a.rres[r] = c.valid ? c.res : 0.f;
    a.lossrow[r] = c.valid ? c.res * c.res + tz : 0.f;
  }
}
#endif

}  // namespace dbsde
