// kernels.hpp -- HIP kernels (gfx950 / CDNA4) of the deep-BSDE training step.
//
// Row layout: one "row" = one (path m, time n) pair, r = m*(N+1)+n, exactly the
// reference's X[M, N+1, D] order (DeepBSDE.py:242).  All activation buffers are
// row-major [Rp, ld] fp32 with Rp a multiple of 64 and ld a multiple of 16.
// Padding rows/columns of the pre-activations are zero and stay zero.  With
// act(0) = 0 (Sine, ReLU, Tanh, SiLU) so are the hidden states; Softplus leaves
// log 2 there, which nothing reads into a result: a padding column meets zero
// weight columns in the next layer and in w_out, and only the padded part of
// a weight-gradient tile, which no finalize window covers; a padding row
// carries no cotangent (row_cotan), so it adds nothing to any gradient.
//
// Unified network (see oracle/timeparallel.py for the derivation):
//   a_0 = x W_in^T + b_in,  h_1 = act(a_0)
//   a_j = h_j B_j^T + [x V_j^T] + beta_j,  h_{j+1} = act(a_j) + rho h_j   (j=1..K)
//   u   = h_{K+1}.w_out + b_out
// "level j" of an [Rp, Stot] buffer holds the width-L_{j+1} quantity of a_j.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "act.hpp"

namespace dbsde {

typedef float floatx4 __attribute__((ext_vector_type(4)));

enum Act { ACT_SINE = 0, ACT_RELU = 1, ACT_TANH = 2, ACT_SILU = 3, ACT_SOFTPLUS = 4 };

// sin and cos together on the transcendental unit: a is reduced modulo 2*pi in
// radians (two-part Cody-Waite 2*pi in fp32, |r| <= pi), scaled to revolutions
// and fed to v_sin_f32 / v_cos_f32 (sin(2*pi*x), quarter rate).  7 VALU-slot
// equivalents per element instead of ~25 for a minimax polynomial; the phase
// kernels evaluate it 4 (phase A) and 8 (phase C) times per activation element.
// Max abs error ~3e-7 (2.5 ulp of 1), independent of |a| because the
// reduction happens before the scaling (tools/ubench/sincos_acc.hip measures
// it against fp64 libm on the GPU; the plain fract-of-a/(2pi) form grows to
// 5.5e-6 at |a| = 64).
__device__ __forceinline__ void fast_sincosf(float a, float& s, float& c) {
  const float k = rintf(a * 0.15915494309189535f);
  float r = fmaf(-k, 6.2831854820251465f, a);   // 2pi_hi = fp32(2pi)
  r = fmaf(-k, -1.7484555314695172e-07f, r);    // 2pi_lo = 2pi - 2pi_hi
  const float rev = r * 0.15915494309189535f;   // [-1/2, 1/2]
  s = __builtin_amdgcn_sinf(rev);
  c = __builtin_amdgcn_cosf(rev);
}
__device__ __forceinline__ float act_f(int act, float a) {
  if (act == ACT_SINE) {
    float sv, cv;
    fast_sincosf(a, sv, cv);
    return sv;
  }
  if (act == ACT_TANH) return tanhf(a);
  if (act == ACT_SILU) return silu_f(a);
  if (act == ACT_SOFTPLUS) return softplus_f(a);
  return a > 0.f ? a : 0.f;
}
__device__ __forceinline__ float act_d1(int act, float a) {
  if (act == ACT_SINE) {
    float sv, cv;
    fast_sincosf(a, sv, cv);
    return cv;
  }
  if (act == ACT_TANH) {
    float t = tanhf(a);
    return 1.f - t * t;
  }
  if (act == ACT_SILU) return silu_1(a);
  if (act == ACT_SOFTPLUS) return softplus_1(a);
  return a > 0.f ? 1.f : 0.f;
}
__device__ __forceinline__ void act_d12(int act, float a, float& d1, float& d2) {
  if (act == ACT_SINE) {
    float s, c;
    fast_sincosf(a, s, c);
    d1 = c;
    d2 = -s;
  } else if (act == ACT_TANH) {
    float t = tanhf(a);
    d1 = 1.f - t * t;
    d2 = -2.f * t * d1;
  } else if (act == ACT_SILU) {
    silu_12(a, d1, d2);
  } else if (act == ACT_SOFTPLUS) {
    softplus_12(a, d1, d2);
  } else {
    d1 = a > 0.f ? 1.f : 0.f;
    d2 = 0.f;
  }
}

__device__ __forceinline__ floatx4 mfma4(float a, float b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// --------------------------------------------------------------------------
// terminal condition g(X_N) over the leading G state columns and the scale of
// its gradient (DeepBSDE.py:196-200 via autograd):
//   0 sumsq   g = |x|^2                     dg = 2 x          (DeepBSDE.py:333-335)
//   1 call    g = max(sum x - K, 0)         dg = gsc          (nd_BSPDE_case.py:521-522)
//   2 basket  g = max(mean x - K, 0)        dg = gsc          (with_corr...py:577-579,
//                                                              heston_dnnpde.py:550)
//   3 log     g = log(1/2 + |x|^2/2)        dg = x gsc        (hjb_implement.py:597-598)
//   4 smooth  g = a / (1 + e^{-alpha a}), a = mean x - K      (heston_dnnpde.py:551-556)
// torch.maximum splits the gradient 1/2 : 1/2 at a tie, so gsc = 1/2 there.
// The puts (DBSDE_G_PUT_SUM / PUT_MEAN / SMOOTH_PUT) arrive here as kinds
// 1 / 2 / 4 with gsign = -1 (terminal_kind below): the moneyness and the
// gradient scale change sign and nothing else does.  gsign = 1 multiplies
// exactly, so the calls keep their bits.
// --------------------------------------------------------------------------
__host__ __device__ inline int terminal_kind(int g_kind, float& gsign) {
  gsign = g_kind >= 5 ? -1.f : 1.f;
  return g_kind == 5 ? 1 : (g_kind == 6 ? 2 : (g_kind == 7 ? 4 : g_kind));
}
__device__ __forceinline__ float terminal_g(int kind, float s_x, float s_xx, int G, float strike, float alpha,
                                            float gsign, float& gsc) {
  gsc = 0.f;
  if (kind == 0) return s_xx;
  if (kind == 1 || kind == 2) {
    const float v = gsign * (kind == 1 ? s_x - strike : s_x / (float)G - strike);
    const float sc = gsign * (kind == 1 ? 1.f : 1.f / (float)G);
    gsc = v > 0.f ? sc : (v == 0.f ? 0.5f * sc : 0.f);
    return v > 0.f ? v : 0.f;
  }
  if (kind == 3) {
    const float q = 0.5f + 0.5f * s_xx;
    gsc = 1.f / q;
    return logf(q);
  }
  const float a = gsign * (s_x / (float)G - strike);
  const float e = expf(-alpha * a);
  const float den = 1.f + e;
  gsc = gsign * ((1.f / den + a * alpha * e / (den * den)) / (float)G);
  return a / den;
}
__device__ __forceinline__ float terminal_dg(int kind, float x, float gsc) {
  return kind == 0 ? 2.f * x : (kind == 3 ? x * gsc : gsc);
}

// --------------------------------------------------------------------------
// The Y-nonlinear part of the driver (dbsde_problem.pen): the
// penalised American problem adds -pen max(g(X) - Y, 0) to phi, g the terminal
// condition on the row's own X, and pen 1[g > Y] to d phi / d Y (strict: 0 at a
// tie, as torch.relu's gradient).  Returns the term; dphidy receives what
// d phi / d Y gains.  Every caller sits inside `if (pen != 0.f)` on the kernel
// argument, so a problem without a penalty runs none of this.
// --------------------------------------------------------------------------
__device__ __forceinline__ float penalty_phi(float pen, float g, float y, float& dphidy) {
  const bool ex = g > y;
  dphidy = ex ? pen : 0.f;
  return ex ? -(pen * (g - y)) : 0.f;
}

// --------------------------------------------------------------------------
// Chain GEMM:  C[Rp, NP] = A[Rp, K] * Bt[NP, K]^T  with a fused epilogue.
// fp32 MFMA v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulate).
// Workgroup: 4 waves, 64 rows x (16*NT) columns; each wave 16 rows x 16*NT.
// K is staged through LDS in chunks of 16 (double buffered, register staged).
// Inside a 16-chunk, lane group q=lane>>4 feeds k = 4q+i to MFMA i (the sum
// over k is order-free), so each lane reads one float4 of A and of Bt.
// --------------------------------------------------------------------------
enum Epi {
  EPI_FWD0 = 0,   // a = acc -> out0 ; level-0 cols: h1 = act(a) -> out1
  EPI_FWD,        // a = acc + (in0 ? in0 : vec0) ; h = act(a) + rho*in1 ; out0=a, out1=h ; last: out2 = vec1*act'(a)
  EPI_BWD,        // g = acc + rho*(in0 ? in0 : vec0) ; out0=g ; out1 = g*act'(in1)
  EPI_COTAN,      // Z GEMM: residuals, zbar, loss rows
  EPI_TAN0,       // adot = acc -> out0 ; level-0 cols: hdot1 = act'(in0)*adot -> out1
  EPI_TAN,        // adot = acc + (in0?in0:0); hdot = act'(in2)*adot + rho*in1 ; last: out2 = alpha_K
  EPI_REV,        // p = acc + rho*(in0 ? in0 : ubar*vec0) ; out0=p ; out1 = p*act'(in1) + in2*in3*act''(in1)
  EPI_STORE,      // out0 = acc (net_u Z / plain)
  EPI_STORE_N,    // out0 = acc for the columns below lvl0_cols (wide Z GEMM: the last column tile may be ragged)
};

struct ChainArgs {
  const float* A;
  int lda;
  const float* Bt;
  int ldb;
  int K;
  const float* in[4];
  int ldi[4];
  float* out[3];
  int ldo[3];
  const float* vec[2];
  const float* ubar;
  float rho;
  int act;
  int lvl0_cols;  // EPI_FWD0 / EPI_TAN0: number of padded level-0 columns; EPI_STORE_N: output columns
  int last;       // EPI_FWD / EPI_TAN: j == K
  // --- EPI_COTAN
  int R, N1, D;
  const float* xin;   // [Rp, ldx]
  const float* sdw;   // [Rp, ldx]
  int ldx;
  const float* u;     // [Rp]
  const float* q3S;   // [N] or null
  const float* umask; // [Rp] u-clamp gradient mask (heston_dnnpde.py:568) or null
  float phi_r, phi_c, phi_zz, strike, g_alpha;
  float gsign;        // -1: put (g_kind holds the call kind, terminal_kind)
  int g_kind, gcols;
  float pen;          // dbsde_problem.pen (penalty_phi)
  float* dphidy;      // [Rp] pen != 0: the row's d phi / d Y = phi_r + pen 1[g > Y], for ubar_kernel
  float* zbar;        // [Rp, ldx]
  float* rres;        // [Rp]
  float* lossrow;     // [Rp]
  // split-bf16 form (chainx3.hpp): the weight as a fragment image (x3_off)
  // with x3_tout output blocks per input block row, x3_ti 16-wide input blocks
  const unsigned short* x3_img;
  int x3_tout, x3_ti;
};

constexpr int CH_BM = 64;
constexpr int CH_KC = 16;
constexpr int CH_LS = 20;  // LDS row stride in floats (16 + 4 pad)

template <int NT>
__device__ __forceinline__ void chain_mainloop(const ChainArgs& p, int row0, int col0, floatx4 (&acc)[NT]) {
  __shared__ float As[2][CH_BM * CH_LS];
  __shared__ float Bs[2][16 * NT * CH_LS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NBV = (64 * NT + 255) / 256;  // float4 B loads per thread
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};

  const float* Ag = p.A + (size_t)(row0 + (tid >> 2)) * p.lda + (tid & 3) * 4;
  floatx4 areg;
  floatx4 breg[NBV];
  const int nk = p.K / CH_KC;

  auto gload = [&](int kc) {
    areg = *(const floatx4*)(Ag + kc * CH_KC);
#pragma unroll
    for (int i = 0; i < NBV; ++i) {
      int idx = tid + i * 256;
      if (idx < 64 * NT) {
        int br = idx >> 2, bc = (idx & 3) * 4;
        breg[i] = *(const floatx4*)(p.Bt + (size_t)(col0 + br) * p.ldb + kc * CH_KC + bc);
      }
    }
  };
  auto sstore = [&](int buf) {
    *(floatx4*)&As[buf][(tid >> 2) * CH_LS + (tid & 3) * 4] = areg;
#pragma unroll
    for (int i = 0; i < NBV; ++i) {
      int idx = tid + i * 256;
      if (idx < 64 * NT) *(floatx4*)&Bs[buf][(idx >> 2) * CH_LS + (idx & 3) * 4] = breg[i];
    }
  };

  gload(0);
  sstore(0);
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nk) gload(kc + 1);
    const floatx4 a = *(const floatx4*)&As[buf][(wave * 16 + (lane & 15)) * CH_LS + (lane >> 4) * 4];
    floatx4 b[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) b[t] = *(const floatx4*)&Bs[buf][(t * 16 + (lane & 15)) * CH_LS + (lane >> 4) * 4];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mfma4(a.x, b[t].x, acc[t]);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mfma4(a.y, b[t].y, acc[t]);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mfma4(a.z, b[t].z, acc[t]);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mfma4(a.w, b[t].w, acc[t]);
    if (kc + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }
}

__device__ __forceinline__ float red16(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// split-bf16 mainloop (chainx3.hpp)
template <int NT>
__device__ __forceinline__ void chain_x3_mainloop(const ChainArgs& p, int row0, int col0, floatx4 (&acc)[NT]);

template <int NT, int EPI, bool X3 = false>
__global__ void __launch_bounds__(256) chain_gemm_kernel(ChainArgs p) {
  const int row0 = blockIdx.x * CH_BM;
  const int col0 = blockIdx.y * 16 * NT;
  floatx4 acc[NT];
  if constexpr (X3)
    chain_x3_mainloop<NT>(p, row0, col0, acc);
  else
    chain_mainloop<NT>(p, row0, col0, acc);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rbase = row0 + wave * 16 + (lane >> 4) * 4;
  const int cl = lane & 15;

  if constexpr (EPI == EPI_COTAN) {
    // Each 16-lane group owns 4 rows; the workgroup tile covers every column
    // (the engine launches this epilogue with a single column tile).
    const int D = p.D, G = p.gcols;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = rbase + j;
      const bool valid = row < p.R;
      const int n = valid ? row % p.N1 : 0;
      const bool term = n == p.N1 - 1;
      const float* xr = p.xin + (size_t)row * p.ldx;
      const float* sr = p.sdw + (size_t)row * p.ldx;
      // Heston u clamp: Z = mask * grad u_raw, and the cotangents of the
      // clamped u are masked the same way
      const float um = p.umask ? p.umask[row] : 1.f;
      float s_zs = 0.f, s_xz = 0.f, s_zz = 0.f, s_x = 0.f, s_xx = 0.f, z1 = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = col0 + t * 16 + cl;  // Zfull column (0 = t, 1..D = Z)
        const float z = acc[t][j] * um;
        acc[t][j] = z;
        if (c >= 1 && c <= D) {
          const float xv = xr[c];
          s_zs += z * sr[c];
          s_xz += xv * z;
          s_zz += z * z;
        }
        if (c >= 1 && c <= G) {
          const float xv = xr[c];
          s_x += xv;
          s_xx += xv * xv;
        }
        if (c == 1) z1 = z;
      }
      s_zs = red16(s_zs);
      s_xz = red16(s_xz);
      s_zz = red16(s_zz);
      s_x = red16(s_x);
      s_xx = red16(s_xx);
      z1 = red16(z1);
      float res = 0.f, lossv = 0.f, coefY = 0.f, S = 0.f, dt = 0.f, gsc = 0.f;
      if (valid) {
        const float y = p.u[row];
        if (!term) {
          dt = xr[p.ldx] - xr[0];
          // Q3 (D == 1, 1d_BSPDE_case.py:271-273): Z_i * sum_j (sigma dW)_j
          if (p.q3S) S = p.q3S[n];
          const float zs = p.q3S ? z1 * S : s_zs;
          float phi = p.phi_r * (y - p.phi_c * s_xz) + p.phi_zz * s_zz;
          if (p.pen != 0.f) {   // the row's own g, from the sums it already holds
            float gs, dy;
            phi += penalty_phi(p.pen, terminal_g(p.g_kind, s_x, s_xx, G, p.strike, p.g_alpha, p.gsign, gs), y, dy);
            if (cl == 0) p.dphidy[row] = p.phi_r + dy;
          }
          const float ytil = y + phi * dt + zs;
          res = p.u[row + 1] - ytil;
          lossv = res * res;
          coefY = -2.f * res;
        } else {
          const float g = terminal_g(p.g_kind, s_x, s_xx, G, p.strike, p.g_alpha, p.gsign, gsc);
          res = y - g;
          lossv = res * res;
        }
      }
      // zbar row and the terminal |Z - grad g|^2
      float tz = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = col0 + t * 16 + cl;
        const float z = acc[t][j];
        float zb = 0.f;
        if (valid && c >= 1 && c <= D) {
          const float xv = xr[c];
          if (!term) {
            const float dphidz = -p.phi_r * p.phi_c * xv + 2.f * p.phi_zz * z;
            const float sd = p.q3S ? S : sr[c];
            zb = um * (coefY * (dphidz * dt + sd));
          } else if (c <= G) {
            const float e = z - terminal_dg(p.g_kind, xv, gsc);
            tz += e * e;
            zb = um * (2.f * e);
          }
        }
        p.zbar[(size_t)row * p.ldx + c] = zb;
        p.out[0][(size_t)row * p.ldo[0] + c] = z;
      }
      tz = red16(tz);
      if (cl == 0) {
        p.rres[row] = valid ? res : 0.f;
        p.lossrow[row] = valid ? lossv + tz : 0.f;
      }
    }
    return;
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = col0 + t * 16 + cl;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const size_t row = (size_t)(rbase + j);
        const float v = acc[t][j];
        if constexpr (EPI == EPI_STORE) {
          p.out[0][row * p.ldo[0] + c] = v;
        } else if constexpr (EPI == EPI_STORE_N) {
          if (c < p.lvl0_cols) p.out[0][row * p.ldo[0] + c] = v;
        } else if constexpr (EPI == EPI_FWD0) {
          p.out[0][row * p.ldo[0] + c] = v;
          if (c < p.lvl0_cols) p.out[1][row * p.ldo[1] + c] = act_f(p.act, v);
        } else if constexpr (EPI == EPI_FWD) {
          const float a = v + (p.in[0] ? p.in[0][row * p.ldi[0] + c] : p.vec[0][c]);
          const float h = act_f(p.act, a) + (p.rho != 0.f ? p.rho * p.in[1][row * p.ldi[1] + c] : 0.f);
          p.out[0][row * p.ldo[0] + c] = a;
          p.out[1][row * p.ldo[1] + c] = h;
          if (p.last) p.out[2][row * p.ldo[2] + c] = p.vec[1][c] * act_d1(p.act, a);
        } else if constexpr (EPI == EPI_BWD) {
          const float gn = p.rho == 0.f ? 0.f : (p.in[0] ? p.in[0][row * p.ldi[0] + c] : p.vec[0][c]);
          const float g = v + p.rho * gn;
          p.out[0][row * p.ldo[0] + c] = g;
          p.out[1][row * p.ldo[1] + c] = g * act_d1(p.act, p.in[1][row * p.ldi[1] + c]);
        } else if constexpr (EPI == EPI_TAN0) {
          p.out[0][row * p.ldo[0] + c] = v;
          if (c < p.lvl0_cols) p.out[1][row * p.ldo[1] + c] = act_d1(p.act, p.in[0][row * p.ldi[0] + c]) * v;
        } else if constexpr (EPI == EPI_TAN) {
          const float ad = v + (p.in[0] ? p.in[0][row * p.ldi[0] + c] : 0.f);
          const float a = p.in[2][row * p.ldi[2] + c];
          float d1, d2;
          act_d12(p.act, a, d1, d2);
          const float hd = d1 * ad + (p.rho != 0.f ? p.rho * p.in[1][row * p.ldi[1] + c] : 0.f);
          p.out[0][row * p.ldo[0] + c] = ad;
          p.out[1][row * p.ldo[1] + c] = hd;
          if (p.last) p.out[2][row * p.ldo[2] + c] = p.vec[0][c] * (p.ubar[row] * d1 + ad * d2);
        } else if constexpr (EPI == EPI_REV) {
          const float pn = p.rho == 0.f ? 0.f : (p.in[0] ? p.in[0][row * p.ldi[0] + c] : p.ubar[row] * p.vec[0][c]);
          const float pv = v + p.rho * pn;
          const float a = p.in[1][row * p.ldi[1] + c];
          float d1, d2;
          act_d12(p.act, a, d1, d2);
          p.out[0][row * p.ldo[0] + c] = pv;
          p.out[1][row * p.ldo[1] + c] =
              pv * d1 + p.in[2][row * p.ldi[2] + c] * p.in[3][row * p.ldi[3] + c] * d2;
        }
      }
    }
  }
}

// --------------------------------------------------------------------------
// u = h . w_out + b_out   (one 16-lane group per row)
// --------------------------------------------------------------------------
#ifndef DBSDE_DEVICE_HELPERS_ONLY
__global__ void __launch_bounds__(256) rowdot_kernel(const float* H, int ldh, int ncols, const float* w,
                                                     const float* b, float* u, int Rp, float* umask) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int cl = threadIdx.x & 15;
  if (row >= Rp) return;
  float s = 0.f;
  for (int c = cl; c < ncols; c += 16) s += H[(size_t)row * ldh + c] * w[c];
  s = red16(s);
  if (cl == 0) {
    const float v = s + b[0];
    if (umask) {   // u = clamp(net, min=0) (heston_dnnpde.py:568); clamp passes the gradient at 0
      umask[row] = v >= 0.f ? 1.f : 0.f;
      u[row] = v >= 0.f ? v : 0.f;
    } else {
      u[row] = v;
    }
  }
}
#endif

// ubar[row] from the per-row residuals; loss partial sums per block.
// rres[r] = Y_{n+1} - Ytilde_{n+1} (n < N), or Y_N - g(X_N) (n == N).
#ifndef DBSDE_DEVICE_HELPERS_ONLY
__global__ void __launch_bounds__(256) ubar_kernel(const float* rres, const float* xin, int ldx, int R, int Rp,
                                                   int N1, float phi_r, const float* lossrow, float* ubar,
                                                   float* u16, double* loss_part, const float* umask,
                                                   const float* dphidy) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  float ub = 0.f;
  double lv = 0.0;
  if (row < R) {
    const int n = row % N1;
    if (n >= 1) ub += 2.f * rres[row - 1];
    if (n < N1 - 1) {
      const float dt = xin[(size_t)(row + 1) * ldx] - xin[(size_t)row * ldx];
      // dphidy (pen != 0): the interior row's d phi / d Y as its cotangent kernel wrote it
      ub += -2.f * rres[row] * (1.f + (dphidy ? dphidy[row] : phi_r) * dt);
    } else {
      ub += 2.f * rres[row];
    }
    if (umask) ub *= umask[row];
    lv = (double)lossrow[row];
  }
  if (row < Rp) {
    ubar[row] = ub;
    u16[(size_t)row * 16] = ub;
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
#endif

// net_u VJP inputs (dbsde_net_u_vjp): the caller's ubar [R] and zbar [R, D]
// as row buffers -- ub [Rp] (zero past R) and z rows [Rp, ldz] (columns
// 1..D, zero elsewhere).  With umask (the per-layer form, Heston u-clamp) the
// values are masked here and u16 (the output-layer operand) is written too.
#ifndef DBSDE_DEVICE_HELPERS_ONLY
__global__ void __launch_bounds__(256) ext_cotan_kernel(const float* ubar, const float* zbar, int R, int Rp, int D,
                                                        int ldz, const float* umask, float* ub, float* zrows,
                                                        float* u16) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i < (long long)Rp * ldz) {
    const int r = (int)(i / ldz), col = (int)(i - (long long)r * ldz);
    const float m = (umask && r < R) ? umask[r] : 1.f;
    zrows[i] = (r < R && col >= 1 && col <= D) ? m * zbar[(size_t)r * D + col - 1] : 0.f;
  }
  if (i < Rp) {
    const float m = (umask && i < R) ? umask[i] : 1.f;
    const float v = i < R ? m * ubar[i] : 0.f;
    ub[i] = v;
    if (u16) u16[(size_t)i * 16] = v;
  }
}
#endif

#ifndef DBSDE_DEVICE_HELPERS_ONLY
__global__ void __launch_bounds__(256) loss_final_kernel(const double* part, int n, float* loss) {
  __shared__ double red[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += part[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)red[0];
}
#endif

// --------------------------------------------------------------------------
// TN reduction GEMM for parameter gradients:
//   C[m, n] = sum_r A0[r, m] B0[r, n] + A1[r, m] B1[r, n]
// split over r into slabs; 64x64 output tile per workgroup (4 waves of 32x32).
// --------------------------------------------------------------------------
struct TNProb {
  const float* A[2];
  int lda[2], nA[2];
  const float* B[2];
  int ldb[2], nB[2];
  int npairs;
  int ones_col;   // pair-0 B column treated as 1.0 (bias gradient); -1 none
  int mv, nv;     // valid output extent
  int mt, nt;     // tiles of 64
  float* slab;    // [splits][mt*64][nt*64]
};
struct TNArgs {
  TNProb prob[8];
  int rows_per_split;
  int Rp;
  int split0;   // tn_x3_kernel: first row split of this launch (piped per path chunk)
};

constexpr int TN_KC = 16;
constexpr int TN_LS = 80;

#ifndef DBSDE_DEVICE_HELPERS_ONLY
__global__ void __launch_bounds__(256) tn_gemm_kernel(TNArgs args) {
  const TNProb& P = args.prob[blockIdx.z];
  const int tile = blockIdx.x;
  if (tile >= P.mt * P.nt) return;
  const int tm = tile / P.nt, tn = tile - tm * P.nt;
  const int split = blockIdx.y;
  const int r_begin = split * args.rows_per_split;
  int r_end = r_begin + args.rows_per_split;
  if (r_end > args.Rp) r_end = args.Rp;
  __shared__ float As[2][TN_KC * TN_LS];
  __shared__ float Bs[2][TN_KC * TN_LS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  // a wave whose 32x32 quadrant lies outside the valid output skips its MFMAs
  const bool active = (tm * 64 + wm * 32 < P.mv) && (tn * 64 + wn * 32 < P.nv);
  floatx4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int lr = tid >> 4, lc = (tid & 15) * 4;  // loader: row in chunk, col (float4)
  const int nch = (r_end > r_begin) ? (r_end - r_begin) / TN_KC : 0;
  const int total = nch * P.npairs;
  floatx4 ar, br;
  auto gload = [&](int it) {
    const int pr = it / nch, ch = it - pr * nch;
    const size_t r = (size_t)(r_begin + ch * TN_KC + lr);
    const int ca = tm * 64 + lc, cb = tn * 64 + lc;
    ar = (ca < P.nA[pr]) ? *(const floatx4*)(P.A[pr] + r * P.lda[pr] + ca) : floatx4{0.f, 0.f, 0.f, 0.f};
    if (cb < P.nB[pr]) {
      br = *(const floatx4*)(P.B[pr] + r * P.ldb[pr] + cb);
    } else {
      br = floatx4{0.f, 0.f, 0.f, 0.f};
      if (pr == 0 && P.ones_col >= cb && P.ones_col < cb + 4) {
        const int o = P.ones_col - cb;
        br = floatx4{o == 0 ? 1.f : 0.f, o == 1 ? 1.f : 0.f, o == 2 ? 1.f : 0.f, o == 3 ? 1.f : 0.f};
      }
    }
  };
  auto sstore = [&](int buf) {
    *(floatx4*)&As[buf][lr * TN_LS + lc] = ar;
    *(floatx4*)&Bs[buf][lr * TN_LS + lc] = br;
  };
  if (total > 0) {
    gload(0);
    sstore(0);
    __syncthreads();
    for (int it = 0; it < total; ++it) {
      const int buf = it & 1;
      if (it + 1 < total) gload(it + 1);
      if (active) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = 4 * i + (lane >> 4);
          float a[2], b[2];
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            a[s] = As[buf][k * TN_LS + wm * 32 + s * 16 + (lane & 15)];
            b[s] = Bs[buf][k * TN_LS + wn * 32 + s * 16 + (lane & 15)];
          }
#pragma unroll
          for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[x][y] = mfma4(a[x], b[y], acc[x][y]);
        }
      }
      if (it + 1 < total) sstore(buf ^ 1);
      __syncthreads();
    }
  }
  const int ldc = P.nt * 64;
  float* C = P.slab + (size_t)split * (P.mt * 64) * ldc;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = tm * 64 + wm * 32 + x * 16 + (lane >> 4) * 4 + j;
        const int n = tn * 64 + wn * 32 + y * 16 + (lane & 15);
        C[(size_t)m * ldc + n] = acc[x][y][j];
      }
}
#endif

#ifndef DBSDE_DEVICE_HELPERS_ONLY
__global__ void __launch_bounds__(256) fill_col0_kernel(float* buf, int ld, long long rows, float v) {
  const long long r = blockIdx.x * 256LL + threadIdx.x;
  if (r < rows) buf[r * ld] = v;
}
#endif

// --------------------------------------------------------------------------
// Descriptor-driven gather/scatter (weight packing, gradient finalize)
// --------------------------------------------------------------------------
enum PackMode { PK_COPY = 0, PK_ADD2 = 1, PK_NEGPROJ = 2, PK_SLABSUM = 3 };
constexpr int NAIS_LMAX = 128;   // NAIS projection matrices: L x L, L <= 128 (rtr / proj kernels)
// |R|_F from the rtr partials (at most 64, one per lane) in a fixed order: a
// xor butterfly, the order pack_tagged_kernel's norm also follows
__device__ __forceinline__ double nais_norm_from(double part_of_lane) {
  double sq = part_of_lane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
  return sqrt(sq);
}
struct PackDesc {
  const float* src;
  const float* src2;   // PK_ADD2 second source
  int src_ld, src2_ld;
  float* dst;
  int dst_ld;
  int rows, cols;
  int transpose;       // dst[c][r] = v(r, c)
  int mode;
  float scale;         // PK_COPY / PK_SLABSUM / PK_ADD2 multiplier
  int nslab;           // PK_SLABSUM: slabs of stride slab_stride
  long long slab_stride;
  const double* proj;  // PK_NEGPROJ: the |R_j|^2 partial sums of this block (rtr_params_kernel)
  int proj_n;          //   number of partials
  double* proj_norm;   //   |R_j|_F written here by block 0 (for the backward)
  const float* dotR;   // PK_SLABSUM into Abar_j: R_j (same layout as dst); the block's
  double* dot_part;    //   partial <Abar_j, R_j> goes to dot_part[blockIdx.x]
  // optional second destination: an MFMA fragment image (phase.hpp) of the
  // logical [out][in] matrix, element (dr + frow0, dc + fcol0) with
  // (dr, dc) = transpose ? (c, r) : (r, c); ftin = 16-col input blocks
  float* fdst;
  int ftin, frow0, fcol0;
  int ftout;           // > 0: t-major image (phase.hpp), fragment (o, t) at t * ftout + o
  int fsplit;          // 1: split-bf16 image (x3_off), fdst holds bf16 triples
  int sp, sr0, sc0;    // tilefin_kernel: the window's problem tile and its first row / column
};
// bf16 offset of W[o][i] in a split-bf16 fragment image (phase.hpp, X3 kernels)
// with tout 16-row output blocks: fragment (o/16, kb = i/32) at kb * tout + o/16,
// 3 KiB = [hi | mid | lo] x 64 lanes x 8 bf16; lane (o%16) + 16 q, element j
// for input column i = 32 kb + 16 (j >> 2) + 4 q + (j & 3) -- the permuted k
// order in which a 16x16 MFMA output tile pair is already the next layer's
// 16x16x32 B operand.  The mid / lo parts sit 512 / 1024 bf16 further on.
__host__ __device__ __forceinline__ long long x3_off(int o, int i, int tout) {
  const int ii = i & 31, q = (ii >> 2) & 3, j = ((ii >> 4) << 2) | (ii & 3);
  const long long f = (long long)(i >> 5) * tout + (o >> 4);
  return f * 1536 + ((o & 15) + 16 * q) * 8 + j;
}
// float offset of W[o][i] in a fragment image with tin input / tout output
// blocks: fragment (o/16, i/16) -- o-major (phase.hpp) or, when tout > 0,
// t-major (phase3.hpp) -- lane (o%16) + 16 ((i/4)%4), component i%4
__host__ __device__ __forceinline__ long long frag_off(int o, int i, int tin, int tout) {
  const long long f = tout > 0 ? (long long)(i >> 4) * tout + (o >> 4) : (long long)(o >> 4) * tin + (i >> 4);
  return ((f * 64 + (o & 15) + 16 * ((i >> 2) & 3)) << 2) + (i & 3);
}

// --------------------------------------------------------------------------
// clip_grad_norm_ + Adam/AdamW/SGD (nd_BSPDE_case.py:383-384; torch defaults)
// --------------------------------------------------------------------------
#ifndef DBSDE_DEVICE_HELPERS_ONLY
__global__ void __launch_bounds__(256) sqnorm_kernel(const float* g, const unsigned char* used, long long n,
                                                     double* part) {
  __shared__ double red[256];
  double s = 0.0;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    if (used[i]) s += (double)g[i] * (double)g[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
#endif

// optimizer kinds (include/dbsde.h DBSDE_OPT_*), each in torch.optim's
// single-tensor formula order (the reference's CPU path; torch 2.10)
enum OptKind { OPT_ADAM = 0, OPT_ADAMW, OPT_SGD, OPT_RMSPROP, OPT_ADAGRAD, OPT_ADAMAX, OPT_ADADELTA, OPT_ASGD };

struct OptArgs {
  int kind;
  float lr, beta2, eps, wd, max_norm;
  float omb1, omb2;           // 1-beta1, 1-beta2 (computed in double, as torch's Python floats)
  float step_size, bc2_sqrt;  // Adam: lr/(1-beta1^t), sqrt(1-beta2^t); Adamax/Adagrad: the step's clr
  float alpha, rho;           // RMSprop alpha / Adadelta rho
  float asgd_decay, asgd_eta; // ASGD: 1 - lambd*eta (double, cast), eta
  int asgd_copy;              // ASGD: mu == 1 -> ax = p
  float asgd_mu;
  const float* loss;          // nullable: skip the whole update when the loss is not finite
  int nparts;
  // device step counter (nullable): the step-dependent scalars above are then
  // derived on the device from step = state[parity] + 1, and the count advances
  // (state[1 - parity]) only when the update is not skipped
  double* state;
  int parity;
  double lr_d, beta1_d, beta2_d, lr_decay_d, lambd_d, asgd_alpha_d, asgd_t0_d;
};

// torch.optim's Python-float scalars of update number t (torch 2.10
// single-tensor paths): Adam/AdamW/Adamax bias corrections, Adagrad's clr and
// ASGD's eta / mu, which torch computes after step t - 1 and keeps as fp32
__device__ inline void opt_step_scalars(OptArgs& a, double t) {
  const double bc1 = 1.0 - pow(a.beta1_d, t), bc2 = 1.0 - pow(a.beta2_d, t);
  a.step_size = (float)(a.lr_d / bc1);
  a.bc2_sqrt = (float)sqrt(bc2);
  if (a.kind == OPT_ADAGRAD) a.step_size = (float)(a.lr_d / (1.0 + (t - 1.0) * a.lr_decay_d));
  if (a.kind == OPT_ASGD) {
    const double tp = t - 1.0;   // eta / mu were set by the previous step (lr and 1 before the first)
    const float eta = tp < 1.0 ? (float)a.lr_d : (float)(a.lr_d / pow(1.0 + a.lambd_d * a.lr_d * tp, a.asgd_alpha_d));
    const float mu = tp < 1.0 ? 1.f : (float)(1.0 / fmax(1.0, tp - a.asgd_t0_d));
    a.asgd_eta = eta;
    a.asgd_decay = (float)(1.0 - a.lambd_d * (double)eta);
    a.asgd_mu = mu;
    a.asgd_copy = mu == 1.f;
  }
}

// a parameter element and its moments, loaded ahead of the update (the
// finalize kernels issue these loads with their operand loads)
struct OptVals {
  float p, m, v;
};
__device__ __forceinline__ OptVals opt_load(long long i, const float* prm, const float* m, const float* v) {
  return OptVals{prm[i], m ? m[i] : 0.f, v ? v[i] : 0.f};
}
// one parameter element of the update: params / moments at index i (their
// values pv), its (clipped) gradient gi
__device__ __forceinline__ void opt_apply(const OptArgs& a, long long i, float gi, OptVals pv, float* prm, float* m,
                                          float* v) {
  // every product and sum rounded as written (torch's op-by-op formulas), and
  // the same in every kernel that inlines this (optim_kernel, the finalize)
#pragma clang fp contract(off)
  float p = pv.p;
  switch (a.kind) {
    case OPT_SGD: {
      if (a.wd != 0.f) gi = gi + a.wd * p;
      prm[i] = p - a.lr * gi;
      break;
    }
    case OPT_RMSPROP: {   // square_avg.mul_(alpha).addcmul_(g, g, 1-alpha); p.addcdiv_(g, sqrt(sa)+eps, -lr)
      if (a.wd != 0.f) gi = gi + a.wd * p;
      const float sa = pv.v * a.alpha + a.omb2 * gi * gi;
      v[i] = sa;
      prm[i] = p + (-a.lr) * (gi / (sqrtf(sa) + a.eps));
      break;
    }
    case OPT_ADAGRAD: {   // state_sum.addcmul_(g, g, 1); p.addcdiv_(g, sqrt(ss)+eps, -clr)
      if (a.wd != 0.f) gi = gi + a.wd * p;
      const float ss = pv.v + gi * gi;
      v[i] = ss;
      prm[i] = p + (-a.step_size) * (gi / (sqrtf(ss) + a.eps));
      break;
    }
    case OPT_ADAMAX: {    // exp_avg.lerp_(g, 1-b1); exp_inf = max(exp_inf*b2, |g|+eps); p.addcdiv_(m, u, -clr)
      if (a.wd != 0.f) gi = gi + a.wd * p;
      const float mi = pv.m + a.omb1 * (gi - pv.m);
      const float ui = fmaxf(pv.v * a.beta2, fabsf(gi) + a.eps);
      m[i] = mi;
      v[i] = ui;
      prm[i] = p + (-a.step_size) * (mi / ui);
      break;
    }
    case OPT_ADADELTA: {  // sq.mul_(rho).addcmul_(g,g,1-rho); d = sqrt(acc+eps)/sqrt(sq+eps)*g; acc.mul_(rho).addcmul_(d,d,1-rho)
      if (a.wd != 0.f) gi = gi + a.wd * p;
      const float sq = pv.v * a.rho + a.omb2 * gi * gi;
      const float dl = sqrtf(pv.m + a.eps) / sqrtf(sq + a.eps) * gi;
      v[i] = sq;
      m[i] = pv.m * a.rho + a.omb2 * dl * dl;
      prm[i] = p + (-a.lr) * dl;
      break;
    }
    case OPT_ASGD: {      // p.mul_(1 - lambd eta); p.add_(g, -eta); ax = p (mu == 1) or ax += (p - ax) mu
      if (a.wd != 0.f) gi = gi + a.wd * p;
      p = p * a.asgd_decay;
      p = p + (-a.asgd_eta) * gi;
      prm[i] = p;
      m[i] = a.asgd_copy ? p : pv.m + (p - pv.m) * a.asgd_mu;
      break;
    }
    default: {            // Adam / AdamW
      if (a.kind == OPT_ADAMW) p = p * (1.f - a.lr * a.wd);   // decoupled decay
      else if (a.wd != 0.f) gi = gi + a.wd * p;                // Adam L2
      float mi = pv.m;
      mi = mi + a.omb1 * (gi - mi);                            // exp_avg.lerp_(g, 1-beta1)
      float vi = pv.v * a.beta2 + a.omb2 * gi * gi;            // mul_(beta2).addcmul_(g, g, 1-beta2)
      m[i] = mi;
      v[i] = vi;
      const float denom = sqrtf(vi) / a.bc2_sqrt + a.eps;
      prm[i] = p - a.step_size * (mi / denom);                 // addcdiv_(m, denom, -step_size)
    }
  }
}

__device__ __forceinline__ void opt_update(const OptArgs& a, long long i, float gi, float* prm, float* m, float* v) {
  opt_apply(a, i, gi, opt_load(i, prm, m, v), prm, m, v);
}

#ifndef DBSDE_DEVICE_HELPERS_ONLY
__global__ void __launch_bounds__(256) optim_kernel(float* prm, float* g, float* m, float* v, const unsigned char* used,
                                                    long long n, const double* part, OptArgs a) {
  __shared__ float clip_s;
  __shared__ int skip_s;
  __shared__ OptArgs a_s;
  // the squared-norm partials summed by wave 0 (lane l: partials l, l + 64,
  // ...; then a fixed xor butterfly): one thread summing 256 of them in
  // series left every block waiting on dependent global loads
  double ssq = 0.0;
  if (threadIdx.x < 64 && a.max_norm > 0.f) {
    for (int i = threadIdx.x; i < a.nparts; i += 64) ssq += part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ssq += __shfl_xor(ssq, o);
  }
  if (threadIdx.x == 0) {
    float coef = 1.f;
    if (a.max_norm > 0.f) {
      const float tot = (float)sqrt(ssq);
      coef = a.max_norm / (tot + 1e-6f);
      if (coef > 1.f) coef = 1.f;
    }
    clip_s = coef;
    const int skip = a.loss ? !isfinite(a.loss[0]) : 0;   // heston_dnnpde.py:409-411 NaN skip
    skip_s = skip;
    if (a.state) {
      // every block reads state[parity]; only block 0 writes the other slot
      const double done = a.state[a.parity];
      opt_step_scalars(a, done + 1.0);
      if (blockIdx.x == 0) a.state[1 - a.parity] = skip ? done : done + 1.0;
    }
    a_s = a;
  }
  __syncthreads();
  if (skip_s) return;
  a = a_s;
  const float coef = clip_s;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    if (!used[i]) continue;
    const float gi = g[i] * coef;
    g[i] = gi;
    opt_update(a, i, gi, prm, m, v);
  }
}
#endif

// The optimizer folded into the gradient finalize (single process, no clip,
// no NaN skip, device step counter): every finalize thread that writes the
// gradient of a parameter element also applies the update to it, so the
// step needs no separate optimizer launch.  step_writer: the one block that
// advances the counter.
struct FusedOpt {
  float *prm, *m, *v;
  OptArgs a;   // a.state set (device step count)
};
__device__ __forceinline__ void fused_opt_prologue(FusedOpt& fo, bool step_writer) {
  __shared__ OptArgs fa_s;
  if (threadIdx.x == 0) {
    const double done = fo.a.state[fo.a.parity];
    opt_step_scalars(fo.a, done + 1.0);
    if (step_writer) fo.a.state[1 - fo.a.parity] = done + 1.0;
    fa_s = fo.a;
  }
  __syncthreads();
  fo.a = fa_s;
}

// --------------------------------------------------------------------------
// output export: rows -> reference layouts
// --------------------------------------------------------------------------
#ifndef DBSDE_DEVICE_HELPERS_ONLY
// zmask (nullable): the u-clamp gradient mask (heston_dnnpde.py:568) for a
// Z that is not masked yet (the per-layer net_u's plain Z GEMM)
__global__ void __launch_bounds__(256) export_kernel(const float* xin, const float* zfull, int ldx, const float* u,
                                                     int R, int D, float* X, float* Y, float* Z,
                                                     const float* zmask) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= (long long)R * D) return;
  const long long r = i / D;
  const int d = (int)(i - r * D);
  if (X) X[i] = xin[r * ldx + 1 + d];
  if (Z) Z[i] = zmask ? zfull[r * ldx + 1 + d] * zmask[r] : zfull[r * ldx + 1 + d];
  if (Y && d == 0) Y[r] = u[r];
}
#endif

// net_u input rows: xin[r] = [t_r, X_r, 1, 0..]
#ifndef DBSDE_DEVICE_HELPERS_ONLY
__global__ void __launch_bounds__(256) netu_input_kernel(const float* t, const float* X, int R, int D, int ldx,
                                                         float* xin) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= (long long)R * ldx) return;
  const long long r = i / ldx;
  const int c = (int)(i - r * ldx);
  float v = 0.f;
  if (c == 0) v = t[r];
  else if (c <= D) v = X[r * D + c - 1];
  else if (c == D + 1) v = 1.f;
  xin[i] = v;
}
#endif

// grad[...] = scale * sum_k slab_k[...] for each PK_SLABSUM descriptor:
// 64 elements per block, the slabs split over 4 thread groups whose fp64
// partials are added in a fixed order.
#ifndef DBSDE_DEVICE_HELPERS_ONLY
// Output-layer weight gradient of the chain layouts (u = h_K . w_out + b_out,
// loss.backward, DeepBSDE.py:279): for row split s (rows [s rps, (s+1) rps)
// of the R valid rows), row 0 of slab s = [sum_r ubar_r h_K[r] + hdot_K[r] |
// sum_r ubar_r] -- the [w_out | b_out] window the finalize reads.  A GEMV
// over the two level-K tiles, HBM-bound: 1024 threads = 16 row phases x 64
// float4 column groups (a wave reads whole 1 KB rows), 8 rows in flight per
// thread, the phases combined in a fixed order.  grid (splits, ceil(W / 256)).
__global__ void __launch_bounds__(1024) tn_out_kernel(const float* u16, const float* H, const float* Hd, int ld,
                                                      int W, int R, int rps, float* slab, long long sstride,
                                                      int s0) {
  const int s = s0 + (int)blockIdx.x, t = threadIdx.x, cg = t & 63, ph = t >> 6;
  const int c = blockIdx.y * 256 + 4 * cg;
  const bool cin = c < W;   // W % 4 == 0
  const int r0 = s * rps, r1 = min(r0 + rps, R);
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int rb = r0 + ph; rb < r1; rb += 16 * 8) {
    floatx4 h[8], hd[8];
    float ub[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = rb + 16 * u;
      const bool ok = r < r1 && cin;
      const size_t o = (size_t)(ok ? r : r0) * ld + (cin ? c : 0);
      h[u] = *(const floatx4*)(H + o);
      hd[u] = *(const floatx4*)(Hd + o);
      ub[u] = r < r1 ? u16[(size_t)r * 16] : 0.f;
      if (!ok) {
        h[u] = floatx4{0.f, 0.f, 0.f, 0.f};
        hd[u] = floatx4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += ub[u] * h[u][e] + hd[u][e];
      bsum += ub[u];
    }
  }
  __shared__ floatx4 part[16][64];
  __shared__ float bpart[16];
  part[ph][cg] = acc;
  if (cg == 0) bpart[ph] = bsum;
  __syncthreads();
  if (ph != 0) return;
  floatx4 v[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = part[k][cg];
#pragma unroll
  for (int h = 1; h < 16; h <<= 1)
#pragma unroll
    for (int k = 0; k + h < 16; k += 2 * h) v[k] += v[k + h];
  float* row = slab + (size_t)s * sstride;
  if (cin) *(floatx4*)(row + c) = v[0];
  if (blockIdx.y == 0 && cg == 0) {
    float b[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) b[k] = bpart[k];
#pragma unroll
    for (int h = 1; h < 16; h <<= 1)
#pragma unroll
      for (int k = 0; k + h < 16; k += 2 * h) b[k] += b[k + h];
    row[W] = b[0];
  }
}

// nslab: the slabs the weight-gradient launch wrote (its row splits); a
// descriptor's own nslab is the capacity (0: a zero window)
// loss (nullable): block (0, 0) also sums the loss partials into it, in
// loss_final_kernel's fixed order (one launch fewer)
__global__ void __launch_bounds__(256) slabsum_kernel(const PackDesc* descs, float* grad, int nslab,
                                                      const double* loss_part, int nloss, float* loss) {
  if (loss && blockIdx.x == 0 && blockIdx.y == 0) {
    __shared__ double red[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < nloss; i += 256) a += loss_part[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)red[0];
  }
  PackDesc d = descs[blockIdx.y];
  if (d.nslab > 0) d.nslab = nslab;
  const int total = d.rows * d.cols;
  if ((int)blockIdx.x * 64 >= total) return;
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  double s = 0.0;
  int r = 0, cc = 0;
  if (e < total) {
    r = e / d.cols;
    cc = e - r * d.cols;
    const float* src = d.src + (size_t)r * d.src_ld + cc;
    const int k0 = grp * d.nslab / 4, k1 = (grp + 1) * d.nslab / 4;
    // 8 slabs per round, all loads in flight before the (fixed-order) sum: a
    // wave's share is 2-24 slabs, so a 32-slab round never ran and the tail
    // loop left one load in flight at a time
    int k = k0;
    for (; k + 8 <= k1; k += 8) {
      float x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = src[(size_t)(k + u) * d.slab_stride];
      s += (((double)x[0] + (double)x[1]) + ((double)x[2] + (double)x[3])) +
           (((double)x[4] + (double)x[5]) + ((double)x[6] + (double)x[7]));
    }
    for (; k < k1; ++k) s += src[(size_t)k * d.slab_stride];
  }
  __shared__ double part[4][64];
  part[grp][lane] = s;
  __syncthreads();
  if (grp == 0) {
    double dp = 0.0;
    if (e < total) {
      const float v = d.scale * (float)((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]));
      uintptr_t dv = (uintptr_t)d.dst;
      float* dst = (dv & ((uintptr_t)1 << 61)) ? grad + ((dv & (((uintptr_t)1 << 61) - 1)) >> 2) : d.dst;
      if (d.transpose)
        dst[(size_t)cc * d.dst_ld + r] = v;
      else
        dst[(size_t)r * d.dst_ld + cc] = v;
      if (d.dotR) dp = (double)v * (double)d.dotR[(size_t)r * d.dst_ld + cc];
    }
    if (d.dotR) {   // fixed-order wave reduction of the block's <Abar, R> partial
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) dp += __shfl_xor(dp, o);
      if (lane == 0) d.dot_part[blockIdx.x] = dp;
    }
  }
}
#endif

// Weight-gradient finalize of the wave-owned tiles (tnw.hpp): one pass over
// each problem's T x T slab tile, float4 per lane (whole 128-byte lines, no
// descriptor-window overfetch), the S slabs split over the 4 waves and summed
// in fp64 in a fixed order; each summed element is then scattered to every
// descriptor window that covers it (W, biases, Abar + its <Abar, R> partial).
// grid (ceil(T*T / 256), P + 1): y = P zero-fills the nslab == 0 windows.
constexpr int TF_ELEMS = 256;   // elements per block (64 lanes x float4)
constexpr int TF_WMAX = 16;     // descriptor windows per problem tile
constexpr int TNW_PMAX_FIN = 16;   // problem tiles of the wave-owned layouts (2K + 2 <= 14)
// The finalize's descriptor windows grouped by problem on the host (one row
// per problem p < P, row P = the zero windows): a block loads its row with one
// parallel copy instead of scanning every descriptor in thread 0 (a chain of
// dependent global loads, ~17 round trips per block)
struct TileFinTable {
  int n[TNW_PMAX_FIN + 1];
  PackDesc w[TNW_PMAX_FIN + 1][TF_WMAX];
};
#ifndef DBSDE_DEVICE_HELPERS_ONLY
// the block's window row into LDS: every thread copies dwords in parallel
__device__ __forceinline__ int tilefin_windows(const TileFinTable* tab, int p, PackDesc* wins) {
  constexpr int NW = (int)(sizeof(PackDesc) * TF_WMAX / 4);
  const unsigned* src = (const unsigned*)&tab->w[p][0];
  unsigned* dst = (unsigned*)wins;
  for (int i = threadIdx.x; i < NW; i += blockDim.x) dst[i] = src[i];
  return tab->n[p];
}
__global__ void __launch_bounds__(256) tilefin_kernel(const TileFinTable* tab, const float* slab, int S, int P, int T,
                                                      float* grad, const double* loss_part, int nloss, float* loss,
                                                      FusedOpt fo, int fuse) {
  const int p = blockIdx.y;
  __shared__ PackDesc wins[TF_WMAX];
  const int nwin = tilefin_windows(tab, p, wins);
  if (p == P) {   // zero windows (NAIS-Net's never-used input_layers[K])
    if (fuse) fused_opt_prologue(fo, blockIdx.x == 0);
    // and, in block 0, the loss sum (loss_final_kernel's fixed order: one
    // launch fewer on the step's critical path)
    if (loss && blockIdx.x == 0) {
      __shared__ double red[256];
      double a = 0.0;
      for (int i = threadIdx.x; i < nloss; i += 256) a += loss_part[i];
      red[threadIdx.x] = a;
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
      }
      if (threadIdx.x == 0) loss[0] = (float)red[0];
    }
    __syncthreads();
    for (int i = 0; i < nwin; ++i) {
      const PackDesc& d = wins[i];
      uintptr_t dv = (uintptr_t)d.dst;
      float* dst = (dv & ((uintptr_t)1 << 61)) ? grad + ((dv & (((uintptr_t)1 << 61) - 1)) >> 2) : d.dst;
      const int total = d.rows * d.cols;
      for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) dst[e] = 0.f;
    }
    return;
  }
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int TT = T * T;
  const int e0 = blockIdx.x * TF_ELEMS + 4 * lane;   // T % 4 == 0: the float4 stays in one row
  const long long stride = (long long)P * TT;
  double s4[4] = {0.0, 0.0, 0.0, 0.0};
  if (e0 < TT) {
    const float* src = slab + (size_t)p * TT + e0;
    const int k0 = grp * S / 4, k1 = (grp + 1) * S / 4;
    int k = k0;
    for (; k + 16 <= k1; k += 16) {
      floatx4 x[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) x[u] = *(const floatx4*)(src + (size_t)(k + u) * stride);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          q[u] = ((double)x[4 * u][c] + (double)x[4 * u + 1][c]) + ((double)x[4 * u + 2][c] + (double)x[4 * u + 3][c]);
        s4[c] += (q[0] + q[1]) + (q[2] + q[3]);
      }
    }
    for (; k < k1; ++k) {
      const floatx4 x = *(const floatx4*)(src + (size_t)k * stride);
#pragma unroll
      for (int c = 0; c < 4; ++c) s4[c] += (double)x[c];
    }
  }
  // the optimizer scalars after the slab loads are in flight (its global
  // load and barrier overlap them)
  if (fuse) fused_opt_prologue(fo, false);
  __shared__ double part[4][4][64];
  __shared__ double dps[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) part[grp][c][lane] = s4[c];
  __syncthreads();
  // wave grp scatters (and updates) component grp of the lane's four
  // columns: the four waves' optimizer read-modify-writes run side by side
  // instead of four dependent rounds in one wave
  double dp = 0.0;
  const PackDesc* dotd = nullptr;
  if (e0 < TT) {
    const int r = e0 / T, c00 = e0 - r * T, c = grp;
    const double v = (part[0][c][lane] + part[1][c][lane]) + (part[2][c][lane] + part[3][c][lane]);
    const int cc = c00 + c;
    for (int i = 0; i < nwin; ++i) {
      const PackDesc& d = wins[i];
      const int rr = r - d.sr0, ck = cc - d.sc0;
      if (rr < 0 || rr >= d.rows || ck < 0 || ck >= d.cols) continue;
      const float fv = d.scale * (float)v;
      uintptr_t dv = (uintptr_t)d.dst;
      const bool to_grad = dv & ((uintptr_t)1 << 61);
      float* dst = to_grad ? grad + ((dv & (((uintptr_t)1 << 61) - 1)) >> 2) : d.dst;
      const size_t off = d.transpose ? (size_t)ck * d.dst_ld + rr : (size_t)rr * d.dst_ld + ck;
      dst[off] = fv;
      if (fuse && to_grad) opt_update(fo.a, (dst - grad) + (long long)off, fv, fo.prm, fo.m, fo.v);
      if (d.dotR) dp += (double)fv * (double)d.dotR[(size_t)rr * d.dst_ld + ck];
    }
  }
  for (int i = 0; i < nwin; ++i)
    if (wins[i].dotR) dotd = &wins[i];
  if (dotd) {   // the block's <Abar, R> partial: each wave's sum, then the waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dp += __shfl_xor(dp, o);
    if (lane == 0) dps[grp] = dp;
    __syncthreads();
    if (threadIdx.x == 0) dotd->dot_part[blockIdx.x] = (dps[0] + dps[1]) + (dps[2] + dps[3]);
  }
}

// tagged-pointer fixup happens inside a thin wrapper kernel
__device__ __forceinline__ const float* untag(const float* p, const float* params, const float* grad) {
  uintptr_t v = (uintptr_t)p;
  if (v & ((uintptr_t)1 << 62)) return params + ((v & (((uintptr_t)1 << 61) - 1)) >> 2);
  if (v & ((uintptr_t)1 << 61)) return grad + ((v & (((uintptr_t)1 << 61) - 1)) >> 2);
  return p;
}
__device__ __forceinline__ void pack_block(const PackDesc* descs, int di, const float* params, float* grad) {
  PackDesc d = descs[di];
  d.src = untag(d.src, params, grad);
  d.src2 = untag(d.src2, params, grad);
  d.dst = (float*)untag(d.dst, params, grad);
  const int total = d.rows * d.cols;
  if ((int)blockIdx.x * 256 >= total) return;
  // the first element's source value in the round of the norm partials below
  const int i0 = blockIdx.x * 256 + threadIdx.x;
  const float rv0 = (d.mode == PK_NEGPROJ && i0 < total) ? d.src[(size_t)(i0 / d.cols) * d.src_ld + i0 % d.cols] : 0.f;
  // NAIS projection: |RtR|_F from rtr_params_kernel's partials (fixed order)
  __shared__ float nrm_s;
  if (d.mode == PK_NEGPROJ) {
    if (threadIdx.x < 64) {   // wave 0: lane b holds partials b, b + 64, ... ; fixed-order butterfly
      double sq = 0.0;
      for (int b = threadIdx.x; b < d.proj_n; b += 64) sq += d.proj[b];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
      if (threadIdx.x == 0) {
        const double n = sqrt(sq);
        nrm_s = (float)n;
        if (blockIdx.x == 0 && d.proj_norm) *d.proj_norm = n;
      }
    }
    __syncthreads();
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int r = i / d.cols, cc = i - r * d.cols;
    float v;
    if (d.mode == PK_COPY) {
      v = d.scale * d.src[(size_t)r * d.src_ld + cc];
    } else if (d.mode == PK_ADD2) {
      v = d.src[(size_t)r * d.src_ld + cc] + d.src2[(size_t)r * d.src2_ld + cc];
    } else if (d.mode == PK_NEGPROJ) {
      const float rv = i == i0 ? rv0 : d.src[(size_t)r * d.src_ld + cc];
      const float nrm = nrm_s;
      float a = rv;
      if (nrm > 0.98f) a = ((float)0.98994949366116658 * rv) / sqrtf(nrm);
      a = a + (r == cc ? 0.01f : 0.f);
      v = -a;
    } else {
      const float* src = d.src + (size_t)r * d.src_ld + cc;
      double sa[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      int k = 0;
      for (; k + 8 <= d.nslab; k += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) sa[u] += src[(size_t)(k + u) * d.slab_stride];
      }
      for (; k < d.nslab; ++k) sa[0] += src[(size_t)k * d.slab_stride];
      const double s0 = (sa[0] + sa[1]) + (sa[2] + sa[3]), s1 = (sa[4] + sa[5]) + (sa[6] + sa[7]);
      const double s2 = 0.0, s3 = 0.0;
      v = d.scale * (float)((s0 + s1) + (s2 + s3));
    }
    if (d.dst) {
      if (d.transpose)
        d.dst[(size_t)cc * d.dst_ld + r] = v;
      else
        d.dst[(size_t)r * d.dst_ld + cc] = v;
    }
    if (d.fdst) {
      const int dr = (d.transpose ? cc : r) + d.frow0, dc = (d.transpose ? r : cc) + d.fcol0;
      if (d.fsplit) {
        // v = hi + mid + lo exactly: hi, mid rounded to nearest even, lo the
        // remainder (phase.hpp split_two)
        unsigned short* img = (unsigned short*)d.fdst + x3_off(dr, dc, d.ftout);
        const __bf16 h = (__bf16)v;
        const float r1 = v - (float)h;
        const __bf16 m = (__bf16)r1;
        const float r2 = r1 - (float)m;
        img[0] = __builtin_bit_cast(unsigned short, h);
        img[512] = __builtin_bit_cast(unsigned short, m);
        img[1024] = (unsigned short)(__float_as_uint(r2) >> 16);
      } else {
        d.fdst[frag_off(dr, dc, d.ftin, d.ftout)] = v;
      }
    }
  }
}
__global__ void __launch_bounds__(256) pack_tagged_kernel(const PackDesc* descs, const float* params, float* grad) {
  pack_block(descs, blockIdx.y, params, grad);
}
// RtR_j = W_j^T W_j (Functions/naisnet.py:33) and per-tile partial sums of
// squares for the Frobenius norm (fixed order).  One 16x16 output tile per
// 256-thread workgroup; the whole 16 x L and L x 16 operand strips (L <= 128)
// are staged in LDS with one round of independent loads (a K-tiled loop would
// chain L/16 dependent global-load latencies).
__device__ __forceinline__ void rtr_tile(const float* params, const long long* woffs, int L, float* const* rtr,
                                         float* const* wsnap, double* part, int nblk, int j, int tile) {
  __shared__ float As[16][NAIS_LMAX + 1];   // As[r][k] = W[k][16 ti + r]
  __shared__ float Bs[NAIS_LMAX][17];       // Bs[k][c] = W[k][16 tj + c]
  const int nt = (L + 15) / 16;
  const int ti = tile / nt, tj = tile % nt;
  const float* W = params + woffs[j];
  // every operand load in one round (a strided loop waited for each load
  // before the next: ~7 dependent global round trips)
  constexpr int PER = NAIS_LMAX * 16 / 256;
  float av[PER], bv[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = threadIdx.x + 256 * u;
    const int k = e >> 4, q = e & 15;
    const int ra = 16 * ti + q, cb = 16 * tj + q;
    av[u] = (k < L && ra < L) ? W[k * L + ra] : 0.f;
    bv[u] = (k < L && cb < L) ? W[k * L + cb] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = threadIdx.x + 256 * u;
    const int k = e >> 4, q = e & 15;
    if (k < L) {
      As[q][k] = av[u];
      Bs[k][q] = bv[u];
    }
  }
  __syncthreads();
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float v = 0.f;
  for (int k = 0; k < L; ++k) v += As[ty][k] * Bs[k][tx];
  const int row = ti * 16 + ty, col = tj * 16 + tx;
  // snapshot of W_j before this step's update (one 16 x 16 tile per block):
  // the fused optimizer update rewrites params while proj_backward_kernel's
  // other blocks still read W_j
  if (row < L && col < L) wsnap[j][row * L + col] = W[row * L + col];
  double sq = 0.0;
  if (row < L && col < L) {
    rtr[j][row * L + col] = v;
    sq = (double)v * (double)v;
  }
  __shared__ double red[256];
  red[threadIdx.x] = sq;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[j * nblk + tile] = red[0];
}
__global__ void __launch_bounds__(256) rtr_params_kernel(const float* params, const long long* woffs, int L,
                                                         float* const* rtr, float* const* wsnap, double* part, int nblk) {
  rtr_tile(params, woffs, L, rtr, wsnap, part, nblk, blockIdx.y, blockIdx.x);
}
// NAIS projection adjoint (Functions/naisnet.py:30-39 reversed), one kernel:
//   Abar_j = dL/dA_j (slab sums), R_j = W_j^T W_j, n = |R_j|_F
//   Rbar   = c n^-1/2 (Abar - 1/2 <Abar, R> R / n^2)  (Q4 branch taken, c = sqrt 0.98)
//          = Abar                                     (not taken)
//   Wbar_j = W_j (Rbar + Rbar^T)  -> grad
// Every block recomputes <Abar_j, R_j> in the same fixed order (L^2 products,
// cheap), so no separate reduction launch is needed; S = Rbar + Rbar^T is
// formed on the fly in the B tile of the LDS-tiled GEMM.
__global__ void __launch_bounds__(256) proj_backward_kernel(const float* const* wsnap, const long long* woffs,
                                                            float* const* abar, float* const* rtr, int L,
                                                            const double* proj_part, int proj_n, const double* dot_part,
                                                            int dot_nblk, int dot_nused, float* grad, FusedOpt fo,
                                                            int fuse) {
  __shared__ float As[16][NAIS_LMAX + 1];   // As[r][k] = W[16 ti + r][k]
  __shared__ float Bs[NAIS_LMAX][17];       // Bs[k][c] = S[k][16 tj + c], S = Rbar + Rbar^T
  __shared__ double dot_s, nrm_s;
  const int j = blockIdx.y, nt = (L + 15) / 16;
  const int ti = blockIdx.x / nt, tj = blockIdx.x % nt;
  const float* Ab = abar[j];
  const float* R = rtr[j];
  // W_j from the snapshot rtr_params_kernel took: with the fused update, the
  // blocks (ti, tj') of this launch rewrite params' W_j rows in place while
  // this block still reads them
  const float* W = wsnap[j];
  // every operand load in one round, before the scalars are known
  constexpr int PER = NAIS_LMAX * 16 / 256;
  float wv[PER], abs_[PER], rs[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = threadIdx.x + 256 * u;
    const int k = e >> 4, q = e & 15;
    const int ra = 16 * ti + q, cb = 16 * tj + q;
    const bool in = k < L;
    wv[u] = (in && ra < L) ? W[ra * L + k] : 0.f;
    const bool ok = in && cb < L;
    abs_[u] = ok ? Ab[k * L + cb] + Ab[cb * L + k] : 0.f;
    rs[u] = ok ? R[k * L + cb] + R[cb * L + k] : 0.f;
  }
  // this thread's parameter / moments for the fused update, in the same round
  const int row = ti * 16 + (threadIdx.x >> 4), col = tj * 16 + (threadIdx.x & 15);
  const bool own = row < L && col < L;
  const long long gi_idx = own ? woffs[j] + row * L + col : 0;
  OptVals pv{};
  if (fuse && own) pv = opt_load(gi_idx, fo.prm, fo.m, fo.v);
  // the optimizer scalars while the operand loads are in flight
  if (fuse) fused_opt_prologue(fo, false);
  if (threadIdx.x < 64) {   // <Abar_j, R_j> from the finalize partials, fixed-order butterfly
    double dsum = 0.0;
    for (int b = threadIdx.x; b < dot_nused; b += 64) dsum += dot_part[(size_t)j * dot_nblk + b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dsum += __shfl_xor(dsum, o);
    // |R_j|_F from the rtr partials (proj_n <= 64), the phase kernels' order
    const double nrm = nais_norm_from(threadIdx.x < proj_n ? proj_part[(size_t)j * proj_n + threadIdx.x] : 0.0);
    if (threadIdx.x == 0) {
      dot_s = dsum;
      nrm_s = nrm;
    }
  }
  __syncthreads();
  const double dot = dot_s;
  const double n = nrm_s;
  const bool taken = (float)n > 0.98f;
  const float cA = taken ? (float)(0.98994949366116658 / sqrt(n)) : 1.f;
  const float cR = taken ? (float)(0.98994949366116658 / sqrt(n) * 0.5 * dot / (n * n)) : 0.f;
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int e = threadIdx.x + 256 * u;
    const int k = e >> 4, q = e & 15;
    if (k < L) {
      As[q][k] = wv[u];
      Bs[k][q] = cA * abs_[u] - cR * rs[u];
    }
  }
  __syncthreads();
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc = 0.f;
  for (int k = 0; k < L; ++k) acc += As[ty][k] * Bs[k][tx];
  if (own) {
    grad[gi_idx] = acc;
    if (fuse) opt_apply(fo.a, gi_idx, acc, pv, fo.prm, fo.m, fo.v);
  }
}
#endif

}  // namespace dbsde
