// jet.hip -- dbsde_net_u_jet and dbsde_pde_residual: the forward jet kernels
// (jet.hpp), the direction / contraction kernels of the PDE residual and the
// host code behind the two C ABI entries.
//
// Kernel layout (as xbar.hip): out^T = W . S^T, the weights are the MFMA A
// operand and the state rows the B operand; every operand value is split into
// hi + mid + lo bf16 parts (the state rows in registers, the weights once per
// call by jet_split_kernel) and each 16x16 block accumulates the six
// v_mfma_f32_16x16x32_bf16 products wl.sh + wh.sl + wm.sm + wm.sh + wh.sm
// + wh.sh over a 32-wide k-step, in fp32.  Element j of lane (i, q) is
// k0 + 16 (j >> 2) + 4 q + (j & 3) in both operands, so the accumulator of
// output block o -- lane (i, q) holds units 16 o + 4 q .. + 3 of row i -- is
// exactly what the same lane reads as the next level's operand.
//
// One wave owns NT 16-row tiles (JET_NT = 1) through every level.  Its state (hdot, hddot;
// h in the point pass) lives in a per-lane-private part of LDS: a lane only
// ever reads the elements it wrote, so the levels need no synchronisation,
// and the accumulators of a level (2 NT tw float4) are the only large register
// arrays.  The input rows (v; z = [t, x, 1] in the point pass) are staged once
// per tile with lane-linear loads and serve level 0 and every V_j.  No
// atomics, one fixed summation order: bitwise repeatable.
#include <hip/hip_runtime.h>

#define DBSDE_DEVICE_HELPERS_ONLY
#include "ctx.hpp"
#include "jet.hpp"
#include "sde.hpp"

namespace dbsde {

namespace {

typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

struct Split3 {
  bf16x8 h, m, l;
};

struct JetSplitMat {
  const float* W;   // fp32 row-major [16 tout][ld]
  int ld, K, tout;
  long long off;    // the matrix's first fragment in the image (16-byte units)
};
struct JetSplitArgs {
  JetSplitMat mat[2 * JET_KMAX + 2];
  uintx4* img;
};

__device__ __forceinline__ unsigned hi_pair(float a, float b) {
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
// hi = bf16(x), mid = bf16(x - hi) (round to nearest even), lo = the exact
// remainder (phase.hpp split_two, xbar.hip split8)
__device__ __forceinline__ Split3 split8(floatx4 x0, floatx4 x1) {
  const float x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
  uintx4 H, M, L;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const bf16x2 h = __builtin_convertvector(floatx2{x[2 * d], x[2 * d + 1]}, bf16x2);
    const float r0 = x[2 * d] - (float)h[0], r1 = x[2 * d + 1] - (float)h[1];
    const bf16x2 m = __builtin_convertvector(floatx2{r0, r1}, bf16x2);
    H[d] = __builtin_bit_cast(unsigned, h);
    M[d] = __builtin_bit_cast(unsigned, m);
    L[d] = hi_pair(r0 - (float)m[0], r1 - (float)m[1]);
  }
  return Split3{__builtin_bit_cast(bf16x8, H), __builtin_bit_cast(bf16x8, M), __builtin_bit_cast(bf16x8, L)};
}
__device__ __forceinline__ floatx4 mfma_bf(const bf16x8& a, const bf16x8& b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Orders this wave's LDS accesses (xbar.hip): the staged input rows are
// written by other lanes than the ones that read them.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0), vmcnt / expcnt untouched
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The weights as the jet kernels read them: for every 32-wide k-step ks and
// 16-row output block o of a matrix, the hi / mid / lo bf16 fragments of lane
// (i, q) -- W[16 o + i][32 ks + 16 (j >> 2) + 4 q + (j & 3)], j = 0..7, zero
// past K -- at [(ks tout + o) 3 + part][lane], 16 bytes each.  Split once per
// call here instead of once per row tile in the kernel.
__global__ void __launch_bounds__(256) jet_split_kernel(JetSplitArgs a) {
  const JetSplitMat m = a.mat[blockIdx.y];
  const int nks = (m.K + 31) / 32;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nks * m.tout * 64) return;
  const int lane = idx & 63, i = lane & 15, q = lane >> 4;
  const int blk = idx >> 6, ks = blk / m.tout, o = blk - ks * m.tout;
  const int k0 = 32 * ks;
  const float* w = m.W + (size_t)(16 * o + i) * m.ld + k0 + 4 * q;
  const floatx4 zero4 = floatx4{0.f, 0.f, 0.f, 0.f};
  const Split3 sw = split8(*(const floatx4*)w, k0 + 16 < m.K ? *(const floatx4*)(w + 16) : zero4);
  uintx4* f = a.img + m.off + (size_t)blk * (3 * 64) + lane;
  f[0] = __builtin_bit_cast(uintx4, sw.h);
  f[64] = __builtin_bit_cast(uintx4, sw.m);
  f[128] = __builtin_bit_cast(uintx4, sw.l);
}

// TWMAX: an upper bound of the level widths in 16-blocks (the accumulator
// arrays); NT: row tiles per wave; POINT: the point pass
template <int TWMAX, int NT, bool POINT>
__global__ void __launch_bounds__(64) jet_kernel(JetArgs a) {
  extern __shared__ float lds[];
  constexpr int NS = POINT ? 1 : 2;   // state vectors per row: h, or hdot and hddot
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const int Dp = a.Dp, D = a.D, LDV = Dp + 4, LDW = a.ldw, Stot = a.Stot;
  float* vs = lds;                      // [NT][16][LDV] input rows
  float* hs = lds + NT * 16 * LDV;      // [NT][NS][16][LDW] state rows
  const long long row_base = (long long)blockIdx.x * (16 * NT);
  const floatx4 zero4 = floatx4{0.f, 0.f, 0.f, 0.f};

  // ---- stage the input rows (the tile's valid rows are one contiguous run)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const long long row0 = row_base + 16 * t;
    const long long left = a.nrows - row0;
    const int nr = left >= 16 ? 16 : (left > 0 ? (int)left : 0);
    for (int e = lane; e < 16 * Dp; e += 64) {
      const int r = e / Dp, c = e - r * Dp;
      float v = 0.f;
      if (r < nr) {
        const long long g = row0 + r;
        if constexpr (POINT) {
          if (c == 0) v = a.t[g];
          else if (c <= D) v = a.X[g * D + c - 1];
          else if (c == D + 1) v = 1.f;
        } else {
          if (c <= D) v = a.V[g * (D + 1) + c];
        }
      }
      vs[(t * 16 + r) * LDV + c] = v;
    }
  }
  wave_lds_sync();

  // this lane's rows
  bool valid[NT];
  long long grow[NT], pt[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    grow[t] = row_base + 16 * t + i;
    valid[t] = grow[t] < a.nrows;
    pt[t] = !valid[t] ? 0 : (POINT ? grow[t] : a.p0 + (a.g0 + grow[t]) / a.nd);
  }

  for (int j = 0; j <= a.K; ++j) {
    const int twj = a.tw[j];
    floatx4 acc1[NT][TWMAX], acc2[NT][TWMAX];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int o = 0; o < TWMAX; ++o) acc1[t][o] = acc2[t][o] = zero4;

    // The level's 32-wide k-steps in one sequence: B_j . state_{j-1}, then
    // W_in / V_j . input row (the second derivative has no such term).  The
    // weight fragments of (step, block) n = step tw_j + o (jet_split_kernel:
    // three 16-byte loads) are contiguous in n within each of the two images
    // and are loaded three blocks ahead of their products: nothing else hides
    // the load latency of a wave that is alone on its SIMD.
    const int nB = j > 0 ? (a.tw[j - 1] + 1) / 2 : 0;
    const int nX = (j == 0 || a.has_v) ? (Dp + 31) / 32 : 0;
    const int S = nB + nX, nBt = nB * twj, Nt = S * twj;
    const uintx4* imgB = a.img + a.offB[j] + lane;
    const uintx4* imgX = a.img + a.offX[j] + lane;
    auto ldf = [&](int n) {
      Split3 w{};
      if (n < Nt) {
        const uintx4* f = n < nBt ? imgB + (size_t)n * (3 * 64) : imgX + (size_t)(n - nBt) * (3 * 64);
        w = Split3{__builtin_bit_cast(bf16x8, f[0]), __builtin_bit_cast(bf16x8, f[64]),
                   __builtin_bit_cast(bf16x8, f[128])};
      }
      return w;
    };
    Split3 w0 = ldf(0), w1 = ldf(1), w2 = ldf(2);
    // one step's blocks, product-major over the independent accumulators
    auto blocks = [&](int st, const Split3* s1, const Split3* s2) {
#pragma unroll
      for (int o = 0; o < TWMAX; ++o) {
        if (o < twj) {
          const Split3 w3 = ldf(st * twj + o + 3);
#define JET_PROD(WP, SP)                                                        \
  _Pragma("unroll") for (int t = 0; t < NT; ++t) {                              \
    acc1[t][o] = mfma_bf(w0.WP, s1[t].SP, acc1[t][o]);                          \
    if (s2) acc2[t][o] = mfma_bf(w0.WP, s2[t].SP, acc2[t][o]);                  \
  }
          JET_PROD(l, h)
          JET_PROD(h, l)
          JET_PROD(m, m)
          JET_PROD(m, h)
          JET_PROD(h, m)
          JET_PROD(h, h)
#undef JET_PROD
          w0 = w1;
          w1 = w2;
          w2 = w3;
        }
      }
    };
    for (int st = 0; st < S; ++st) {
      if (st < nB) {
        const int Kin = 16 * a.tw[j - 1], k0 = 32 * st;
        const bool second = k0 + 16 < Kin;
        Split3 s1[NT], s2[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float* h1 = hs + ((t * NS) * 16 + i) * LDW + k0 + 4 * q;
          s1[t] = split8(*(const floatx4*)h1, second ? *(const floatx4*)(h1 + 16) : zero4);
          if constexpr (!POINT) {
            const float* h2 = h1 + 16 * LDW;
            s2[t] = split8(*(const floatx4*)h2, second ? *(const floatx4*)(h2 + 16) : zero4);
          }
        }
        blocks(st, s1, POINT ? nullptr : s2);
      } else {
        const int k0 = 32 * (st - nB);
        const bool second = k0 + 16 < Dp;
        Split3 s1[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float* v1 = vs + (t * 16 + i) * LDV + k0 + 4 * q;
          s1[t] = split8(*(const floatx4*)v1, second ? *(const floatx4*)(v1 + 16) : zero4);
        }
        blocks(st, s1, nullptr);
      }
    }

    // ---- the level's epilogue: the new state of this lane's elements
    const float rho = j > 0 ? a.rho : 0.f;
    const float* bias = (POINT && j > 0 && !a.has_v) ? a.beta[j] : nullptr;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int o = 0; o < TWMAX; ++o) {
        if (o < twj) {
          float* hp = hs + ((t * NS) * 16 + i) * LDW + 16 * o + 4 * q;
          const size_t pofs = (size_t)pt[t] * Stot + a.col[j] + 16 * o + 4 * q;
          if constexpr (POINT) {
            floatx4 p = acc1[t][o];
            if (bias) p += *(const floatx4*)(bias + 16 * o + 4 * q);
            const floatx4 old = rho != 0.f ? *(const floatx4*)hp : zero4;
            floatx4 h, e1, e2;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float d1, d2;
              act_d12(a.act, p[e], d1, d2);
              h[e] = act_f(a.act, p[e]) + rho * old[e];
              e1[e] = d1;
              e2[e] = d2;
            }
            *(floatx4*)hp = h;
            if (valid[t]) {
              *(floatx4*)(a.A1 + pofs) = e1;
              *(floatx4*)(a.A2 + pofs) = e2;
            }
          } else {
            const floatx4 e1 = valid[t] ? *(const floatx4*)(a.A1 + pofs) : zero4;
            const floatx4 e2 = valid[t] ? *(const floatx4*)(a.A2 + pofs) : zero4;
            const floatx4 o1 = rho != 0.f ? *(const floatx4*)hp : zero4;
            const floatx4 o2 = rho != 0.f ? *(const floatx4*)(hp + 16 * LDW) : zero4;
            const floatx4 pd = acc1[t][o], pdd = acc2[t][o];
            *(floatx4*)hp = e1 * pd + rho * o1;
            *(floatx4*)(hp + 16 * LDW) = e2 * pd * pd + e1 * pdd + rho * o2;
          }
        }
      }
  }

  // ---- w_out . state_K: the lane's units in order, then the four lanes of a row
  const int twK = a.tw[a.K];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float s1 = 0.f, s2 = 0.f;
    for (int o = 0; o < twK; ++o) {
      const floatx4 w = *(const floatx4*)(a.wout + 16 * o + 4 * q);
      const float* hp = hs + ((t * NS) * 16 + i) * LDW + 16 * o + 4 * q;
      const floatx4 h1 = *(const floatx4*)hp;
#pragma unroll
      for (int e = 0; e < 4; ++e) s1 = fmaf(w[e], h1[e], s1);
      if constexpr (!POINT) {
        const floatx4 h2 = *(const floatx4*)(hp + 16 * LDW);
#pragma unroll
        for (int e = 0; e < 4; ++e) s2 = fmaf(w[e], h2[e], s2);
      }
    }
    s1 += __shfl_xor(s1, 16);
    s1 += __shfl_xor(s1, 32);
    s2 += __shfl_xor(s2, 16);
    s2 += __shfl_xor(s2, 32);
    if (q == 0 && valid[t]) {
      if constexpr (POINT) {
        // the rows dbsde_net_u clamps: u = max(net, 0), gradient passed at 0 (rowdot_kernel)
        if (a.umask) a.umask[grow[t]] = (s1 + a.bout[0]) >= 0.f ? 1.f : 0.f;
      } else {
        const bool on = !a.umask || a.umask[pt[t]] != 0.f;
        if (a.d1) a.d1[grow[t]] = on ? s1 : 0.f;
        if (a.d2) a.d2[grow[t]] = on ? s2 : 0.f;
      }
    }
  }
}

// row tiles per wave.  Measured at 65,536 jet rows of the 4 x 110 network
// (D = 100): two tiles 233 us (358 registers, 44.5 KB LDS: three waves per
// CU), one tile 160 us (232 registers, 22 KB: seven waves per CU, two per SIMD,
// one wave's operand splits and loads behind the other's products): 1
constexpr int JET_NT = 1;

template <int TWMAX>
int launch_tw(const JetArgs& a, int point, hipStream_t s) {
  const unsigned grid = (unsigned)((a.nrows + 16 * JET_NT - 1) / (16 * JET_NT));
  const size_t lds = (size_t)JET_NT * 16 * ((a.Dp + 4) + (point ? 1 : 2) * a.ldw) * sizeof(float);
  // wide contexts stage more than the default 64 KB (Dp = 1024, width 256:
  // 97 KB); a CU has 160 KB
  if (lds > 160 * 1024) return -2;
  if (lds > 64 * 1024) {
    const void* f = point ? (const void*)jet_kernel<TWMAX, JET_NT, true> : (const void*)jet_kernel<TWMAX, JET_NT, false>;
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -2;
  }
  if (point)
    jet_kernel<TWMAX, JET_NT, true><<<grid, 64, lds, s>>>(a);
  else
    jet_kernel<TWMAX, JET_NT, false><<<grid, 64, lds, s>>>(a);
  return 0;
}

// ---------------------------------------------------------------------------
// PDE residual: the directions of a chunk of points, and the contraction
// ---------------------------------------------------------------------------
struct PdeArgs {
  dbsde_problem pr;
  int heston, D, nb, nd;   // heston: 0 DIAG, 1 HESTON, 2 HESTON2
  float rhob;              // HESTON2: fp32(sqrt(1 - (double)h_rho^2))
  // (DBSDE_PROB_BARRIER has heston = asian = 0: DIAG's drift and diffusion columns.  The generators of the stopped
  // and the unstopped process agree on the live side of the barrier; the residual means nothing beyond it.)
  int asian;               // 1 DBSDE_PROB_ASIAN: state [A, S_1..S_nb] (heston = 0); 2 DBSDE_PROB_GEO_ASIAN: [G, S]
  float T;                 // its averaging horizon
  int gcols;               // leading state columns entering g (pr.pen != 0: the penalty's g)
  const float* Lt;      // [nb][nb] L^T (dbsde_set_corr) or null
  const float* X;
  long long r0;          // the chunk's first point
  int np;                // points of the chunk
  float* V;              // [np, nd, D + 1]
  const float* d1;       // [np, nd]
  const float* d2;
  const float* u;        // [R]
  const float* Du;       // [R, D]
  dbsde_pde_terms out;
};

// direction 0 = e_t; direction 1 + j = column j of the diffusion matrix:
// DIAG diag(sig_a X + sig_b) . L; Heston Sigma_j . (1, 1)^T in the (S_j, v_j)
// plane with the rollout's own coefficients (heston_coef, sde.hpp),
// and with a factor L between the assets column j of Sigma(x) . L: for every
// asset i >= j the (S_i, v_i) entries of Sigma_i . (1, 1)^T times L[i][j];
// two-factor Heston (nd = 1 + 2k) the 2k columns of its diffusion matrix;
// arithmetic average (state [A, S_1..S_k], nd = 1 + k) DIAG's columns over the
// S columns with A component 0; geometric average (state [G, S_1..S_k]) the
// same with G component 0
__global__ void __launch_bounds__(256) pde_dirs_kernel(PdeArgs a) {
  const int ld = a.D + 1;
  const long long n = (long long)a.np * a.nd * ld;
  const long long idx = blockIdx.x * 256LL + threadIdx.x;
  if (idx >= n) return;
  const long long row = idx / ld;
  const int c = (int)(idx - row * ld);
  const long long r = row / a.nd;
  const int j = (int)(row - r * a.nd);
  const float* x = a.X + (size_t)(a.r0 + r) * a.D;
  float v = 0.f;
  if (j == 0) {
    v = c == 0 ? 1.f : 0.f;
  } else if (c > 0) {
    const int jb = j - 1, d = c - 1;
    if (a.heston == 2) {
      // two-factor Heston, k = D / 2: direction 1 + i is the dW^S_i column
      // (S_i: d00, v_i: d10), direction 1 + k + i the dW^v_i column (v_i: d11)
      const int k = a.D >> 1;
      const int i = d < k ? d : d - k;   // the asset of column d
      if (i == (jb < k ? jb : jb - k) && (jb < k || d >= k)) {
        const Heston2Coef h = heston2_coef(a.pr.mu_a, a.pr.h_kappa, a.pr.h_theta, a.pr.h_sigma, a.pr.h_rho, a.rhob,
                                           x[i], x[k + i]);
        v = jb >= k ? h.d11 : (d < k ? h.d00 : h.d10);
      }
    } else if (a.heston) {
      const int k = a.nb;
      const int i = d < k ? d : d - k;   // the asset of column d
      if (a.Lt ? i >= jb : i == jb) {
        const HestonCoef h = heston_coef(a.pr.mu_a, a.pr.h_kappa, a.pr.h_theta, a.pr.h_sigma, a.pr.h_rho, x[i], x[k + i]);
        v = d < k ? h.d00 + h.d01 : h.d10 + h.d11;
        if (a.Lt) v *= a.Lt[(size_t)jb * k + i];   // L[i][jb]
      }
    } else if (a.asian) {
      // [A, S_1..S_k]: direction 1 + j is column j of diag(sig_a S + sig_b) . L in the S columns, 0 in A
      const int i = d - 1;
      if (i >= 0) {
        const float l = a.Lt ? (jb <= i ? a.Lt[(size_t)jb * a.nb + i] : 0.f) : (i == jb ? 1.f : 0.f);
        v = (a.pr.sig_a * x[d] + a.pr.sig_b) * l;
      }
    } else {
      const float l = a.Lt ? (jb <= d ? a.Lt[(size_t)jb * a.nb + d] : 0.f) : (d == jb ? 1.f : 0.f);
      v = (a.pr.sig_a * x[d] + a.pr.sig_b) * l;
    }
  }
  a.V[idx] = v;
}

// one wave per point: lane l takes the indices l, l + 64, ... of every sum, the
// lanes are added by a fixed xor butterfly
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__global__ void __launch_bounds__(256) pde_terms_kernel(PdeArgs a) {
  const int lane = threadIdx.x & 63;
  const long long r = blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (r >= a.np) return;
  const long long p = a.r0 + r;
  const int D = a.D;
  const float* x = a.X + (size_t)p * D;
  const float* du = a.Du + (size_t)p * D;
  float drift = 0.f, xz = 0.f, zz = 0.f;
  // pr.pen != 0 (DIAG only): g of the point's own x for the penalty term, its
  // sums taken on this walk of the row
  float s_x = 0.f, s_xx = 0.f;
  if (a.pr.pen != 0.f) {
    for (int d = lane; d < a.gcols; d += 64) {
      s_x += x[d];
      s_xx += x[d] * x[d];
    }
    s_x = wave_sum(s_x);
    s_xx = wave_sum(s_xx);
  }
  const int k = a.heston == 2 ? D >> 1 : a.nb;   // assets of a Heston state
  for (int d = lane; d < D; d += 64) {
    const float xd = x[d], zd = du[d];
    float mu;
    if (a.heston)
      mu = d < k ? heston_mu_s(a.pr.mu_a, xd) : heston_mu_v(a.pr.h_kappa, a.pr.h_theta, xd);
    else
      mu = a.pr.mu_a * xd;
    drift += mu * zd;
    xz += xd * zd;
    zz += zd * zd;
  }
  if (a.asian) {
    // [A, S_1..S_k]: mu_a S_i on the S columns and mean S / T on A;
    // [G, S_1..S_k]: G mean log S / T on G
    float ss = 0.f;
    drift = 0.f;
    for (int d = 1 + lane; d < D; d += 64) {
      ss += a.asian == 2 ? logf(x[d]) : x[d];
      drift += a.pr.mu_a * x[d] * du[d];
    }
    ss = wave_sum(ss);
    if (lane == 0) drift += (a.asian == 2 ? x[0] : 1.f) * (ss / (float)a.nb / a.T) * du[0];
  }
  float tr = 0.f, atr = 0.f;
  for (int j = 1 + lane; j < a.nd; j += 64) {
    const float v = a.d2[r * a.nd + j];
    tr += v;
    atr += fabsf(v);
  }
  drift = wave_sum(drift);
  xz = wave_sum(xz);
  zz = wave_sum(zz);
  tr = wave_sum(tr);
  atr = wave_sum(atr);
  if (lane != 0) return;
  const float u = a.u[p];
  const float ut = a.d1[r * a.nd];
  const float diff = 0.5f * tr;
  float phi = a.pr.phi_r * (u - a.pr.phi_c * xz) + a.pr.phi_zz * zz;
  if (a.pr.pen != 0.f) {   // the penalised PDE's driver (kernels.hpp penalty_phi)
    float gsign, gs, dy;
    const int gk = terminal_kind(a.pr.g_kind, gsign);
    phi += penalty_phi(a.pr.pen, terminal_g(gk, s_x, s_xx, a.gcols, a.pr.strike, a.pr.g_alpha, gsign, gs), u, dy);
  }
  if (a.out.u) a.out.u[p] = u;
  if (a.out.u_t) a.out.u_t[p] = ut;
  if (a.out.drift) a.out.drift[p] = drift;
  if (a.out.diffusion) a.out.diffusion[p] = diff;
  if (a.out.phi) a.out.phi[p] = phi;
  if (a.out.residual) a.out.residual[p] = ut + drift + diff - phi;
  if (a.out.scale) a.out.scale[p] = fabsf(ut) + fabsf(drift) + 0.5f * atr + fabsf(phi);
}

}  // namespace

// fills a.offX / a.offB and returns the image size in 16-byte units
long long jet_image_layout(JetArgs& a) {
  long long off = 0;
  const int nks_x = (a.Dp + 31) / 32;
  for (int j = 0; j <= a.K; ++j) {
    if (j == 0 || a.has_v) {
      a.offX[j] = off;
      off += (long long)nks_x * a.tw[j] * 3 * 64;
    }
    if (j > 0) {
      a.offB[j] = off;
      off += (long long)((16 * a.tw[j - 1] + 31) / 32) * a.tw[j] * 3 * 64;
    }
  }
  return off;
}

int jet_split_launch(const JetArgs& a, hipStream_t s) {
  JetSplitArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.img = (uintx4*)a.img;
  int n = 0, blocks = 1;
  auto add = [&](const float* W, int ld, int K, int tout, long long off) {
    sa.mat[n++] = JetSplitMat{W, ld, K, tout, off};
    blocks = std::max(blocks, ((K + 31) / 32 * tout * 64 + 255) / 256);
  };
  for (int j = 0; j <= a.K; ++j) {
    if (j == 0 || a.has_v) add(a.Wx + (size_t)a.col[j] * a.Dp, a.Dp, a.Dp, a.tw[j], a.offX[j]);
    if (j > 0) add(a.Bf[j], 16 * a.tw[j - 1], 16 * a.tw[j - 1], a.tw[j], a.offB[j]);
  }
  jet_split_kernel<<<dim3(blocks, n), 256, 0, s>>>(sa);
  return 0;
}

int jet_launch(const JetArgs& a, int point, hipStream_t s) {
  if (a.nrows < 1 || a.K < 1 || a.K > JET_KMAX || a.Dp % 16 != 0 || a.D + 2 > a.Dp || a.Stot % 4 != 0 ||
      a.ldw != 16 * a.twmax + 4 || (!point && a.nd < 1))
    return -1;
  for (int j = 0; j <= a.K; ++j)
    if (a.tw[j] < 1 || a.tw[j] > a.twmax) return -1;
  if (a.twmax <= 1) return launch_tw<1>(a, point, s);
  if (a.twmax <= 2) return launch_tw<2>(a, point, s);
  if (a.twmax <= 4) return launch_tw<4>(a, point, s);
  if (a.twmax <= 7) return launch_tw<7>(a, point, s);
  if (a.twmax <= 8) return launch_tw<8>(a, point, s);
  if (a.twmax <= 16) return launch_tw<16>(a, point, s);
  return -1;
}

}  // namespace dbsde

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

// jet rows per launch and per direction workspace (DBSDE_JET_CAP at context creation)
constexpr long long JET_CAP_DEFAULT = 65536;

long long jet_cap(dbsde_ctx* c) { return c->jet_cap > 0 ? c->jet_cap : JET_CAP_DEFAULT; }

JetArgs jet_args(dbsde_ctx* c) {
  JetArgs a;
  memset(&a, 0, sizeof(a));
  a.Wx = c->BtIn;
  a.twmax = 0;
  for (int j = 0; j <= c->K; ++j) {
    a.tw[j] = c->Wp[j] / 16;
    a.col[j] = c->col[j];
    a.twmax = std::max(a.twmax, a.tw[j]);
    if (j > 0) {
      a.Bf[j] = c->Bf[j];
      a.beta[j] = c->has_v ? nullptr : c->beta[j];
    }
  }
  a.ldw = 16 * a.twmax + 4;
  a.wout = c->wout;
  a.bout = c->bout;
  a.K = c->K;
  a.D = c->D;
  a.Dp = c->Dp;
  a.Stot = c->Stot;
  a.has_v = c->has_v ? 1 : 0;
  a.act = c->act;
  a.rho = c->rho;
  a.A1 = c->Abuf;
  a.A2 = c->Adot;
  a.umask = c->u_clamp ? c->umask : nullptr;
  jet_image_layout(a);
  a.img = (const uintx4*)c->jet_img;
  return a;
}

template <typename T>
int grow(dbsde_ctx* c, T** p, size_t& cap, size_t n) {
  if (n <= cap) return DBSDE_OK;
  if (*p) {
    HIPC(c, hipStreamSynchronize(c->stream));
    (void)hipFree(*p);
    c->allocs.erase(std::find(c->allocs.begin(), c->allocs.end(), (void*)*p));
    *p = nullptr;
    cap = 0;
  }
  const int rc = dalloc_t(c, p, n);
  if (!rc) cap = n;
  return rc;
}

double jet_flops_row(dbsde_ctx* c, int nvec) {
  double fl = 0.0;
  for (int j = 1; j <= c->K; ++j) fl += 2.0 * nvec * c->L[j] * (double)c->L[j + 1];
  for (int j = 0; j <= (c->has_v ? c->K : 0); ++j) fl += 2.0 * (c->D + 1) * (double)c->L[j + 1];
  return fl + 2.0 * nvec * c->L[c->K + 1];
}
double jet_weight_bytes(dbsde_ctx* c) {
  double by = 0.0;
  for (int j = 1; j <= c->K; ++j) by += 4.0 * c->Wp[j] * (double)c->Wp[j - 1];
  return by + 4.0 * c->Stot_x * (double)c->Dp;
}

// weights (full: the whole prep; else the fp32 copies alone) and the point
// pass: act'(p_j), act''(p_j) of every point into Abuf / Adot, the clamp mask
int jet_points(dbsde_ctx* c, const float* params, int R, const float* t, const float* X, bool full) {
  int rc;
  if ((rc = jet_pack_weights(c, params, full))) return rc;
  hipStream_t s = c->stream;
  {
    JetArgs l = jet_args(c);
    const size_t need = (size_t)jet_image_layout(l) * 4;   // 16-byte units -> unsigned
    if ((rc = grow(c, &c->jet_img, c->jet_img_cap, need))) return rc;
  }
  JetArgs a = jet_args(c);
  a.nrows = R;
  a.t = t;
  a.X = X;
  RUN(c, s, "jet_split_weights", 0.0, 2.5 * jet_weight_bytes(c), jet_split_launch(a, s));
  int ok = 0;
  RUN(c, s, "jet_points", (double)R * jet_flops_row(c, 1),
      4.0 * R * (c->D + 1.0 + 2.0 * c->Stot) + jet_weight_bytes(c), ok = jet_launch(a, 1, s));
  if (ok == -2) return fail(c, DBSDE_EINVAL, "net_u_jet: the input and state rows exceed the CU's 160 KB of LDS");
  if (ok) return fail(c, DBSDE_EINVAL, "net_u_jet: hidden widths above 256 are not supported");
  return DBSDE_OK;
}

// jet rows [0, n) of V (row g belongs to point p0 + (g0 + g) / nd)
int jet_rows(dbsde_ctx* c, long long n, long long g0, long long p0, int nd, const float* V, float* d1, float* d2) {
  hipStream_t s = c->stream;
  JetArgs a = jet_args(c);
  a.nrows = n;
  a.g0 = g0;
  a.p0 = p0;
  a.nd = nd;
  a.V = V;
  a.d1 = d1;
  a.d2 = d2;
  int ok = 0;
  RUN(c, s, "net_u_jet", (double)n * jet_flops_row(c, 2),
      4.0 * n * (c->D + 3.0) + jet_weight_bytes(c), ok = jet_launch(a, 0, s));
  if (ok == -2) return fail(c, DBSDE_EINVAL, "net_u_jet: the input and state rows exceed the CU's 160 KB of LDS");
  if (ok) return fail(c, DBSDE_EINVAL, "net_u_jet: hidden widths above 256 are not supported");
  return DBSDE_OK;
}

// the context's row buffers for R points.  A held-back prefetch is issued as
// dbsde_net_u issues it (flush_deferred); the jet kernels read and write no
// path buffer, so no buffer is selected and pending rollouts stay pending.
int jet_begin(dbsde_ctx* c, int R) {
  HIPC(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_rows(c, pad_rows(R), 1))) return rc;
  return flush_deferred(c);
}

}  // namespace

extern "C" {

int dbsde_net_u_jet(dbsde_ctx* c, const float* params, int R, const float* t, const float* X, int nd,
                    const float* V, float* d1, float* d2) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (!params || !t || !X || !V || R < 1 || nd < 1 || (!d1 && !d2))
    return fail(c, DBSDE_EINVAL, "bad net_u_jet arguments");
  int rc;
  if ((rc = jet_begin(c, R))) return rc;
  if ((rc = jet_points(c, params, R, t, X, true))) return rc;
  const long long total = (long long)R * nd, cap = jet_cap(c);
  const int ld = c->D + 1;
  for (long long g0 = 0; g0 < total; g0 += cap) {
    const long long n = std::min(cap, total - g0);
    if ((rc = jet_rows(c, n, g0, 0, nd, V + (size_t)g0 * ld, d1 ? d1 + g0 : nullptr, d2 ? d2 + g0 : nullptr)))
      return rc;
  }
  return DBSDE_OK;
}

int dbsde_pde_residual(dbsde_ctx* c, const float* params, int R, const float* t, const float* X,
                       const dbsde_pde_terms* out) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (!params || !t || !X || R < 1 || !out) return fail(c, DBSDE_EINVAL, "bad pde_residual arguments");
  if (!out->u && !out->u_t && !out->drift && !out->diffusion && !out->phi && !out->residual && !out->scale)
    return fail(c, DBSDE_EINVAL, "pde_residual: no output requested");
  HIPC(c, hipSetDevice(c->device));
  const int D = c->D, nd = 1 + c->nb;
  int rc;
  // u and Du from the existing forward
  if ((rc = grow(c, &c->jet_u, c->jet_u_cap, (size_t)R))) return rc;
  if ((rc = grow(c, &c->jet_du, c->jet_du_cap, (size_t)R * D))) return rc;
  if ((rc = dbsde_net_u(c, params, R, t, X, c->jet_u, c->jet_du))) return rc;
  if ((rc = jet_begin(c, R))) return rc;
  if ((rc = jet_points(c, params, R, t, X, false))) return rc;   // dbsde_net_u ran the prep
  // chunks of whole points, at most jet_cap jet rows each
  const long long pc = std::max<long long>(1, jet_cap(c) / nd);
  const long long np_max = std::min<long long>(pc, R);
  if ((rc = grow(c, &c->jet_V, c->jet_V_cap, (size_t)np_max * nd * (D + 1)))) return rc;
  if ((rc = grow(c, &c->jet_d, c->jet_d_cap, (size_t)np_max * nd * 2))) return rc;
  hipStream_t s = c->stream;
  for (long long r0 = 0; r0 < R; r0 += pc) {
    const int np = (int)std::min<long long>(pc, R - r0);
    const long long rows = (long long)np * nd;
    PdeArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.pr = c->cfg.problem;
    pa.heston = c->heston2 ? 2 : (c->heston ? 1 : 0);
    pa.rhob = c->rhob;
    pa.asian = c->geo ? 2 : (c->asian ? 1 : 0);
    pa.T = c->cfg.T;
    pa.gcols = c->gcols;
    pa.D = D;
    pa.nb = c->nb;
    pa.nd = nd;
    pa.Lt = c->Lt;
    pa.X = X;
    pa.r0 = r0;
    pa.np = np;
    pa.V = c->jet_V;
    pa.d1 = c->jet_d;
    pa.d2 = c->jet_d + np_max * nd;
    pa.u = c->jet_u;
    pa.Du = c->jet_du;
    pa.out = *out;
    const long long nv = rows * (D + 1);
    RUN(c, s, "pde_dirs", 0.0, 4.0 * nv, pde_dirs_kernel<<<(unsigned)((nv + 255) / 256), 256, 0, s>>>(pa));
    if ((rc = jet_rows(c, rows, 0, r0, nd, c->jet_V, c->jet_d, c->jet_d + np_max * nd))) return rc;
    RUN(c, s, "pde_terms", (double)np * (6.0 * D + 3.0 * nd), 4.0 * np * (2.0 * D + 2.0 * nd + 8.0),
        pde_terms_kernel<<<(unsigned)((np + 3) / 4), 256, 0, s>>>(pa));
  }
  return DBSDE_OK;
}

}  // extern "C"
