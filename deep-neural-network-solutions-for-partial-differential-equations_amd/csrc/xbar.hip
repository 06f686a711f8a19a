// xbar.hip -- the input cotangent of net_u, xbar = (Alpha . W)[:, 1..D]
// (xbar.hpp), in split-bf16 products for every network form.
//
// Orientation (as the phase kernels): out^T = W^T . Alpha^T, the weights are
// the MFMA A operand and the cotangent rows the B operand, so lane (i, q) of a
// 16-row tile ends with columns 16 o + 4 q .. + 3 of row i.  Each operand
// value is split into hi + mid + lo bf16 parts in registers (phase.hpp
// split_two) and every 16x16 block accumulates the six
// v_mfma_f32_16x16x32_bf16 products wl.ah + wh.al + wm.am + wm.ah + wh.am +
// wh.ah over a 32-wide k-step; the dropped products stay within 2^-24 of each
// product (tools/ubench/x3_acc.hip).  The same kernel serves the contexts
// whose phase kernels run the fp32-input MFMA form.
//
// k order of a step: element j of lane (i, q) is k0 + 16 (j >> 2) + 4 q + (j & 3)
// in both operands -- two 16-byte loads per lane from the row-major operands,
// and a K that is an odd multiple of 16 zero-fills the whole second load.
//
// One wave owns NT 16-row tiles and all Dp / 16 output blocks, so a weight
// block is loaded and split once per NT tiles; the four waves of a workgroup
// run in step over neighbouring rows and share the weight reads through the
// cache.  No atomics, one fixed summation order: bitwise repeatable.
// (Dp > 128: the output blocks in passes of 8, netu_xbar_wide_kernel below.)
//
// Output: the tile's valid rows of the dense [R, D] result are one contiguous
// run of floats; the tile goes through a wave-private LDS strip so that run is
// written with lane-linear dword stores.  Column 0 (the t cotangent) and the
// padding columns are dropped there (as export_kernel drops them for Z); rows
// past R are neither loaded nor stored.
#include "xbar.hpp"

namespace dbsde {

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

struct Split3 {
  bf16x8 h, m, l;
};

__device__ __forceinline__ unsigned hi_pair(float a, float b) {
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
// hi = bf16(x), mid = bf16(x - hi) (round to nearest even), lo = the exact
// remainder (phase.hpp split_two)
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

constexpr int XB_WAVES = 4;
// row tiles per wave.  Measured at R = 52,224, K = 448, Dp = 112: 1 tile 115 us,
// 2 tiles 83 us, 4 tiles 80 us (at 252 registers, one wave per SIMD): 2
constexpr int XB_NT = 2;

// Orders this wave's LDS accesses: its earlier ones are complete (lgkmcnt(0))
// and the compiler moves none across.  The strip below is wave-private, so no
// workgroup barrier is needed (the four waves stay uncoupled).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0), vmcnt / expcnt untouched
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// TD = Dp / 16 output blocks, NT row tiles per wave
template <int TD, int NT>
__global__ void __launch_bounds__(64 * XB_WAVES) netu_xbar_kernel(XbarArgs a) {
  constexpr int LDL = 16 * TD + 4;   // strip row stride (16-byte aligned rows)
  __shared__ float strip[XB_WAVES][16 * LDL];
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long row_base = ((long long)blockIdx.x * XB_WAVES + wave) * (16 * NT);
  const int K = a.K;
  const floatx4 zero4 = floatx4{0.f, 0.f, 0.f, 0.f};

  floatx4 acc[NT][TD];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int o = 0; o < TD; ++o) acc[t][o] = zero4;

  // this lane's operand rows: cotangent row row_base + 16 t + i (valid below
  // R), weight row (= output column) 16 o + i
  const float* ap[NT];
  bool av[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const long long row = row_base + 16 * t + i;
    av[t] = row < a.R;
    ap[t] = a.Alpha + (size_t)(av[t] ? row : 0) * a.lda + 4 * q;
  }
  const float* wp = a.Wt + (size_t)i * K + 4 * q;

  floatx4 ra[NT][2];
  auto load_alpha = [&](int k0) {
    const bool second = k0 + 16 < K;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      ra[t][0] = av[t] ? *(const floatx4*)(ap[t] + k0) : zero4;
      ra[t][1] = (av[t] && second) ? *(const floatx4*)(ap[t] + k0 + 16) : zero4;
    }
  };
  load_alpha(0);
  for (int k0 = 0; k0 < K; k0 += 32) {
    const bool second = k0 + 16 < K;
    Split3 sa[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) sa[t] = split8(ra[t][0], ra[t][1]);
    if (k0 + 32 < K) load_alpha(k0 + 32);   // the next step's rows, a step ahead
#pragma unroll
    for (int o = 0; o < TD; ++o) {
      const float* w = wp + (size_t)(16 * o) * K + k0;
      const floatx4 w0 = *(const floatx4*)w;
      const floatx4 w1 = second ? *(const floatx4*)(w + 16) : zero4;
      const Split3 sw = split8(w0, w1);
      // product-major over the row tiles: consecutive MFMAs are independent
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.l, sa[t].h, acc[t][o]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.h, sa[t].l, acc[t][o]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.m, sa[t].m, acc[t][o]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.m, sa[t].h, acc[t][o]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.h, sa[t].m, acc[t][o]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.h, sa[t].h, acc[t][o]);
    }
  }

  // ---- epilogue: tile -> strip -> the tile's contiguous run of xbar
  float* st = strip[wave];
  const int D = a.D;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t > 0) wave_lds_sync();   // the strip's previous tile has been read
#pragma unroll
    for (int o = 0; o < TD; ++o) *(floatx4*)(st + i * LDL + 16 * o + 4 * q) = acc[t][o];
    wave_lds_sync();
    const long long row0 = row_base + 16 * t;
    const long long left = (long long)a.R - row0;
    const int nrows = left >= 16 ? 16 : (left > 0 ? (int)left : 0);
    float* out = a.xbar + (size_t)(nrows > 0 ? row0 : 0) * D;
    const int n = nrows * D;
    for (int e = lane; e < n; e += 64) {
      const int r = e / D, c = e - r * D + 1;
      out[e] = st[r * LDL + c];
    }
  }
}

// Wide contexts (Dp > 128): the Dp / 16 output blocks in passes of XW_TD = 8,
// pass = blockIdx.y, so a wave holds at most 8 blocks per row tile and the strip
// stays 16 x (128 + 4) floats.  A pass is the kernel above restricted to its
// blocks (the last pass may hold fewer: a wave-uniform guard): the same
// products in the same k order per output element, so bitwise repeatable.  The
// strip's 128 columns map to xbar columns 128 pass + lc - 1; each row's share
// is one contiguous run, stored lane-linear.
constexpr int XW_TD = 8;
template <int NT>
__global__ void __launch_bounds__(64 * XB_WAVES) netu_xbar_wide_kernel(XbarArgs a) {
  constexpr int TD = XW_TD, LDL = 16 * TD + 4;
  __shared__ float strip[XB_WAVES][16 * LDL];
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long row_base = ((long long)blockIdx.x * XB_WAVES + wave) * (16 * NT);
  const int K = a.K;
  const int ob0 = blockIdx.y * TD;
  const int nbp = min(TD, a.Dp / 16 - ob0);   // this pass's blocks
  const floatx4 zero4 = floatx4{0.f, 0.f, 0.f, 0.f};

  floatx4 acc[NT][TD];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int o = 0; o < TD; ++o) acc[t][o] = zero4;

  const float* ap[NT];
  bool av[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const long long row = row_base + 16 * t + i;
    av[t] = row < a.R;
    ap[t] = a.Alpha + (size_t)(av[t] ? row : 0) * a.lda + 4 * q;
  }
  const float* wp = a.Wt + (size_t)(16 * ob0 + i) * K + 4 * q;

  floatx4 ra[NT][2];
  auto load_alpha = [&](int k0) {
    const bool second = k0 + 16 < K;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      ra[t][0] = av[t] ? *(const floatx4*)(ap[t] + k0) : zero4;
      ra[t][1] = (av[t] && second) ? *(const floatx4*)(ap[t] + k0 + 16) : zero4;
    }
  };
  load_alpha(0);
  for (int k0 = 0; k0 < K; k0 += 32) {
    const bool second = k0 + 16 < K;
    Split3 sa[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) sa[t] = split8(ra[t][0], ra[t][1]);
    if (k0 + 32 < K) load_alpha(k0 + 32);
#pragma unroll
    for (int o = 0; o < TD; ++o) {
      if (o < nbp) {
        const float* w = wp + (size_t)(16 * o) * K + k0;
        const floatx4 w0 = *(const floatx4*)w;
        const floatx4 w1 = second ? *(const floatx4*)(w + 16) : zero4;
        const Split3 sw = split8(w0, w1);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.l, sa[t].h, acc[t][o]);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.h, sa[t].l, acc[t][o]);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.m, sa[t].m, acc[t][o]);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.m, sa[t].h, acc[t][o]);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.h, sa[t].m, acc[t][o]);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t][o] = mfma_bf(sw.h, sa[t].h, acc[t][o]);
      }
    }
  }

  float* st = strip[wave];
  const int D = a.D;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t > 0) wave_lds_sync();
#pragma unroll
    for (int o = 0; o < TD; ++o) *(floatx4*)(st + i * LDL + 16 * o + 4 * q) = acc[t][o];
    wave_lds_sync();
    const long long row0 = row_base + 16 * t;
    const long long left = (long long)a.R - row0;
    const int nrows = left >= 16 ? 16 : (left > 0 ? (int)left : 0);
    for (int e = lane; e < nrows * (16 * TD); e += 64) {
      const int r = e / (16 * TD), lc = e - r * (16 * TD);
      const int col = 16 * ob0 + lc;   // row-buffer column: 0 = t, 1..D = X
      if (col >= 1 && col <= D) a.xbar[(size_t)(row0 + r) * D + col - 1] = st[r * LDL + lc];
    }
  }
}

template <int TD>
int launch_td(const XbarArgs& a, hipStream_t s) {
  constexpr int ROWS = 16 * XB_NT * XB_WAVES;
  const unsigned grid = (unsigned)(((long long)a.R + ROWS - 1) / ROWS);
  netu_xbar_kernel<TD, XB_NT><<<grid, 64 * XB_WAVES, 0, s>>>(a);
  return 0;
}

}  // namespace

int netu_xbar_launch(const XbarArgs& a, hipStream_t s) {
  if (a.R < 1 || a.K < 16 || a.K % 16 != 0 || a.Dp % 16 != 0 || a.D < 1 || a.D + 1 > a.Dp || a.lda < a.K ||
      a.lda % 4 != 0)
    return -1;
  switch (a.Dp / 16) {
    case 1: return launch_td<1>(a, s);
    case 2: return launch_td<2>(a, s);
    case 3: return launch_td<3>(a, s);
    case 4: return launch_td<4>(a, s);
    case 5: return launch_td<5>(a, s);
    case 6: return launch_td<6>(a, s);
    case 7: return launch_td<7>(a, s);
    case 8: return launch_td<8>(a, s);
    default: break;
  }
  if (a.Dp > 1024) return -1;
  constexpr int ROWS = 16 * XB_NT * XB_WAVES;
  const dim3 grid((unsigned)(((long long)a.R + ROWS - 1) / ROWS), (unsigned)((a.Dp / 16 + XW_TD - 1) / XW_TD));
  netu_xbar_wide_kernel<XB_NT><<<grid, 64 * XB_WAVES, 0, s>>>(a);
  return 0;
}

}  // namespace dbsde
