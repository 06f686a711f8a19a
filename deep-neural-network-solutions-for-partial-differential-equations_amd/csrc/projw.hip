// projw.hip -- the NAIS projection products at hidden widths above 128
// (projw.hpp), fp32-input MFMA (v_mfma_f32_16x16x4_f32: an exact k-ordered
// fp32 FMA chain per output element, the form the chain GEMMs use).
//
// Both products run as 64 x 64 output tiles per 256-thread workgroup: four
// waves of 32 x 32, so a wave holds four independent accumulators (the
// 16x16x4 form has a longer dependent latency than its issue interval).  K is
// staged through LDS in chunks of 32, register staged and double buffered.
// L need not be a multiple of anything: operand loads are scalar and guarded
// (rows of W_j at L = 129 are not 16-byte aligned), rows and columns >= L
// contribute zeros and are not stored.
//
//   rtr_wide_kernel   R_j = W_j^T W_j.  Both operands are column strips of the
//                     row-major W_j, so every load runs along a row.  Only the
//                     tiles ti <= tj are computed and each is written to
//                     (ti, tj) and (tj, ti): R_j is exactly symmetric.  (Inside
//                     a diagonal tile (r, c) and (c, r) are the same products
//                     in the same order.)  Per-tile fp64 sum of squares, an
//                     off-diagonal tile counted twice.
//   reduce_kernel     part[j, :] -> sq[j], dot_part[j, :] -> dot[j]: thread t
//                     sums elements t, t + 256, ..., then a fixed tree over
//                     the 256 threads.
//   sform_kernel      S_j = cA (Abar_j + Abar_j^T) - cR (R_j + R_j^T), the
//                     transposed Abar tile through LDS.  S_j is symmetric.
//   wbar_wide_kernel  grad W_j = W_j S_j from the snapshot.
#include "projw.hpp"

namespace dbsde {

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ floatx4 mfma4(float a, float b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

constexpr int PW_KC = 32;    // K rows per LDS stage
constexpr int PW_LS = 80;    // row stride of a [k][64] stage (the four k of an MFMA step 16 banks apart)
constexpr int PW_LSA = 36;   // row stride of a [64][k] stage (16 rows x 4 k on distinct banks)

// the 32-deep MFMA step of one wave's 32 x 32 quadrant: a(m, k), b(k, n)
template <typename FA, typename FB>
__device__ __forceinline__ void quad_step(floatx4 (&acc)[2][2], FA&& a_at, FB&& b_at) {
#pragma unroll
  for (int i = 0; i < PW_KC / 4; ++i) {
    float a[2], b[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      a[s] = a_at(s, i);
      b[s] = b_at(s, i);
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) acc[x][y] = mfma4(a[x], b[y], acc[x][y]);
  }
}

__global__ void __launch_bounds__(256) rtr_wide_kernel(ProjWideArgs p) {
  __shared__ float As[2][PW_KC * PW_LS];   // As[k][m] = W[k][64 ti + m]
  __shared__ float Bs[2][PW_KC * PW_LS];   // Bs[k][n] = W[k][64 tj + n]
  __shared__ double red[256];
  const int L = p.L, j = blockIdx.y;
  const int nt = (L + PW_TILE - 1) / PW_TILE;
  // triangle index -> (ti, tj), ti <= tj
  int t = blockIdx.x, ti = 0;
  while (t >= nt - ti) {
    t -= nt - ti;
    ++ti;
  }
  const int tj = ti + t;
  const float* W = p.params + p.woffs[j];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int q = lane >> 4, l16 = lane & 15;

  // the snapshot of W_j the adjoint reads: this workgroup's share
  {
    float* snap = p.wsnap[j];
    const int total = L * L, step = gridDim.x * 256;
    for (int e = blockIdx.x * 256 + tid; e < total; e += step) snap[e] = W[e];
  }

  const bool active = (ti * PW_TILE + wm * 32 < L) && (tj * PW_TILE + wn * 32 < L);
  floatx4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int lc = tid & 63, lr = tid >> 6;
  const int ca = ti * PW_TILE + lc, cb = tj * PW_TILE + lc;
  float ar[PW_KC / 4], br[PW_KC / 4];
  auto gload = [&](int kc) {
#pragma unroll
    for (int u = 0; u < PW_KC / 4; ++u) {
      const int k = kc * PW_KC + lr + 4 * u;
      const bool in = k < L;
      ar[u] = (in && ca < L) ? W[(size_t)k * L + ca] : 0.f;
      br[u] = (in && cb < L) ? W[(size_t)k * L + cb] : 0.f;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int u = 0; u < PW_KC / 4; ++u) {
      As[buf][(lr + 4 * u) * PW_LS + lc] = ar[u];
      Bs[buf][(lr + 4 * u) * PW_LS + lc] = br[u];
    }
  };
  const int nk = (L + PW_KC - 1) / PW_KC;
  gload(0);
  sstore(0);
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nk) gload(kc + 1);
    if (active)
      quad_step(
          acc, [&](int s, int i) { return As[buf][(4 * i + q) * PW_LS + wm * 32 + s * 16 + l16]; },
          [&](int s, int i) { return Bs[buf][(4 * i + q) * PW_LS + wn * 32 + s * 16 + l16]; });
    if (kc + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }

  float* R = p.rtr[j];
  const bool offdiag = ti != tj;
  double sq = 0.0;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = ti * PW_TILE + wm * 32 + x * 16 + q * 4 + e;
        const int n = tj * PW_TILE + wn * 32 + y * 16 + l16;
        if (m < L && n < L) {
          const float v = acc[x][y][e];
          R[(size_t)m * L + n] = v;
          if (offdiag) R[(size_t)n * L + m] = v;
          sq += (double)v * (double)v;
        }
      }
  if (offdiag) sq *= 2.0;
  red[tid] = sq;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) p.part[(size_t)j * p.npart + blockIdx.x] = red[0];
}

// out[j] = sum of in[j * stride + 0 .. n), fixed order
__global__ void __launch_bounds__(256) reduce_kernel(const double* in, int stride, int n, double* out) {
  __shared__ double red[256];
  const double* src = in + (size_t)blockIdx.x * stride;
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += src[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// S_j, 32 x 32 elements per workgroup; the factors exactly as
// proj_backward_kernel forms them
__global__ void __launch_bounds__(256) sform_kernel(ProjWideArgs p) {
  __shared__ float Tt[32][33];   // Tt[a][b] = Abar[32 bx + a][32 by + b]
  const int L = p.L, j = blockIdx.z;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float* Ab = p.abar[j];
  const float* R = p.rtr[j];
  float* S = p.sbuf[j];
  const double n = sqrt(p.sq[j]), dot = p.dot[j];   // |R_j|_F as pack_block forms it
  const bool taken = (float)n > 0.98f;
  const float cA = taken ? (float)(0.98994949366116658 / sqrt(n)) : 1.f;
  const float cR = taken ? (float)(0.98994949366116658 / sqrt(n) * 0.5 * dot / (n * n)) : 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int a = ty + 8 * u;
    const int r = 32 * bx + a, c = 32 * by + tx;
    Tt[a][tx] = (r < L && c < L) ? Ab[(size_t)r * L + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int b = ty + 8 * u;
    const int r = 32 * by + b, c = 32 * bx + tx;   // S[r][c]; Abar[c][r] = Tt[tx][b]
    if (r < L && c < L) {
      const float ab = Ab[(size_t)r * L + c] + Tt[tx][b];
      const float rv = R[(size_t)r * L + c];   // R_j is exactly symmetric: R + R^T = rv + rv
      S[(size_t)r * L + c] = cA * ab - cR * (rv + rv);
    }
  }
}

__global__ void __launch_bounds__(256) wbar_wide_kernel(ProjWideArgs p) {
  __shared__ float As[2][PW_TILE * PW_LSA];   // As[m][k] = W[64 tm + m][k]
  __shared__ float Bs[2][PW_KC * PW_LS];      // Bs[k][n] = S[k][64 tn + n]
  const int L = p.L, j = blockIdx.y;
  const int nt = (L + PW_TILE - 1) / PW_TILE;
  const int tm = blockIdx.x / nt, tn = blockIdx.x - tm * nt;
  const float* W = p.wsnap[j];
  const float* S = p.sbuf[j];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int q = lane >> 4, l16 = lane & 15;
  const bool active = (tm * PW_TILE + wm * 32 < L) && (tn * PW_TILE + wn * 32 < L);
  floatx4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int ak = tid & 31, am = tid >> 5;    // A loader: k in the chunk, first row
  const int bc = tid & 63, bk = tid >> 6;    // B loader: column, first k
  const int cb = tn * PW_TILE + bc;
  float ar[PW_TILE / 8], br[PW_KC / 4];
  auto gload = [&](int kc) {
    const int ka = kc * PW_KC + ak;
#pragma unroll
    for (int u = 0; u < PW_TILE / 8; ++u) {
      const int m = tm * PW_TILE + am + 8 * u;
      ar[u] = (m < L && ka < L) ? W[(size_t)m * L + ka] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < PW_KC / 4; ++u) {
      const int k = kc * PW_KC + bk + 4 * u;
      br[u] = (k < L && cb < L) ? S[(size_t)k * L + cb] : 0.f;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int u = 0; u < PW_TILE / 8; ++u) As[buf][(am + 8 * u) * PW_LSA + ak] = ar[u];
#pragma unroll
    for (int u = 0; u < PW_KC / 4; ++u) Bs[buf][(bk + 4 * u) * PW_LS + bc] = br[u];
  };
  const int nk = (L + PW_KC - 1) / PW_KC;
  gload(0);
  sstore(0);
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nk) gload(kc + 1);
    if (active)
      quad_step(
          acc, [&](int s, int i) { return As[buf][(wm * 32 + s * 16 + l16) * PW_LSA + 4 * i + q]; },
          [&](int s, int i) { return Bs[buf][(4 * i + q) * PW_LS + wn * 32 + s * 16 + l16]; });
    if (kc + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }
  float* G = p.grad + p.woffs[j];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = tm * PW_TILE + wm * 32 + x * 16 + q * 4 + e;
        const int n = tn * PW_TILE + wn * 32 + y * 16 + l16;
        if (m < L && n < L) G[(size_t)m * L + n] = acc[x][y][e];
      }
}

bool geometry_ok(const ProjWideArgs& a) {
  return a.L > 0 && a.L <= NAIS_WIDE_LMAX && a.K >= 1 && a.npart == projw_tri_tiles(a.L);
}

}  // namespace

int projw_forward_launch(const ProjWideArgs& a, hipStream_t s) {
  if (!geometry_ok(a)) return -1;
  rtr_wide_kernel<<<dim3(a.npart, a.K), 256, 0, s>>>(a);
  reduce_kernel<<<a.K, 256, 0, s>>>(a.part, a.npart, a.npart, a.sq);
  return 0;
}

int projw_backward_launch(const ProjWideArgs& a, hipStream_t s) {
  if (!geometry_ok(a) || a.dot_nused > a.dot_nblk) return -1;
  const int nt = (a.L + PW_TILE - 1) / PW_TILE, n32 = (a.L + 31) / 32;
  reduce_kernel<<<a.K, 256, 0, s>>>(a.dot_part, a.dot_nblk, a.dot_nused, a.dot);
  sform_kernel<<<dim3(n32, n32, a.K), 256, 0, s>>>(a);
  wbar_wide_kernel<<<dim3(nt * nt, a.K), 256, 0, s>>>(a);
  return 0;
}

}  // namespace dbsde
