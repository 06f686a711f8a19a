// vec.hip -- the C ABI of the flat-vector operations behind the L-BFGS
// optimizer (vec.hpp): reductions, axpby, the two-loop direction.
#include <hip/hip_runtime.h>

#define DBSDE_DEVICE_HELPERS_ONLY
#include "ctx.hpp"
#include "vec.hpp"

extern "C" {

int dbsde_vec_reduce(dbsde_ctx* c, int op, const float* a, const float* b, long long n, double* result) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (op < DBSDE_VEC_DOT || op > DBSDE_VEC_AMAX || !a || (op == DBSDE_VEC_DOT && !b) || n < 1 || !result)
    return fail(c, DBSDE_EINVAL, "bad dbsde_vec_reduce arguments");
  HIPC(c, hipSetDevice(c->device));
  int rc;
  if (!c->vec_part && (rc = dalloc_t(c, &c->vec_part, VEC_RED_BLOCKS + 1))) return rc;
  hipStream_t s = c->stream;
  RUN(c, c->stream, "vec_reduce", 2.0 * n, 8.0 * n, vec_reduce_kernel<<<VEC_RED_BLOCKS, 256, 0, s>>>(op, a, b, n, c->vec_part));
  RUN(c, c->stream, "vec_reduce", 0.0, 0.0,
      vec_reduce_final_kernel<<<1, 256, 0, s>>>(op, c->vec_part, VEC_RED_BLOCKS, c->vec_part + VEC_RED_BLOCKS));
  HIPC(c, hipMemcpyAsync(result, c->vec_part + VEC_RED_BLOCKS, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPC(c, hipStreamSynchronize(s));
  return DBSDE_OK;
}

int dbsde_vec_axpby(dbsde_ctx* c, float* z, const float* x, const float* y, long long n, float alpha, float beta) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (!z || !x || n < 1 || (!y && beta != 0.f)) return fail(c, DBSDE_EINVAL, "bad dbsde_vec_axpby arguments");
  HIPC(c, hipSetDevice(c->device));
  const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 1024);
  RUN(c, c->stream, "vec_axpby", 3.0 * n, 12.0 * n, vec_axpby_kernel<<<blocks, 256, 0, c->stream>>>(z, x, y, n, alpha, beta));
  return DBSDE_OK;
}

int dbsde_lbfgs_direction(dbsde_ctx* c, const float* g, const float* S, const float* Y, long long ld, long long n,
                          const int* slot, const float* ro, int num, float h_diag, float* d) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (!g || !d || n < 1 || num < 0 || num > LBFGS_HMAX || (num > 0 && (!S || !Y || !slot || !ro || ld < n)))
    return fail(c, DBSDE_EINVAL, "bad dbsde_lbfgs_direction arguments (at most 128 history entries)");
  HIPC(c, hipSetDevice(c->device));
  LbfgsArgs a{};
  a.g = g;
  a.S = S;
  a.Y = Y;
  a.ld = ld;
  a.n = n;
  a.d = d;
  a.num = num;
  a.h_diag = h_diag;
  for (int i = 0; i < num; ++i) {
    if (slot[i] < 0) return fail(c, DBSDE_EINVAL, "negative history slot");
    a.slot[i] = slot[i];
    a.ro[i] = ro[i];
  }
  RUN(c, c->stream, "lbfgs_direction", 8.0 * n * num, 16.0 * n * num, lbfgs_direction_kernel<<<1, 1024, 0, c->stream>>>(a));
  return DBSDE_OK;
}

}  // extern "C"
