// step.hip -- the launch sequence of the deep-BSDE step and of net_u, and the
// optimizer update, exported through the C ABI of include/dbsde.h.
//
// One dbsde_loss_grad call = FBSNN.loss_function + loss.backward of the
// reference (DeepBSDE.py:202-245, 279) restated time-parallel:
//   prep      NAIS projection A_j (Q4), weight packing       (once per call)
//   rollout   Euler-Maruyama X path, sigma*dW (rollout.hip)   (HBM-bound)
//   forward   x-stack GEMM + K block GEMMs, u                 (MFMA fp32)
//   input-grad K block GEMMs + Z GEMM with the residual epilogue
//   tangent   forward-mode along zbar                         (MFMA fp32)
//   reverse   K block GEMMs                                   (MFMA fp32)
//   weight-grad split-K TN GEMMs into slabs, fixed-order slab sums, NAIS adjoint
// State dimensions above 126 (Dp > 128) run this per-layer sequence with the Z
// GEMM over column tiles (zgemm_wide) and the residual epilogue as a row kernel
// behind it (fused.hpp zrow_cotan_kernel); DESIGN 3.6.  NAIS hidden widths
// above 128 run it too, with the projection and its adjoint on the
// matrix-core kernels of projw.hip.
//
// This unit instantiates the kernels of kernels.hpp, fused.hpp, phase.hpp,
// chainx3.hpp and tnx3.hpp.
#include <hip/hip_runtime.h>

// minimum rows per weight-gradient row split of the chain layouts: 448 keeps
// HJB's 43,008 rows at the 96-split capacity (1.222-1.232 ms/step against
// 1.244-1.250 with 84 splits) and gives config 1's 13,056 rows 30 splits
// (0.457-0.465 against 0.483-0.494 ms with 96: a third of the finalize reads),
// profiles/r4_ab_tn_splits.txt
#ifndef DBSDE_TN_SPLIT_ROWS
#define DBSDE_TN_SPLIT_ROWS 448
#endif
#include "ctx.hpp"
#include "xbar.hpp"
#include "chainx3.hpp"
#include "tnx3.hpp"
#include "tnw.hpp"

// ---------------------------------------------------------------------------
// fused phase-kernel instantiations (FusedVariant, ctx.hpp)
// HV: the network has the NAIS x-stack (V_j); a template flag, so each kernel
// carries only its own code path (smaller straight-line kernels).  X3: the
// split-bf16 matrix-core form (phase.hpp), at width 110/112; the fp32-input
// MFMA form stays selectable (DBSDE_X3=0) and serves width 16.  phase2.hpp:
// the width-112 networks with two tiles per wave (DBSDE_NT=2; DBSDE_ADOT=1 the
// adot-in-memory phase C) and config 4's FC width 256.
#define FV(T, TD, K, ACT, HV, X3)                                                                      \
  {T, TD, K, ACT, HV, X3, P3_ROWS, 0, (X3) && (HV), phaseA_kernel<T, TD, K, ACT, HV, X3>, \
   phaseC_kernel<T, TD, K, ACT, HV, X3>}
#define FV2(T, TD, K, ACT, X3) FV(T, TD, K, ACT, true, X3), FV(T, TD, K, ACT, false, X3)
#define FQ(T, TD, K, ACT, HV, NT, NBUF, ADOT)                                                              \
  {T, TD, K, ACT, HV, 1, 64 * NT, ADOT, (HV) && !(ADOT), phaseA2_kernel<T, TD, K, ACT, HV, NT, NBUF, ADOT>, \
   phaseC2_kernel<T, TD, K, ACT, HV, NT, NBUF, ADOT>},
// column-split kernels (phasecs.hpp): 16 rows per workgroup, the small-M form
#define FCS(T, TD, K, ACT, HV) \
  {T, TD, K, ACT, HV, 1, CS_ROWS, 0, (HV), phaseAcs_kernel<T, TD, K, ACT, HV>, phaseCcs_kernel<T, TD, K, ACT, HV>},
const FusedVariant kFused[] = {
    DBSDE_PHASE2_INSTANCES(FQ)
    DBSDE_PHASECS_INSTANCES(FCS)
    FV2(7, 7, 3, 0, 1), FV2(7, 7, 3, 1, 1), FV2(7, 7, 3, 2, 1), FV2(7, 7, 3, 0, 0), FV2(7, 7, 3, 1, 0),
    FV2(7, 7, 3, 2, 0), FV2(1, 1, 1, 0, 0), FV2(1, 1, 1, 1, 0), FV2(1, 1, 1, 2, 0), FV2(1, 1, 2, 0, 0),
    FV2(1, 1, 2, 1, 0), FV2(1, 1, 2, 2, 0), FV2(1, 1, 3, 0, 0), FV2(1, 1, 3, 1, 0), FV2(1, 1, 3, 2, 0),
    // SiLU (3) and Softplus (4): the instances tanh has
    FV2(7, 7, 3, 3, 1), FV2(7, 7, 3, 4, 1), FV2(7, 7, 3, 3, 0), FV2(7, 7, 3, 4, 0), FV2(1, 1, 1, 3, 0),
    FV2(1, 1, 1, 4, 0), FV2(1, 1, 2, 3, 0), FV2(1, 1, 2, 4, 0), FV2(1, 1, 3, 3, 0), FV2(1, 1, 3, 4, 0),
};
#undef FQ
#undef FCS
#undef FV2
#undef FV
constexpr int kNumFused = (int)(sizeof(kFused) / sizeof(kFused[0]));
static_assert(kNumFused <= 96, "dbsde_ctx::fv_slots");
const FusedVariant& fused_at(int fv) { return kFused[fv]; }
// the variant for a network (each (T, TD, K, act, hv, x3) has at most one
// 64-row and one column-split instance)
// (DBSDE_W256=0 leaves the width-256 FC networks to the per-layer chain)
// (cs: the column-split variant, which the launch picks for small batches)
int fused_variant(int T, int TD, int K, int act, bool hv, bool x3, bool cs) {
  const char* ew = getenv("DBSDE_W256");
  const bool wide = !(ew && ew[0] == '0');
  for (int i = 0; i < kNumFused; ++i)
    if ((wide || kFused[i].T <= 8) && kFused[i].T == T && kFused[i].TD == TD && kFused[i].K == K &&
        kFused[i].act == act && kFused[i].hv == hv && kFused[i].x3 == (int)x3 && (kFused[i].rows == CS_ROWS) == cs)
      return i;
  return -1;
}

int fill_col0(dbsde_ctx* c, float* buf, int ld, long long rows, float v) {
  fill_col0_kernel<<<(unsigned)((rows + 255) / 256), 256, 0, c->stream>>>(buf, ld, rows, v);
  HIPC(c, hipGetLastError());
  return DBSDE_OK;
}

namespace {

// ---------------------------------------------------------------------------
// chain GEMM dispatch
// ---------------------------------------------------------------------------
template <int EPI>
int chain(dbsde_ctx* c, const char* name, ChainArgs& a, int Rp, int NP, int NT, double flops, double bytes) {
  // (EPI_STORE_N: the last column tile may reach past NP; its weight rows are
  // allocated, zero, and its stores guarded)
  constexpr bool ragged = EPI == EPI_STORE_N;
  if (NT < 1) return fail(c, DBSDE_EINVAL, "internal: bad NT");
  dim3 grid(Rp / CH_BM, (NP + 16 * NT - 1) / (16 * NT));
  if (!ragged && NP % (16 * NT) != 0) return fail(c, DBSDE_EINVAL, "internal: column tiling mismatch");
  if (a.K % CH_KC != 0) return fail(c, DBSDE_EINVAL, "internal: K not a multiple of 16");
  hipStream_t s = c->stream;
  // split-bf16 form (the weight image must hold this launch's output columns);
  // tile widths without an X3 instantiation (e.g. the Z GEMM at Dp = 32) run the
  // fp32 chain on the fp32 weights the packer writes alongside the images
  if (a.x3_img && (NT == 7 || NT == 8)) {
    if (a.x3_tout < NP / 16 || a.x3_ti * 16 < a.K) return fail(c, DBSDE_EINVAL, "internal: x3 chain image geometry");
    switch (NT) {
      case 7:
        RUN(c, s, name, flops, bytes, (chain_gemm_kernel<7, EPI, true><<<grid, 256, 0, s>>>(a)));
        return DBSDE_OK;
      case 8:
        RUN(c, s, name, flops, bytes, (chain_gemm_kernel<8, EPI, true><<<grid, 256, 0, s>>>(a)));
        return DBSDE_OK;
      default:
        return fail(c, DBSDE_EINVAL, "internal: x3 chain tile");
    }
  }
#define CASE_NT(X) \
  case X:          \
    RUN(c, s, name, flops, bytes, chain_gemm_kernel<X, EPI><<<grid, 256, 0, s>>>(a)); \
    break;
  switch (NT) {
    CASE_NT(1)
    CASE_NT(2)
    CASE_NT(3)
    CASE_NT(4)
    CASE_NT(5)
    CASE_NT(6)
    CASE_NT(7)
    CASE_NT(8)
    default:
      return fail(c, DBSDE_EINVAL, "internal: bad NT");
  }
#undef CASE_NT
  return DBSDE_OK;
}

ChainArgs base_args(dbsde_ctx* c) {
  ChainArgs a;
  memset(&a, 0, sizeof(a));
  a.rho = c->rho;
  a.act = c->act;
  return a;
}
// the split-bf16 chain form of a launch: weight image img with tout output /
// ti input 16-blocks (no-op for the fp32 chain)
void x3_weights(dbsde_ctx* c, ChainArgs& a, const float* img, int tout, int ti) {
  if (!c->x3chain) return;
  a.x3_img = (const unsigned short*)img;
  a.x3_tout = tout;
  a.x3_ti = ti;
}

// arguments of the wide projection kernels (projw.hpp)
ProjWideArgs projw_args(dbsde_ctx* c, const float* params, float* grad) {
  ProjWideArgs a{};
  a.params = params;
  a.woffs = c->d_woffs;
  a.L = c->L[1];
  a.K = c->K;
  a.rtr = c->d_rtr;
  a.wsnap = c->d_wsnap;
  a.abar = c->d_abar;
  a.sbuf = c->d_sbuf;
  a.part = c->proj_part;
  a.npart = projw_tri_tiles(a.L);
  a.sq = c->proj_sq;
  a.dot_part = c->dot_part;
  a.dot_nblk = c->dot_nblk;
  a.dot_nused = c->dot_nused;
  a.dot = c->proj_dot;
  a.grad = grad;
  return a;
}

int prep_weights(dbsde_ctx* c, const float* params) {
  hipStream_t s = c->stream;
  const int LW = c->L[1];
  if (c->proj_wide) {
    int ok = 0;
    const ProjWideArgs pa = projw_args(c, params, nullptr);
    RUN(c, s, "rtr_wide", 2.0 * c->K * LW * (double)LW * LW, 0.0, ok = projw_forward_launch(pa, s));
    if (ok) return fail(c, DBSDE_EINVAL, "internal: wide projection geometry");
  } else if (c->proj) {
    const double fl = 2.0 * c->K * LW * (double)LW * LW;
    const int nblk = ((LW + 15) / 16) * ((LW + 15) / 16);
    RUN(c, s, "rtr", fl, 0.0,
        rtr_params_kernel<<<dim3(nblk, c->K), 256, 0, s>>>(params, c->d_woffs, LW, c->d_rtr, c->d_wsnap,
                                                            c->proj_part, nblk));
  }
  RUN(c, s, "pack_weights", 0.0, 0.0, pack_tagged_kernel<<<dim3(c->prep_blocks, c->n_prep), 256, 0, s>>>(c->d_prep, params, nullptr));
  return DBSDE_OK;
}

// Weight-gradient contraction, wave-owned tiles (tnw.hpp).  Problem p = j:
// x-stack level j (alpha_j^T x + delta_j^T zbar); p = K + j: block B_j
// (alpha_j^T h_{j-1} + delta_j^T hdot_{j-1}); plus the output-layer column sums.
// Slices [s0, s0 + sn) (sn < 0: all), on stream st without profiling records
// (st == nullptr: the context stream, profiled).
int launch_tnw(dbsde_ctx* c, int R, int Rp, int s0 = 0, int sn = -1, hipStream_t st = nullptr) {
  const int K = c->K, S = c->Stot, T = c->Dp;
  TNWArgs a;
  memset(&a, 0, sizeof(a));
  for (int j = 0; j <= K; ++j) {
    TNWProb& p = a.prob[j];
    p.A1 = c->Alpha + c->col[j];
    p.lda1 = S;
    p.B1 = c->xin;
    p.ldb1 = c->Dp;
    p.A2 = c->Delta + c->col[j];
    p.lda2 = S;
    p.B2 = c->zbar;
    p.ldb2 = c->Dp;
  }
  for (int j = 1; j <= K; ++j) {
    TNWProb& p = a.prob[K + j];
    p.A1 = c->Alpha + c->col[j];
    p.lda1 = S;
    p.B1 = c->H + c->col[j - 1];
    p.ldb1 = S;
    p.A2 = c->Delta + c->col[j];
    p.lda2 = S;
    p.B2 = c->Hdot + c->col[j - 1];
    p.ldb2 = S;
  }
  a.P = c->tnw_P;
  a.S = c->tnw_S;
  // the four waves of a workgroup (one CU, one slice, in step) share operand
  // rows through the CU's cache: group 0 = {x-stack 0, x-stack 1, block 1,
  // output}, group g = {x-stack 2g, 2g + 1, blocks 2g, 2g + 1} -- x / zbar
  // twice and alpha_j / delta_j of each block with its x-stack level
  for (int g = 0; g < a.P / 4; ++g) {
    int* o = a.order + 4 * g;
    if (g == 0) {
      o[0] = 0; o[1] = 1; o[2] = K + 1; o[3] = a.P - 1;
    } else {
      o[0] = 2 * g; o[1] = 2 * g + 1; o[2] = K + 2 * g; o[3] = K + 2 * g + 1;
    }
  }
  if (const char* e = getenv("DBSDE_TNW_ORDER"))   // A/B: 0 = problems in index order
    if (e[0] == '0')
      for (int q = 0; q < a.P; ++q) a.order[q] = q;
  a.s0 = s0;
  a.sn = sn < 0 ? a.S : sn;
  a.nchunk = Rp / 16;
  a.slab = c->slabW;
  a.ubar = c->ubar;
  a.Hk = c->H + c->col[K];
  a.Hdk = c->Hdot + c->col[K];
  a.ldh = S;
  a.R = R;
  if (Rp % 16 != 0 || c->Wp[K] != T || a.S % 8 != 0 || a.P != 2 * K + 2 || a.P % 4 != 0 || a.sn % 8 != 0 ||
      a.s0 < 0 || a.s0 + a.sn > a.S)
    return fail(c, DBSDE_EINVAL, "internal: tnw geometry");
  const double fl = 2.0 * 2.0 * (double)R * (K + 1) * c->L[1] * (c->D + 2) + 2.0 * 2.0 * (double)R * K * c->L[1] * c->L[1] +
                    4.0 * (double)R * c->L[K + 1];
  if (c->tnw_nb < 1 || c->tnw_nb > 8) return fail(c, DBSDE_EINVAL, "internal: tnw tile");
  if (c->tnw_x3 && Rp % 32 != 0) return fail(c, DBSDE_EINVAL, "internal: tnw x3 geometry");
  int lr = 0;
  auto launch = [&](hipStream_t q) { lr = c->tnw_x3 ? tnw_x3_launch(c->tnw_nb, a, q) : tnw_launch(c->tnw_nb, a, q); };
  if (st) {   // a slice range inside the phase pipeline (loss_grad_impl)
    launch(st);
    HIPC(c, hipGetLastError());
  } else {
    RUN(c, c->stream, "tn_weight_grad", fl, 0.0, launch(c->stream));
  }
  if (lr) return fail(c, DBSDE_EINVAL, "internal: tnw launch geometry");
  return DBSDE_OK;
}

int finalize_grads(dbsde_ctx* c, const float* params, float* grad, const double* loss_part, int nloss, float* loss,
                   const FusedOpt* fo) {
  hipStream_t s = c->stream;
  FusedOpt fz{};
  const FusedOpt& f = fo ? *fo : fz;
  const int fuse = fo ? 1 : 0;
  if (fo && !c->tnw) return fail(c, DBSDE_EINVAL, "internal: fused update needs the tile finalize");
  if (c->tnw) {
    const int T = c->Dp;
    RUN(c, s, fuse ? "grad_finalize_update" : "grad_finalize", 0.0, 0.0,
        tilefin_kernel<<<dim3((T * T + TF_ELEMS - 1) / TF_ELEMS, c->tnw_P + 1), 256, 0, s>>>(
            c->d_fintab, c->slabW, c->tnw_S, c->tnw_P, T, grad, loss_part, nloss, loss, f, fuse));
  } else {
    RUN(c, s, "grad_finalize", 0.0, 0.0,
        slabsum_kernel<<<dim3(c->fin_blocks, c->n_fin), 256, 0, s>>>(c->d_fin, grad, c->tn_splits_cur, loss_part,
                                                                      nloss, loss));
  }
  if (c->proj_wide) {
    if (fuse) return fail(c, DBSDE_EINVAL, "internal: fused update at a wide projection");
    const int LW = c->L[1];
    int ok = 0;
    const ProjWideArgs pa = projw_args(c, params, grad);
    RUN(c, s, "proj_backward_wide", 2.0 * c->K * LW * (double)LW * LW, 0.0, ok = projw_backward_launch(pa, s));
    if (ok) return fail(c, DBSDE_EINVAL, "internal: wide projection geometry");
  } else if (c->proj) {
    const int LW = c->L[1];
    const int ntile = ((LW + 15) / 16) * ((LW + 15) / 16);
    RUN(c, s, "proj_backward", 2.0 * c->K * LW * (double)LW * LW, 0.0,
        proj_backward_kernel<<<dim3(ntile, c->K), 256, 0, s>>>(c->d_wsnap, c->d_woffs, c->d_abar, c->d_rtr, LW,
                                                               c->proj_part, ntile, c->dot_part, c->dot_nblk,
                                                               c->dot_nused, grad, f, fuse));
  }
  return DBSDE_OK;
}

// output columns of the x-stack GEMM: the input layer's and, for NAIS, every V_j's
int nv_x(dbsde_ctx* c) {
  int nv = 0;
  for (int j = 0; j <= (c->has_v ? c->K : 0); ++j) nv += c->L[j + 1];
  return nv;
}

// forward + input gradient for rows already in xin; leaves u, Abuf, H, Delta, G.
int forward_and_inputgrad(dbsde_ctx* c, int R, int Rp) {
  hipStream_t s = c->stream;
  const int K = c->K, S = c->Stot, D = c->D;
  const auto& L = c->L;
  // x-stack GEMM (a_0 and, for NAIS, the x V_j^T + beta_j parts of every level)
  {
    ChainArgs a = base_args(c);
    a.A = c->xin;
    a.lda = c->Dp;
    a.Bt = c->BtIn;
    x3_weights(c, a, c->imgX[0], c->Wp[0] / 16, c->Dp / 16);
    a.ldb = c->Dp;
    a.K = c->Dp;
    a.out[0] = c->Abuf;
    a.ldo[0] = S;
    a.out[1] = c->H;
    a.ldo[1] = S;
    a.lvl0_cols = c->Wp[0];
    const int nv = nv_x(c);
    const double fl = 2.0 * R * (D + 1) * nv;
    int rc = chain<EPI_FWD0>(c, "gemm_xstack_fwd", a, Rp, c->Stot_x, nt_for(c->Wp[0]), fl,
                             4.0 * R * ((D + 1) + nv + L[1]));
    if (rc) return rc;
  }
  for (int j = 1; j <= K; ++j) {
    ChainArgs a = base_args(c);
    a.A = c->H + c->col[j - 1];
    a.lda = S;
    a.Bt = c->Bf[j];
    x3_weights(c, a, c->imgF[j], c->Wp[j] / 16, c->Wp[j - 1] / 16);
    a.ldb = c->Wp[j - 1];
    a.K = c->Wp[j - 1];
    a.in[0] = c->has_v ? c->Abuf + c->col[j] : nullptr;
    a.ldi[0] = S;
    a.vec[0] = c->beta[j];
    a.in[1] = c->H + c->col[j - 1];
    a.ldi[1] = S;
    a.out[0] = c->Abuf + c->col[j];
    a.ldo[0] = S;
    a.out[1] = c->H + c->col[j];
    a.ldo[1] = S;
    a.last = j == K;
    a.out[2] = c->Delta + c->col[K];
    a.ldo[2] = S;
    a.vec[1] = c->wout;
    const double fl = 2.0 * R * L[j] * L[j + 1];
    int rc = chain<EPI_FWD>(c, "gemm_block_fwd", a, Rp, c->Wp[j], nt_for(c->Wp[j]), fl,
                            4.0 * R * (L[j] + 4.0 * L[j + 1]));
    if (rc) return rc;
  }
  RUN(c, s, "rowdot_u", 2.0 * R * L[K + 1], 4.0 * R * L[K + 1],
      rowdot_kernel<<<Rp / 16, 256, 0, c->stream>>>(c->H + c->col[K], S, c->Wp[K], c->wout, c->bout, c->u, Rp,
                                                   c->u_clamp ? c->umask : nullptr));
  for (int j = K; j >= 1; --j) {
    ChainArgs a = base_args(c);
    a.A = c->Delta + c->col[j];
    a.lda = S;
    a.Bt = c->Bb[j];
    x3_weights(c, a, c->imgB[j], c->Wp[j - 1] / 16, c->Wp[j] / 16);
    a.ldb = c->Wp[j];
    a.K = c->Wp[j];
    a.in[0] = j == K ? nullptr : c->G + c->col[j];
    a.ldi[0] = S;
    a.vec[0] = c->wout;
    a.in[1] = c->Abuf + c->col[j - 1];
    a.ldi[1] = S;
    a.out[0] = c->G + c->col[j - 1];
    a.ldo[0] = S;
    a.out[1] = c->Delta + c->col[j - 1];
    a.ldo[1] = S;
    const double fl = 2.0 * R * L[j] * L[j + 1];
    int rc = chain<EPI_BWD>(c, "gemm_block_inputgrad", a, Rp, c->Wp[j - 1], nt_for(c->Wp[j - 1]), fl,
                            4.0 * R * (L[j + 1] + 4.0 * L[j]));
    if (rc) return rc;
  }
  return DBSDE_OK;
}

int zgemm_args(dbsde_ctx* c, ChainArgs& a) {
  a.A = c->Delta;
  a.lda = c->Stot;
  a.Bt = c->BtZ;
  x3_weights(c, a, c->imgZ[0], c->Dp / 16, c->Wp[0] / 16);
  a.ldb = c->Stot_x;
  a.K = c->Stot_x;
  a.out[0] = c->zfull;
  a.ldo[0] = c->Dp;
  return DBSDE_OK;
}

double zgemm_flops(dbsde_ctx* c, int R) { return 2.0 * R * nv_x(c) * c->D; }

// Column tiling of the wide Z GEMM (Dp > 128): ceil(Dp / 128) column tiles of
// NT <= 8 blocks each, NT the smallest that covers Dp (9 blocks: 2 tiles of 5,
// 13: 2 of 7, 19: 3 of 7, 64: 8 of 8).  BtZ holds ZG_PAD spare zero rows for
// the ragged last tile (build_buffers).
int zgemm_wide_nt(int Dp) {
  const int nblk = Dp / 16, tiles = (nblk + 7) / 8;
  return (nblk + tiles - 1) / tiles;
}
// Z = Delta . W_in of a wide context into zfull, plain stores
int zgemm_wide(dbsde_ctx* c, const char* name, int R, int Rp) {
  ChainArgs a = base_args(c);
  zgemm_args(c, a);
  a.lvl0_cols = c->Dp;
  const int NT = zgemm_wide_nt(c->Dp);
  if (((c->Dp / 16 + NT - 1) / NT) * NT * 16 > c->Dp + ZG_PAD) return fail(c, DBSDE_EINVAL, "internal: wide Z tiling");
  return chain<EPI_STORE_N>(c, name, a, Rp, c->Dp, NT, zgemm_flops(c, R), 4.0 * R * (c->Stot_x + (double)c->D));
}

CotanParams cotan_params(dbsde_ctx* c, int R, int Rp, int N1, bool q3) {
  const dbsde_problem& pr = c->cfg.problem;
  CotanParams p{};
  p.R = R;
  p.Rp = Rp;
  p.N1 = N1;
  p.D = c->D;
  p.Dp = c->Dp;
  p.gcols = c->gcols;
  p.xin = c->xin;
  p.sdw = c->sdw;
  p.zfull = c->zfull;
  p.u = c->u;
  p.rowsum = c->rowsum;
  p.q3S = q3 ? c->q3S : nullptr;
  p.phi_r = pr.phi_r;
  p.phi_c = pr.phi_c;
  p.phi_zz = pr.phi_zz;
  p.strike = pr.strike;
  p.g_alpha = pr.g_alpha;
  p.g_kind = terminal_kind(pr.g_kind, p.gsign);
  p.pen = pr.pen;
  return p;
}

FusedArgs fused_args(dbsde_ctx* c, int R, int Rp, int N1, bool q3) {
  FusedArgs a;
  memset(&a, 0, sizeof(a));
  a.R = R;
  a.N1 = N1;
  a.D = c->D;
  a.gcols = c->gcols;
  a.u_clamp = c->u_clamp;
  a.Dp = c->Dp;
  a.W = c->Wp[0];
  a.S = c->Stot;
  a.has_v = c->has_v;
  a.act = c->act;
  a.rho = c->rho;
  a.xin = c->xin;
  for (int j = 1; j <= c->K; ++j) a.beta[j - 1] = c->beta[j];
  a.wout = c->wout;
  a.bout = c->bout;
  a.Abuf = c->Abuf;
  a.H = c->H;
  a.G = c->G;
  a.Delta = c->Delta;
  a.u = c->u;
  a.zfull = c->zfull;
  a.rowsum = c->rowsum;
  a.sdw = c->sdw;
  a.cp = cotan_params(c, R, Rp, N1, q3);
  a.zbar = c->zbar;
  a.ubar = c->ubar;
  a.u16 = c->tnw ? nullptr : c->u16;
  a.loss_part = c->loss_part;
  a.Hdot = c->Hdot;
  a.Alpha = c->Alpha;
  a.Adot = c->Adot;

  // stage sequences (phase.hpp): every image streamed as two pieces, input
  // blocks [0, H) and [H, TI)
  const int TW = c->Wp[0] / 16, TDp = c->Dp / 16, K = c->K;
  auto add = [&](const float** imgs, int* nfs, int& n, const float* img, int TO, int TI) {
    if (c->x3) {   // one piece per 32-wide input block: TO fragments of 3 chunks
      for (int kb = 0; kb < (TI + 1) / 2; ++kb) {
        imgs[n] = img + (size_t)kb * TO * 768;
        nfs[n++] = 3 * TO;
      }
      return;
    }
    if (TI < 2) {
      imgs[n] = img;
      nfs[n++] = TO * TI;
      return;
    }
    const int H = (TI + 1) / 2;
    imgs[n] = img;
    nfs[n++] = H * TO;
    imgs[n] = img + (size_t)H * TO * 256;
    nfs[n++] = (TI - H) * TO;
  };
  auto addA = [&](const float* img, int TO, int TI) { add(a.simgA, a.snfA, a.nA, img, TO, TI); };
  auto addC = [&](const float* img, int TO, int TI) { add(a.simgC, a.snfC, a.nC, img, TO, TI); };
  addA(c->imgX[0], TW, TDp);
  addC(c->imgX[0], TW, TDp);
  const bool xfirst = c->fv >= 0 && kFused[c->fv].xfirst;   // phase C's X-first stage order (phase.hpp)
  if (xfirst)
    for (int j = 1; j <= K; ++j) addC(c->imgX[j], TW, TDp);
  for (int j = 1; j <= K; ++j) {
    addA(c->imgF[j], TW, TW);
    addC(c->imgF[j], TW, TW);
    if (c->has_v) {
      addA(c->imgX[j], TW, TDp);
      if (!xfirst) addC(c->imgX[j], TW, TDp);
    }
  }
  for (int j = K; j >= 1; --j) {
    if (c->has_v) addA(c->imgZ[j], TDp, TW);
    addA(c->imgB[j], TW, TW);
    addC(c->imgB[j], TW, TW);
  }
  addA(c->imgZ[0], TDp, TW);
  return a;
}

// the split-bf16 phase kernels (T == TD) hold their piece counts at compile
// time (phase.hpp PieceStager NP) and the piece pointers in one VGPR's lanes
bool fused_piece_counts_ok(dbsde_ctx* c, const FusedArgs& a) {
  const int TW = c->Wp[0] / 16, TDp = c->Dp / 16, K = c->K, hv = c->has_v ? 1 : 0;
  if (!c->x3 || TW != TDp) return a.nA <= 64 && a.nC <= 64;
  const int nkb = (TW + 1) / 2;
  return a.nA == nkb * (2 + 2 * K * (1 + hv)) && a.nC == nkb * (1 + K * (2 + hv)) && a.nA <= 64 && a.nC <= 64;
}

// The chain layouts' weight-gradient problems over S_ row splits (split-bf16
// tiles + the output-layer GEMV, or the fp32 split-K GEMM): arguments and
// launch geometry, shared by the launch after the phase section and the
// per-chunk launches inside the two-stream pipeline
struct TNGeom {
  int S_ = 0, maxt = 0, maxt3 = 0, rps32 = 0;
  double tfl = 0.0;
  float* oslab = nullptr;
  long long sstride = 0;
};
// align > 0 (split-bf16 form): the row count of the first path chunk, which
// must then end on a split boundary -- when the default split does not, the
// largest 32-row multiple no longer than it that divides align is taken
int tn_setup(dbsde_ctx* c, int R, int Rp, TNArgs& ta, TNGeom& g, long long align = 0) {
  const auto& L = c->L;
  const int K = c->K, S = c->Stot, D = c->D;
  memset(&ta, 0, sizeof(ta));
  // row splits for this batch: at least DBSDE_TN_SPLIT_ROWS rows each, at
  // most the slab capacity; every kernel below covers all S_ splits, empty
  // ones writing zeros, and the finalize sums exactly S_ of them
  int S_ = std::min(c->tn_splits, std::max(8, (Rp + DBSDE_TN_SPLIT_ROWS - 1) / DBSDE_TN_SPLIT_ROWS));
  if (align > 0 && c->tnx3) {
    int r32 = ((Rp + S_ - 1) / S_ + 31) / 32 * 32;
    if (align % r32 != 0) {
      for (r32 -= 32; r32 >= 32 && align % r32 != 0; r32 -= 32) {
      }
      if (r32 >= 32 && (Rp + r32 - 1) / r32 <= c->tn_splits) S_ = (Rp + r32 - 1) / r32;
    }
  }
  g.S_ = c->tn_splits_cur = S_;
  const int rps = ((Rp + S_ - 1) / S_ + TN_KC - 1) / TN_KC * TN_KC;
  ta.rows_per_split = rps;
  ta.Rp = Rp;
  double& tfl = g.tfl;
  tfl = 0.0;
  {
    TNProb& p0 = ta.prob[0];
    p0.A[0] = c->Alpha;
    p0.lda[0] = S;
    p0.nA[0] = c->Stot_x;
    p0.B[0] = c->xin;
    p0.ldb[0] = c->Dp;
    p0.nB[0] = c->Dp;
    p0.A[1] = c->Delta;
    p0.lda[1] = S;
    p0.nA[1] = c->Stot_x;
    p0.B[1] = c->zbar;
    p0.ldb[1] = c->Dp;
    p0.nB[1] = c->Dp;
    p0.npairs = 2;
    p0.ones_col = -1;
    p0.mv = c->slab_mv[0];
    p0.nv = c->slab_nv[0];
    p0.mt = c->slab_mt[0];
    p0.nt = c->slab_nt[0];
    p0.slab = c->slab[0];
    tfl += 2.0 * 2.0 * R * nv_x(c) * (D + 2);
  }
  int& maxt = g.maxt;
  maxt = ta.prob[0].mt * ta.prob[0].nt;
  for (int j = 1; j <= K; ++j) {
    TNProb& pj = ta.prob[j];
    pj.A[0] = c->Alpha + c->col[j];
    pj.lda[0] = S;
    pj.nA[0] = c->Wp[j];
    pj.B[0] = c->H + c->col[j - 1];
    pj.ldb[0] = S;
    pj.nB[0] = c->Wp[j - 1];
    pj.A[1] = c->Delta + c->col[j];
    pj.lda[1] = S;
    pj.nA[1] = c->Wp[j];
    pj.B[1] = c->Hdot + c->col[j - 1];
    pj.ldb[1] = S;
    pj.nB[1] = c->Wp[j - 1];
    pj.npairs = 2;
    pj.ones_col = c->has_v ? -1 : c->Wp[j - 1];
    pj.mv = c->slab_mv[j];
    pj.nv = c->slab_nv[j];
    pj.mt = c->slab_mt[j];
    pj.nt = c->slab_nt[j];
    pj.slab = c->slab[j];
    maxt = std::max(maxt, pj.mt * pj.nt);
    tfl += 2.0 * 2.0 * R * L[j] * (L[j + 1] + (c->has_v ? 0 : 1));
  }
  {
    // output layer: [w_out | b_out] = sum_r ubar_r [h_{K+1} | 1] + hdot_{K+1}
    TNProb& po = ta.prob[K + 1];
    po.A[0] = c->u16;
    po.lda[0] = 16;
    po.nA[0] = 16;
    po.B[0] = c->H + c->col[K];
    po.ldb[0] = S;
    po.nB[0] = c->Wp[K];
    po.A[1] = c->o16;
    po.lda[1] = 16;
    po.nA[1] = 16;
    po.B[1] = c->Hdot + c->col[K];
    po.ldb[1] = S;
    po.nB[1] = c->Wp[K];
    po.npairs = 2;
    po.ones_col = c->Wp[K];
    po.mv = 1;
    po.nv = c->slab_nv[K + 1];
    po.mt = c->slab_mt[K + 1];
    po.nt = c->slab_nt[K + 1];
    po.slab = c->slab[K + 1];
    maxt = std::max(maxt, po.mt * po.nt);
    tfl += 2.0 * 2.0 * R * (L[K + 1] + 1);
  }
  if (K + 2 > 8) return fail(c, DBSDE_EINVAL, "internal: too many TN problems");
  if (c->tnx3) {
    for (int j = 0; j <= K; ++j)
      g.maxt3 = std::max(g.maxt3, ((ta.prob[j].nA[0] + TX_TILE - 1) / TX_TILE) * ((ta.prob[j].nB[0] + TX_TILE - 1) / TX_TILE));
    g.rps32 = ((Rp + S_ - 1) / S_ + 31) / 32 * 32;
    // tn_out_kernel's float4 loads at H + col[K] + r S: 16-byte aligned rows and column
    if (Rp % 32 != 0 || c->Wp[K] % 4 != 0 || c->col[K] % 4 != 0 || S % 4 != 0)
      return fail(c, DBSDE_EINVAL, "internal: tn x3 geometry");
    const TNProb& po = ta.prob[K + 1];
    g.oslab = po.slab;
    g.sstride = (long long)po.mt * 64 * po.nt * 64;
  }
  return DBSDE_OK;
}
// split-bf16 chain weight gradients of row splits [s0, s0 + sn) on stream st
int tn_launch_splits(dbsde_ctx* c, int R, TNArgs ta, const TNGeom& g, int s0, int sn, hipStream_t st) {
  const int K = c->K, S = c->Stot;
  ta.split0 = s0;
  tn_x3_kernel<<<dim3(g.maxt3, sn, K + 1), 256, 0, st>>>(ta, g.rps32);
  tn_out_kernel<<<dim3(sn, (c->Wp[K] + 255) / 256), 1024, 0, st>>>(c->u16, c->H + c->col[K], c->Hdot + c->col[K], S,
                                                                    c->Wp[K], R, g.rps32, g.oslab, g.sstride, s0);
  HIPC(c, hipGetLastError());
  return DBSDE_OK;
}

// Everything after the cotangents: for the per-layer (chain) form the forward
// tangent along zbar and the reverse, then the weight-gradient contraction and
// the finalize (+ the fused optimizer update).  Shared by loss_grad_impl and
// the net_u VJP.
int backward_tail(dbsde_ctx* c, const float* params, int R, int Rp, int fv, float* grad, const double* loss_part,
                  int nloss_parts, float* loss_dst, const FusedOpt* fo, bool tnw_piped, bool tn_piped) {
  int rc;
  hipStream_t s = c->stream;
  const auto& L = c->L;
  const int K = c->K, S = c->Stot, D = c->D;
  if (fv < 0) {
    // ---- forward tangent along zbar
    {
      ChainArgs a = base_args(c);
      a.A = c->zbar;
      a.lda = c->Dp;
      a.Bt = c->BtIn;
      x3_weights(c, a, c->imgX[0], c->Wp[0] / 16, c->Dp / 16);
      a.ldb = c->Dp;
      a.K = c->Dp;
      a.in[0] = c->Abuf;
      a.ldi[0] = S;
      a.out[0] = c->Adot;
      a.ldo[0] = S;
      a.out[1] = c->Hdot;
      a.ldo[1] = S;
      a.lvl0_cols = c->Wp[0];
      const int nv = nv_x(c);
      if ((rc = chain<EPI_TAN0>(c, "gemm_xstack_tangent", a, Rp, c->Stot_x, nt_for(c->Wp[0]),
                                2.0 * R * D * nv, 4.0 * R * (D + 2.0 * nv + L[1]))))
        return rc;
    }
    for (int j = 1; j <= K; ++j) {
      ChainArgs a = base_args(c);
      a.A = c->Hdot + c->col[j - 1];
      a.lda = S;
      a.Bt = c->Bf[j];
      x3_weights(c, a, c->imgF[j], c->Wp[j] / 16, c->Wp[j - 1] / 16);
      a.ldb = c->Wp[j - 1];
      a.K = c->Wp[j - 1];
      a.in[0] = c->has_v ? c->Adot + c->col[j] : nullptr;
      a.ldi[0] = S;
      a.in[1] = c->Hdot + c->col[j - 1];
      a.ldi[1] = S;
      a.in[2] = c->Abuf + c->col[j];
      a.ldi[2] = S;
      a.out[0] = c->Adot + c->col[j];
      a.ldo[0] = S;
      a.out[1] = c->Hdot + c->col[j];
      a.ldo[1] = S;
      a.last = j == K;
      a.out[2] = c->Alpha + c->col[K];
      a.ldo[2] = S;
      a.vec[0] = c->wout;
      a.ubar = c->ubar;
      if ((rc = chain<EPI_TAN>(c, "gemm_block_tangent", a, Rp, c->Wp[j], nt_for(c->Wp[j]),
                               2.0 * R * L[j] * L[j + 1], 4.0 * R * (L[j] + 6.0 * L[j + 1]))))
        return rc;
    }
    // ---- reverse over (primal, tangent)
    for (int j = K; j >= 1; --j) {
      ChainArgs a = base_args(c);
      a.A = c->Alpha + c->col[j];
      a.lda = S;
      a.Bt = c->Bb[j];
      x3_weights(c, a, c->imgB[j], c->Wp[j - 1] / 16, c->Wp[j] / 16);
      a.ldb = c->Wp[j];
      a.K = c->Wp[j];
      a.in[0] = j == K ? nullptr : c->Pbuf[(j + 1) & 1];
      a.ldi[0] = c->Wmax;
      a.ubar = c->ubar;
      a.vec[0] = c->wout;
      a.in[1] = c->Abuf + c->col[j - 1];
      a.ldi[1] = S;
      a.in[2] = c->G + c->col[j - 1];
      a.ldi[2] = S;
      a.in[3] = c->Adot + c->col[j - 1];
      a.ldi[3] = S;
      a.out[0] = c->Pbuf[j & 1];
      a.ldo[0] = c->Wmax;
      a.out[1] = c->Alpha + c->col[j - 1];
      a.ldo[1] = S;
      if ((rc = chain<EPI_REV>(c, "gemm_block_reverse", a, Rp, c->Wp[j - 1], nt_for(c->Wp[j - 1]),
                               2.0 * R * L[j] * L[j + 1], 4.0 * R * (L[j + 1] + 6.0 * L[j]))))
        return rc;
    }
  }
  if (!grad) return DBSDE_OK;   // (dbsde_net_u_xvjp without grad: the sweeps above completed Alpha)
  // ---- parameter gradients
  if (c->tnw) {
    if (!tnw_piped && (rc = launch_tnw(c, R, Rp))) return rc;
    if ((rc = finalize_grads(c, params, grad, loss_part, nloss_parts, loss_dst, fo))) return rc;
  } else {
  if (!tn_piped) {
    TNArgs ta;
    TNGeom g;
    if ((rc = tn_setup(c, R, Rp, ta, g))) return rc;
    if (c->tnx3) {
      const int S_ = g.S_, rps32 = g.rps32;
      RUN(c, s, "tn_weight_grad", g.tfl, 0.0,
          tn_x3_kernel<<<dim3(g.maxt3, S_, K + 1), 256, 0, s>>>(ta, rps32);
          tn_out_kernel<<<dim3(S_, (c->Wp[K] + 255) / 256), 1024, 0, s>>>(c->u16, c->H + c->col[K], c->Hdot + c->col[K],
                                                                           S, c->Wp[K], R, rps32, g.oslab, g.sstride, 0));
    } else {
      RUN(c, s, "tn_weight_grad", g.tfl, 0.0, tn_gemm_kernel<<<dim3(g.maxt, g.S_, K + 2), 256, 0, s>>>(ta));
    }
  }
  if ((rc = finalize_grads(c, params, grad, loss_part, nloss_parts, loss_dst, fo))) return rc;
  }
  return DBSDE_OK;
}

// resident workgroups of the chip for a phase variant (two per CU for the
// 64-row and column-split kernels, one for the 512-register ones), queried once
int variant_slots(dbsde_ctx* c, int fv) {
  if (c->fv_slots[fv] == 0) {
    int per = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kFused[fv].A, 64 * P3_WAVES, 0) != hipSuccess) per = 1;
    c->fv_slots[fv] = std::max(1, per) * c->cus;
  }
  return c->fv_slots[fv];
}

// dbsde_loss_grad, and dbsde_train_step's fused form (fo != NULL: the
// optimizer update is applied inside the gradient finalize)
int loss_grad_impl(dbsde_ctx* c, const float* params, const dbsde_batch* b, float* grad, const dbsde_outputs* out,
                   const FusedOpt* fo) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (!params) return fail(c, DBSDE_EINVAL, "params is NULL");
  int rc = validate_batch(c, b);
  if (rc) return rc;
  HIPC(c, hipSetDevice(c->device));
  const int M = b->M, N = b->N, N1 = N + 1, D = c->D, K = c->K, S = c->Stot;
  const int R = M * N1, Rp = pad_rows(R);
  if ((rc = ensure_rows(c, Rp, N))) return rc;
  hipStream_t s = c->stream;
  const auto& L = c->L;
  const dbsde_problem& pr = c->cfg.problem;

  // a held-back prefetch of this very batch: issue it now (its consumer)
  if ((rc = flush_deferred(c, nullptr, b))) return rc;
  // weight repack (projection, norms, fragment images) overlaps the rollout
  if ((rc = prep_weights(c, params))) return rc;

  // ---- rollout (network-independent: mu/sigma never read Y, Z), unless
  // dbsde_prefetch already produced this batch's paths
  bool from_pf = false;
  if ((rc = select_paths(c, b, from_pf))) return rc;
  if (!from_pf && (rc = issue_rollout(c, *b, c->ps.cur, s, false))) return rc;
  const bool q3 = pr.q3 && D == 1;
  if (q3 && (rc = q3_sum(c, M, N))) return rc;

  int nloss_parts;
  bool tnw_piped = false, tn_piped = false;
  TNArgs tn_a;
  TNGeom tn_g;
  FusedArgs fa;
  // weight-gradient row slices: always the slab capacity.  Fewer, longer
  // slices at small batches (48 at M = 128, four 32-row steps each) cut the
  // finalize's slab reads (23.9 -> 22.4 us) but leave the weight-gradient
  // kernel with a third of the waves (33 -> 49 us,
  // profiles/r4_ab_column_split.txt)
  c->tnw_S = c->tnw_Smax;
  int fv = c->fv;
  // small batches: the column-split kernels when all their 16-row workgroups
  // are resident at once (M <= 128 per GPU at the north star); past that their
  // 4x workgroup count costs more than the shorter chains save (M = 256:
  // 0.235 vs 0.209 ms/step, profiles/r4_ab_column_split.txt)
  if (fv >= 0 && c->fv_cs >= 0 &&
      (c->cs_mode == 1 || (c->cs_mode == 2 && Rp / CS_ROWS <= variant_slots(c, c->fv_cs))))
    fv = c->fv_cs;
  if (fv >= 0) {
    fa = fused_args(c, R, Rp, N1, q3);
    if (!fused_piece_counts_ok(c, fa)) return fail(c, DBSDE_EINVAL, "internal: fused kernel piece counts");
    const int nv = nv_x(c);
    const double flA = 2.0 * R * ((D + 1.0) * nv + 2.0 * K * L[1] * (double)L[1] + (double)nv * D);
    const double byA = 4.0 * R * (c->Dp + 4.0 * S + 8.0);
    const double flC = 2.0 * R * ((double)nv * D + 2.0 * K * L[1] * (double)L[1]);
    const double byC = 4.0 * R * (4.0 * c->Dp + 5.0 * S);
    // chunks of whole paths and whole WR-row tiles (WR paths = WR (N+1) rows =
    // N+1 tiles), WR = the variant's rows per workgroup
    const int WR = kFused[fv].rows;
    // workgroup slots of the chip for this variant (two per CU for the
    // 64-row kernels, one for the 512-register ones)
    const int slots = variant_slots(c, fv);
    int nch = !grad ? 1 : (c->chunks > 0 ? c->chunks : (Rp / WR > slots ? 2 : 1));
    while (nch > 1 && (M % WR != 0 || (M / WR) % nch != 0)) --nch;
    if (nch <= 1) {
      if ((rc = flush_deferred(c, c->xin))) return rc;
      RUN(c, s, "fused_fwd_inputgrad", flA, byA, kFused[fv].A<<<Rp / WR, 64 * P3_WAVES, 0, s>>>(fa));
    } else {
      // phase A / phase C of chunk i on stream (i even ? main : pipe2); the
      // two phases are timed as one pipelined segment
      // equal chunks in units of WR paths
      const int units = M / WR, utile = N1;   // WR paths = N1 tiles
      std::vector<int> cu(nch, units / nch);
      if (c->prof) HIPC(c, hipEventRecord(c->ev_prof[0], s));
      const int np = std::min(2, nch);
      // Unprofiled steps run each chunk's weight-gradient row slices on the
      // chunk's stream right after its phase C (the slices of the first chunk
      // overlap the second chunk's phases; slice s covers 32-row steps
      // [s n32 / S, (s + 1) n32 / S), so the chunk boundary must be a slice
      // boundary).  Profiled steps keep them after the section, so the section
      // and the weight-gradient kernel are timed on their own.
      // sb[i]: the first slice of chunk i (sb[nch] = S); every chunk boundary
      // must be a slice boundary that is a multiple of 8 (the kernel's
      // slice groups)
      std::vector<int> sb(nch + 1, 0);
      {
        const int S = c->tnw_S, n32 = Rp / 32;
        bool ok = Rp % 32 == 0;
        long long crow = 0;
        sb[nch] = S;
        for (int i = 1; i < nch && ok; ++i) {
          crow += (long long)cu[i - 1] * utile * WR;
          for (int k = sb[i - 1] + 8; k < S && !sb[i]; k += 8)
            if (32LL * ((long long)k * n32 / S) == crow) sb[i] = k;
          ok = sb[i] > 0;
        }
        // (two chunks only: with more, a chunk's slices sit in front of the
        // next chunk's phase A on the same stream -- 4 chunks 0.607 vs 0.495
        // ms/step, profiles/r4_ab_chunks_piped.txt)
        tnw_piped = grad && c->tnw && !c->prof && np == 2 && nch == 2 && ok;
      }
      // the chain layouts' split-bf16 weight gradients the same way: row
      // splits of chunk 0 after its phase C on the main stream, the rest after
      // chunk 1's on the second (the chunk boundary must be a split boundary)
      int tn_s0 = 0;
      if (grad && !c->tnw && c->tnx3 && !c->prof && np == 2 && nch == 2) {
        const long long crow = (long long)cu[0] * utile * WR;
        if ((rc = tn_setup(c, R, Rp, tn_a, tn_g, crow))) return rc;
        if (tn_g.rps32 > 0 && crow % tn_g.rps32 == 0 && crow / tn_g.rps32 < tn_g.S_) {
          tn_s0 = (int)(crow / tn_g.rps32);
          tn_piped = true;
        }
      }
      if (!tnw_piped && !tn_piped && (rc = flush_deferred(c, c->xin))) return rc;
      hipStream_t ps[2] = {s, c->pipe2};
      if (np > 1 && (rc = stream_order(c, s, c->pipe2, ORD_FORK))) return rc;
      int t0 = 0;
      for (int i = 0; i < nch; ++i) {
        hipStream_t st = ps[i % np];
        FusedArgs fc = fa;
        fc.tile0 = t0;
        // the last chunk also runs the padding tiles past R (Rp > R when the
        // workgroup is 16 rows and R is not a multiple of the 64-row padding):
        // the loss partials and the weight-gradient rows of every tile up to
        // Rp / WR are then written by this step
        const int tiles = i + 1 < nch ? cu[i] * utile : Rp / WR - t0;
        kFused[fv].A<<<tiles, 64 * P3_WAVES, 0, st>>>(fc);
        kFused[fv].C<<<tiles, 64 * P3_WAVES, 0, st>>>(fc);
        if (tnw_piped && (rc = launch_tnw(c, R, Rp, sb[i], sb[i + 1] - sb[i], st))) return rc;
        if (tn_piped && (rc = tn_launch_splits(c, R, tn_a, tn_g, i == 0 ? 0 : tn_s0,
                                               i == 0 ? tn_s0 : tn_g.S_ - tn_s0, st)))
          return rc;
        t0 += tiles;
      }
      HIPC(c, hipGetLastError());
      // the pending prefetched rollouts (this step's other buffer, started a
      // step ago) are waited for on the second chunk stream, so the join orders
      // the main stream after them too
      if ((rc = join_pending(c, c->pipe2, s))) return rc;
      if ((rc = stream_order(c, c->pipe2, s, ORD_JOIN))) return rc;
      // the held-back batch after the join: beside this step's tail, not in
      // front of it (profiles/r6_ab_rollout.txt 6)
      if ((tnw_piped || tn_piped) && (rc = launch_deferred_on(c, c->pipe2))) return rc;
      if (c->prof) {
        HIPC(c, hipEventRecord(c->ev_prof[1], s));
        HIPC(c, hipEventSynchronize(c->ev_prof[1]));
        float ms = 0.f;
        HIPC(c, hipEventElapsedTime(&ms, c->ev_prof[0], c->ev_prof[1]));
        ProfAgg& ag = c->agg[prof_id(c, "fused_phases_pipelined")];
        ag.ms += ms;
        ag.flops += flA + flC;
        ag.bytes += byA + byC;
        ag.n += 1;
      }
    }
    if (grad) {
      if (nch <= 1)
        RUN(c, s, "fused_tangent_reverse", flC, byC, kFused[fv].C<<<Rp / WR, 64 * P3_WAVES, 0, s>>>(fa));
      nloss_parts = Rp / WR;
    } else {
      RUN(c, s, "loss_rows", 0.0, 4.0 * R * 3.0 * D,
          cotan_kernel<<<Rp / 16, 256, 0, s>>>(cotan_params(c, R, Rp, N1, q3), c->loss_part));
      nloss_parts = Rp / 16;
    }
  } else {
    if ((rc = flush_deferred(c, c->xin))) return rc;
    if ((rc = forward_and_inputgrad(c, R, Rp))) return rc;

    // ---- Z GEMM + residuals / cotangents / loss rows
    if (c->Dp > 128) {
      // wide contexts: the Z GEMM over column tiles, then the row kernel
      // (fused.hpp zrow_cotan_kernel) for what needs a whole Z row
      if ((rc = zgemm_wide(c, "gemm_z", R, Rp))) return rc;
      ZRowArgs za{};
      za.p = cotan_params(c, R, Rp, N1, q3);
      za.umask = c->u_clamp ? c->umask : nullptr;
      za.zfull = c->zfull;
      za.zbar = c->zbar;
      za.rres = c->rres;
      za.lossrow = c->lossrow;
      za.dphidy = c->dphidy;
      RUN(c, s, "z_row_cotangent", 12.0 * R * D, 4.0 * R * (5.0 * c->Dp),
          zrow_cotan_kernel<<<Rp / 16, 256, 0, s>>>(za));
    } else {
      ChainArgs a = base_args(c);
      zgemm_args(c, a);
      a.R = R;
      a.N1 = N1;
      a.D = D;
      a.xin = c->xin;
      a.sdw = c->sdw;
      a.ldx = c->Dp;
      a.u = c->u;
      a.q3S = q3 ? c->q3S : nullptr;
      a.umask = c->u_clamp ? c->umask : nullptr;
      a.phi_r = pr.phi_r;
      a.phi_c = pr.phi_c;
      a.phi_zz = pr.phi_zz;
      a.strike = pr.strike;
      a.g_alpha = pr.g_alpha;
      a.g_kind = terminal_kind(pr.g_kind, a.gsign);
      a.gcols = c->gcols;
      a.pen = pr.pen;
      a.dphidy = c->dphidy;
      a.zbar = c->zbar;
      a.rres = c->rres;
      a.lossrow = c->lossrow;
      if ((rc = chain<EPI_COTAN>(c, "gemm_z_cotangent", a, Rp, c->Dp, c->Dp / 16, zgemm_flops(c, R),
                                 4.0 * R * (c->Stot_x + 5.0 * D))))
        return rc;
    }
    RUN(c, s, "ubar_loss", 0.0, 16.0 * R,
        ubar_kernel<<<Rp / 256 + 1, 256, 0, s>>>(c->rres, c->xin, c->Dp, R, Rp, N1, pr.phi_r, c->lossrow, c->ubar,
                                                 c->u16, c->loss_part, c->u_clamp ? c->umask : nullptr,
                                                 pr.pen != 0.f ? c->dphidy : nullptr));
    nloss_parts = Rp / 256 + 1;
  }
  float* loss_dst = (out && out->loss) ? out->loss : c->loss_tmp;
  // the loss sum: inside the gradient finalize (tilefin_kernel or
  // slabsum_kernel), else (no gradient) its own launch
  const bool loss_in_fin = grad;
  if (!loss_in_fin)
    RUN(c, s, "loss_final", 0.0, 0.0, loss_final_kernel<<<1, 256, 0, s>>>(c->loss_part, nloss_parts, loss_dst));

  if (grad && (rc = backward_tail(c, params, R, Rp, fv, grad, c->loss_part, nloss_parts, loss_dst, fo, tnw_piped,
                                  tn_piped)))
    return rc;
  if ((rc = flush_deferred(c, c->xin))) return rc;   // (every path above has issued it already)

  if (out && (out->X || out->Y || out->Z)) {
    const long long n = (long long)R * D;
    RUN(c, s, "export", 0.0, 0.0,
        export_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(c->xin, c->zfull, c->Dp, c->u, R, D, out->X,
                                                                  out->Y, out->Z, nullptr));
  }
  return DBSDE_OK;
}

// dbsde_optim -> the kernel's OptArgs (scalar factors in double, as
// torch.optim computes them in Python floats)
int make_optargs(dbsde_ctx* c, const dbsde_optim* o, OptArgs& a) {
  if (o->kind < DBSDE_OPT_ADAM || o->kind > DBSDE_OPT_ASGD) return fail(c, DBSDE_EINVAL, "unknown optimizer kind");
  if (o->step < 1) return fail(c, DBSDE_EINVAL, "step must be >= 1");
  a = OptArgs{};
  a.kind = o->kind;
  a.lr = o->lr;
  a.beta2 = o->beta2;
  a.eps = o->eps;
  a.wd = o->weight_decay;
  a.max_norm = o->max_norm;
  a.omb1 = (float)(1.0 - (double)o->beta1);
  a.omb2 = (float)(1.0 - (double)o->beta2);
  const double t = (double)o->step;
  const double bc1 = 1.0 - std::pow((double)o->beta1, t);
  const double bc2 = 1.0 - std::pow((double)o->beta2, t);
  a.step_size = (float)((double)o->lr / bc1);
  a.bc2_sqrt = (float)std::sqrt(bc2);
  a.alpha = o->alpha;
  a.rho = o->rho;
  if (o->kind == DBSDE_OPT_RMSPROP) a.omb2 = (float)(1.0 - (double)o->alpha);
  if (o->kind == DBSDE_OPT_ADADELTA) a.omb2 = (float)(1.0 - (double)o->rho);
  if (o->kind == DBSDE_OPT_ADAGRAD) a.step_size = (float)((double)o->lr / (1.0 + (t - 1.0) * (double)o->lr_decay));
  if (o->kind == DBSDE_OPT_ASGD) {
    a.asgd_eta = o->asgd_eta;
    a.asgd_decay = (float)(1.0 - (double)o->lambd * (double)o->asgd_eta);
    a.asgd_mu = o->asgd_mu;
    a.asgd_copy = o->asgd_mu == 1.f;
  }
  a.loss = o->loss;
  a.nparts = c->opt_nparts;
  if (o->step_state) {
    if (o->step_parity != 0 && o->step_parity != 1) return fail(c, DBSDE_EINVAL, "step_parity must be 0 or 1");
    a.state = o->step_state;
    a.parity = o->step_parity;
    a.lr_d = o->lr;
    a.beta1_d = o->beta1;
    a.beta2_d = o->beta2;
    a.lr_decay_d = o->lr_decay;
    a.lambd_d = o->lambd;
    a.asgd_alpha_d = 0.75;   // torch.optim.ASGD defaults (alpha, t0)
    a.asgd_t0_d = 1e6;
  }
  return DBSDE_OK;
}
// dbsde_net_u_vjp / dbsde_net_u_xvjp: grad (nullable) and xbar (nullable, [R, D])
int net_u_vjp_impl(dbsde_ctx* c, const float* params, int R, const float* t, const float* X, const float* ubar,
                   const float* zbar, float* grad, float* xbar) {
  HIPC(c, hipSetDevice(c->device));
  const int Rp = pad_rows(R), D = c->D;
  int rc;
  if ((rc = ensure_rows(c, Rp, 1))) return rc;
  hipStream_t s = c->stream;
  if ((rc = prep_weights(c, params))) return rc;
  bool from_pf;
  if ((rc = flush_deferred(c))) return rc;
  if ((rc = select_paths(c, nullptr, from_pf))) return rc;
  const long long n = (long long)Rp * c->Dp;
  const unsigned nb = (unsigned)((n + 255) / 256);
  RUN(c, s, "netu_input", 0.0, 0.0, netu_input_kernel<<<nb, 256, 0, s>>>(t, X, R, D, c->Dp, c->xin));
  if (Rp > R) HIPC(c, hipMemsetAsync(c->xin + (size_t)R * c->Dp, 0, (size_t)(Rp - R) * c->Dp * 4, s));
  // xbar = (Alpha[:, :Stot_x] . W)[:, 1..D] once Alpha is final (fused: after
  // phase C; per-layer form: after backward_tail's reverse sweep)
  auto input_cotangent = [&]() -> int {
    if (c->n_prepz)   // fused contexts pack only the fragment images per step
      RUN(c, s, "pack_weights_z", 0.0, 0.0,
          pack_tagged_kernel<<<dim3(c->prepz_blocks, c->n_prepz), 256, 0, s>>>(c->d_prepz, params, nullptr));
    XbarArgs xa{};
    xa.Alpha = c->Alpha;
    xa.lda = c->Stot;
    xa.Wt = c->BtZ;
    xa.K = c->Stot_x;
    xa.Dp = c->Dp;
    xa.R = R;
    xa.D = D;
    xa.xbar = xbar;
    int ok = 0;
    RUN(c, s, "netu_xbar", 2.0 * R * c->Stot_x * (double)D, 4.0 * (R * ((double)c->Stot_x + D) + (double)c->Stot_x * c->Dp),
        ok = netu_xbar_launch(xa, s));
    if (ok) return fail(c, DBSDE_EINVAL, "internal: netu_xbar geometry");
    return DBSDE_OK;
  };
  const int fv = c->fv;
  if (fv >= 0) {
    // ubar -> rres rows, zbar -> the sdw rows phase C reads (phase A's use of
    // sdw only feeds the residual row sums, unused here)
    RUN(c, s, "vjp_cotangents", 0.0, 0.0,
        ext_cotan_kernel<<<nb, 256, 0, s>>>(ubar, zbar, R, Rp, D, c->Dp, nullptr, c->rres, c->sdw, nullptr));
    FusedArgs fa = fused_args(c, R, Rp, 1, false);
    if (!fused_piece_counts_ok(c, fa)) return fail(c, DBSDE_EINVAL, "internal: fused kernel piece counts");
    fa.cp.ext = 1;
    fa.cp.ext_ub = c->rres;
    const int WR = kFused[fv].rows;
    RUN(c, s, "fused_fwd_inputgrad", 0.0, 0.0, kFused[fv].A<<<Rp / WR, 64 * P3_WAVES, 0, s>>>(fa));
    RUN(c, s, "fused_tangent_reverse", 0.0, 0.0, kFused[fv].C<<<Rp / WR, 64 * P3_WAVES, 0, s>>>(fa));
    if (xbar && (rc = input_cotangent())) return rc;
    if (!grad) return DBSDE_OK;   // no weight-gradient launches, no finalize
  } else {
    if ((rc = flush_deferred(c, c->xin))) return rc;
    if ((rc = forward_and_inputgrad(c, R, Rp))) return rc;
    RUN(c, s, "vjp_cotangents", 0.0, 0.0,
        ext_cotan_kernel<<<nb, 256, 0, s>>>(ubar, zbar, R, Rp, D, c->Dp, c->u_clamp ? c->umask : nullptr, c->ubar,
                                            c->zbar, c->u16));
  }
  c->tnw_S = c->tnw_Smax;
  if ((rc = backward_tail(c, params, R, Rp, fv, grad, nullptr, 0, nullptr, nullptr, false, false))) return rc;
  if (fv < 0 && xbar && (rc = input_cotangent())) return rc;
  return DBSDE_OK;
}

}  // namespace

int jet_pack_weights(dbsde_ctx* c, const float* params, bool full) {
  int rc;
  if (full && (rc = prep_weights(c, params))) return rc;
  hipStream_t s = c->stream;
  if (c->n_prepj)   // fused contexts pack only the fragment images per step
    RUN(c, s, "pack_weights_jet", 0.0, 0.0,
        pack_tagged_kernel<<<dim3(c->prepj_blocks, c->n_prepj), 256, 0, s>>>(c->d_prepj, params, nullptr));
  return DBSDE_OK;
}

extern "C" {

int dbsde_loss_grad(dbsde_ctx* c, const float* params, const dbsde_batch* b, float* grad,
                    const dbsde_outputs* out) {
  return loss_grad_impl(c, params, b, grad, out, nullptr);
}

int dbsde_train_step(dbsde_ctx* c, float* params, const dbsde_batch* b, float* grad, float* m, float* v,
                     const dbsde_optim* o, const dbsde_outputs* out) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (!params || !grad || !o) return fail(c, DBSDE_EINVAL, "bad train_step arguments");
  // the update can ride in the gradient finalize when nothing needs the whole
  // gradient first: no clip (global norm), no NaN skip (the loss), a device
  // step counter, and the tile finalize (wave-owned weight-gradient layouts)
  const bool fuse = c->tnw && o->max_norm <= 0.f && !o->loss && o->step_state;
  if (!fuse) {
    int rc = loss_grad_impl(c, params, b, grad, out, nullptr);
    if (rc) return rc;
    return dbsde_optimizer_step(c, params, grad, m, v, o);
  }
  const bool needs_m = o->kind == DBSDE_OPT_ADAM || o->kind == DBSDE_OPT_ADAMW || o->kind == DBSDE_OPT_ADAMAX ||
                       o->kind == DBSDE_OPT_ADADELTA || o->kind == DBSDE_OPT_ASGD;
  const bool needs_v = o->kind != DBSDE_OPT_SGD && o->kind != DBSDE_OPT_ASGD;
  if ((needs_m && !m) || (needs_v && !v)) return fail(c, DBSDE_EINVAL, "optimizer state buffer is NULL");
  FusedOpt fo{};
  int rc = make_optargs(c, o, fo.a);
  if (rc) return rc;
  fo.prm = params;
  fo.m = m;
  fo.v = v;
  return loss_grad_impl(c, params, b, grad, out, &fo);
}

int dbsde_net_u(dbsde_ctx* c, const float* params, int R, const float* t, const float* X, float* u, float* Du) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (!params || !t || !X || R < 1) return fail(c, DBSDE_EINVAL, "bad net_u arguments");
  HIPC(c, hipSetDevice(c->device));
  const int Rp = pad_rows(R), D = c->D;
  int rc;
  if ((rc = ensure_rows(c, Rp, 1))) return rc;
  hipStream_t s = c->stream;
  if ((rc = prep_weights(c, params))) return rc;
  const long long n = (long long)Rp * c->Dp;
  bool from_pf;
  if ((rc = flush_deferred(c))) return rc;
  if ((rc = select_paths(c, nullptr, from_pf))) return rc;
  RUN(c, s, "netu_input", 0.0, 0.0,
      netu_input_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(t, X, R, D, c->Dp, c->xin));
  if (Rp > R) HIPC(c, hipMemsetAsync(c->xin + (size_t)R * c->Dp, 0, (size_t)(Rp - R) * c->Dp * 4, s));
  if (c->fv >= 0) {
    // the fused forward + input-gradient kernel writes u and Z (its residual
    // row sums read sdw, unused here)
    FusedArgs fa = fused_args(c, R, Rp, 1, false);
    if (!fused_piece_counts_ok(c, fa)) return fail(c, DBSDE_EINVAL, "internal: fused kernel piece counts");
    const int WR = kFused[c->fv].rows;
    RUN(c, s, "fused_fwd_inputgrad", 0.0, 0.0, kFused[c->fv].A<<<Rp / WR, 64 * P3_WAVES, 0, s>>>(fa));
  } else {
    if ((rc = forward_and_inputgrad(c, R, Rp))) return rc;
    if (c->Dp > 128) {
      if ((rc = zgemm_wide(c, "gemm_z", R, Rp))) return rc;
    } else {
      ChainArgs a = base_args(c);
      zgemm_args(c, a);
      if ((rc = chain<EPI_STORE>(c, "gemm_z", a, Rp, c->Dp, c->Dp / 16, zgemm_flops(c, R), 0.0))) return rc;
    }
  }
  const long long m = (long long)R * D;
  RUN(c, s, "export", 0.0, 0.0,
      export_kernel<<<(unsigned)((m + 255) / 256), 256, 0, s>>>(c->xin, c->zfull, c->Dp, c->u, R, D, nullptr, u,
                                                                Du, (c->fv < 0 && c->u_clamp) ? c->umask : nullptr));
  return DBSDE_OK;
}

// net_u's VJP (loss.backward through the reference's net_u outputs,
// nd_BSPDE_case.py:191-221 with create_graph=True): grad = d/dparams of
// sum_r ubar_r u_r + zbar_r . Du_r at the points (t, X).  The same backward as
// dbsde_loss_grad with the caller's cotangents in place of the BSDE residual
// ones: the fused phase kernels take them in phase C's prologue, the per-layer
// form in its ubar / zbar buffers.
int dbsde_net_u_vjp(dbsde_ctx* c, const float* params, int R, const float* t, const float* X, const float* ubar,
                    const float* zbar, float* grad) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (!params || !t || !X || !ubar || !zbar || !grad || R < 1) return fail(c, DBSDE_EINVAL, "bad net_u_vjp arguments");
  return net_u_vjp_impl(c, params, R, t, X, ubar, zbar, grad, nullptr);
}

// The same with the input cotangent: xbar = d/dX of the same scalar = ubar Du
// + H zbar, the reverse cotangents alpha_j the backward already forms
// contracted with the input-facing weights (xbar.hpp).
int dbsde_net_u_xvjp(dbsde_ctx* c, const float* params, int R, const float* t, const float* X, const float* ubar,
                     const float* zbar, float* grad, float* xbar) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (!params || !t || !X || !ubar || !zbar || (!grad && !xbar) || R < 1)
    return fail(c, DBSDE_EINVAL, "bad net_u_xvjp arguments");
  return net_u_vjp_impl(c, params, R, t, X, ubar, zbar, grad, xbar);
}

int dbsde_optimizer_step(dbsde_ctx* c, float* params, float* grad, float* m, float* v, const dbsde_optim* o) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (!params || !grad || !o) return fail(c, DBSDE_EINVAL, "bad optimizer arguments");
  const bool needs_m = o->kind == DBSDE_OPT_ADAM || o->kind == DBSDE_OPT_ADAMW || o->kind == DBSDE_OPT_ADAMAX ||
                       o->kind == DBSDE_OPT_ADADELTA || o->kind == DBSDE_OPT_ASGD;
  const bool needs_v = o->kind != DBSDE_OPT_SGD && o->kind != DBSDE_OPT_ASGD;
  if ((needs_m && !m) || (needs_v && !v)) return fail(c, DBSDE_EINVAL, "optimizer state buffer is NULL");
  OptArgs a;
  int rc = make_optargs(c, o, a);
  if (rc) return rc;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const long long n = c->nparams;
  if (o->max_norm > 0.f)
    RUN(c, s, "grad_sqnorm", 2.0 * n, 4.0 * n, sqnorm_kernel<<<c->opt_nparts, 256, 0, s>>>(grad, c->d_used, n, c->opt_part));
  RUN(c, s, "optimizer", 10.0 * n, 24.0 * n,
      optim_kernel<<<256, 256, 0, s>>>(params, grad, m, v, c->d_used, n, c->opt_part, a));
  return DBSDE_OK;
}

}  // extern "C"
