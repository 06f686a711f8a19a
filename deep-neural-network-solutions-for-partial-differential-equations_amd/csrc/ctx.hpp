// ctx.hpp -- the context behind the C ABI of include/dbsde.h and what the host
// units share: net.hip (layout, buffers, streams, profiling), rollout.hip
// (paths and their prefetch scheduler), step.hip (the training step, net_u,
// the optimizer) and vec.hip (L-BFGS vector operations).
//
// kernels.hpp defines its plain (non-template) kernels in one unit only,
// step.hip: every other unit defines DBSDE_DEVICE_HELPERS_ONLY before this
// header and sees the argument structs alone.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <strings.h>
#include <vector>

#include "../../include/dbsde.h"
#include "kernels.hpp"
#include "phase.hpp"
#include "phase2.hpp"
#include "phasecs.hpp"
#include "projw.hpp"

using namespace dbsde;

inline int pad16(int x) { return (x + 15) / 16 * 16; }
inline int padw(int x) { return x <= 128 ? pad16(x) : (x + 127) / 128 * 128; }
inline int nt_for(int w) { return w <= 128 ? w / 16 : 8; }
// the state-dimension cap: Dp = pad16(D + 2) <= DP_MAX, D <= 1022
constexpr int DP_MAX = 1024;
// spare zero rows of BtZ behind Dp for the wide Z GEMM's ragged last column tile
constexpr int ZG_PAD = 128;

// DBSDE_PROB_ASIAN (state [A, S_1..S_k], D = k + 1): why dbsde_create and
// dbsde_mc_value refuse the problem, or null
inline const char* asian_refusal(const dbsde_problem& pr, int D) {
  if (D < 2) return "the Asian state is [A, S_1..S_k]: D must be >= 2";
  if (pr.phi_c != 0.f) return "the Asian problem needs phi_c == 0 (X.Z would include A u_A)";
  if (pr.g_cols != 1) return "the Asian payoff is on the running average alone: g_cols must be 1";
  if (pr.g_kind == DBSDE_G_SUMSQ || pr.g_kind == DBSDE_G_LOG)
    return "the Asian problem takes the call and put payoffs only (not sumsq or log)";
  return nullptr;
}
// DBSDE_PROB_GEO_ASIAN (state [G, S_1..S_k]): asian_refusal's reasons, and the
// assets must stay positive (the closed form is GBM's)
inline const char* geo_asian_refusal(const dbsde_problem& pr, int D) {
  if (const char* why = asian_refusal(pr, D)) return why;
  if (pr.sig_b != 0.f) return "the geometric-average problem needs sig_b == 0 (log S needs positive assets)";
  return nullptr;
}
// DBSDE_PROB_BARRIER (DIAG's state, h_kappa the barrier level B): why
// dbsde_create and dbsde_mc_value refuse the problem, or null.  Only the regular
// barriers (B on the payoff's zero side of the strike), so g and its gradient
// vanish on a knocked state.
inline const char* barrier_refusal(const dbsde_problem& pr) {
  const float B = pr.h_kappa;
  if (!(B > 0.f) || std::isinf(B)) return "h_kappa (the barrier level B of kind BARRIER) must be finite and > 0";
  if (pr.g_kind != DBSDE_G_CALL_SUM && pr.g_kind != DBSDE_G_CALL_MEAN && pr.g_kind != DBSDE_G_PUT_SUM &&
      pr.g_kind != DBSDE_G_PUT_MEAN)
    return "g_kind: the barrier problem takes call_sum, call_mean, put_sum and put_mean only (its payoff must vanish "
           "beyond the barrier)";
  const bool put = pr.g_kind >= DBSDE_G_PUT_SUM;
  if (!put && B > pr.strike)
    return "h_kappa (the barrier B) must be <= strike for a down-and-out call (reverse barriers need an indicator payoff)";
  if (put && B < pr.strike)
    return "h_kappa (the barrier B) must be >= strike for an up-and-out put (reverse barriers need an indicator payoff)";
  if (pr.pen != 0.f) return "pen != 0 cannot be combined with the barrier problem";
  if (pr.q3) return "q3 cannot be combined with the barrier problem";
  if (pr.u_clamp) return "u_clamp cannot be combined with the barrier problem";
  if (pr.h_theta != 0.f) return "h_theta must be 0 for the barrier problem (only h_kappa is used: the barrier level)";
  if (pr.h_sigma != 0.f) return "h_sigma must be 0 for the barrier problem (only h_kappa is used: the barrier level)";
  if (pr.h_rho != 0.f) return "h_rho must be 0 for the barrier problem (only h_kappa is used: the barrier level)";
  return nullptr;
}
// dbsde_problem.pen (the penalised American driver): why dbsde_create refuses
// the problem, or null
inline const char* pen_refusal(const dbsde_problem& pr) {
  if (pr.pen == 0.f) return nullptr;
  if (!(pr.pen > 0.f) || std::isinf(pr.pen)) return "pen must be finite and >= 0";
  if (pr.kind != DBSDE_PROB_DIAG)
    return "pen != 0 (the penalised American driver) is taken for DBSDE_PROB_DIAG only, not the Heston, Asian or "
           "geometric-Asian kinds";
  if (pr.u_clamp) return "pen != 0 cannot be combined with u_clamp";
  return nullptr;
}

struct Lin {
  long long w = -1, b = -1;
  int out = 0, in = 0;
};

struct ProfAgg {
  std::string name;
  double ms = 0, flops = 0, bytes = 0;
  long long n = 0;
};
struct ProfRec {
  int id;
  hipEvent_t e0, e1;
  double flops, bytes;
};

// The two path buffers and the rollouts prefetched into them; rollout.hip's
// scheduler (pick_buffer .. drop_all) is the only code that changes this state.
struct PathSched {
  // path buffers (xin, sdw) x 2: a device-mode rollout can be prefetched into
  // the buffer the queued work no longer reads (dbsde_prefetch) on pf_stream
  float* xin_b[2] = {nullptr, nullptr};
  float* sdw_b[2] = {nullptr, nullptr};
  int cur = 0;   // the buffer ctx xin / sdw point at (select_paths)
  struct Pending {
    bool valid = false;
    dbsde_batch b{};
    hipEvent_t ready = nullptr;
    unsigned long long ready_v = 0;   // its order_mark token
    // joined_to is already ordered after this rollout (the second chunk stream
    // waited for it before its join into joined_to), so a consumer on that
    // stream need not wait; a consumer on any other stream (dbsde_set_stream
    // may have swapped it) waits for the ready mark
    bool joined = false;
    hipStream_t joined_to = nullptr;
    unsigned long long seq = 0;   // issue order: the older pending slot is the one replaced / reused
  } pend[2];
  unsigned long long pf_seq = 0;
  // a prefetch held back for the next chunked step, which runs the rollout on
  // its second stream after that stream's weight-gradient slices (the stream
  // finishes ahead of the main one); other steps issue it on pf_stream
  bool deferred = false;
  dbsde_batch defer_b{};
  hipStream_t pf_stream = nullptr;
  // forget every pending and held-back rollout (the caller has ordered its
  // stream after them: drop_all, or ensure_rows' host synchronisation)
  void clear() {
    pend[0].valid = pend[1].valid = false;
    deferred = false;
  }
};

struct dbsde_ctx {
  dbsde_config cfg{};
  std::string err;
  hipStream_t stream = nullptr;
  int device = 0;
  PathSched ps;
  hipEvent_t ev_pf_order = nullptr;
  hipEvent_t ev_switch = nullptr;   // dbsde_set_stream: the new stream after the old one
  // path-chunked phase pipeline: chunk i runs phase A then phase C on stream
  // (main, pipe2)[i % 2], so one chunk's phase C fills the other's phase-A tail.
  // The context creates only the streams it uses (pipe2, pf_stream): a process
  // gets GPU_MAX_HW_QUEUES (4) hardware queues, and streams beyond that share
  // one, where a stream's event wait also holds the other streams' work queued
  // behind it (the prefetch stream shared the second chunk's queue, so the
  // second chunk's phase A started after the prefetched rollout)
  hipStream_t pipe2 = nullptr;
  hipEvent_t ev_pipe[2] = {nullptr, nullptr};
  // the fork / join of the two chunk streams as stream memory operations
  // (a value written by one stream, waited for by the other) instead of
  // events, when the device supports them: per step 36 us less queue time in
  // the stream model of tools/ubench/stream_gaps.hip (events 467, no-fence
  // events 458, value write / wait 431 us per step)
  bool memops = false;
  unsigned long long* d_order = nullptr;   // [slot] = last epoch written (ORD_* slots)
  unsigned long long order_epoch[8] = {};
  hipEvent_t ev_prof[2] = {nullptr, nullptr};
  // 0 = by size: two chunks only when one phase launch has more workgroups
  // than the chip has slots (below that the chunks only serialize: A0, C0 || A1,
  // C1 is three workgroup lifetimes against A, C's two); DBSDE_CHUNKS=n forces n
  int chunks = 0;
  int cus = 256;   // compute units of the device
  int fv_slots[96] = {0};   // resident workgroups of the chip per phase variant (lazily queried)
  int fv_cs = -1;           // the column-split variant of fv (phasecs.hpp), or -1
  int cs_mode = 2;          // 0 off, 1 always, 2 by batch size

  // ---- network description
  int mode = 0, act = 0, K = 0, D = 0;
  int nb = 0;                 // Brownian dimension (D; D/2 for Heston, kind 1; D - 1 for Asian, kinds 4 and 8)
  bool asian = false;         // DBSDE_PROB_ASIAN: state [A, S_1..S_k], A the running average (nb = D - 1)
  bool geo = false;           // DBSDE_PROB_GEO_ASIAN: asian is set too, column 0 is the geometric average G
  bool barrier = false;       // DBSDE_PROB_BARRIER: DIAG's rollouts, then the stop pass (problem.h_kappa = B)
  int gcols = 0;              // state columns entering g and the terminal Z loss
  bool heston = false, u_clamp = false;
  bool heston2 = false;       // DBSDE_PROB_HESTON2: two Brownian motions per asset (nb = D)
  float rhob = 0.f;           // its fp32(sqrt(1 - (double)h_rho^2))
  float* Lt = nullptr;        // correlated device mode: L^T [nb][nb] (dbsde_set_corr)
  std::vector<int> L;
  bool has_v = false, proj = false;
  float rho = 0.f;
  Lin in, out;
  std::vector<Lin> B, V;  // B[j-1], V[j-1] for block j = 1..K
  long long nparams = 0;
  std::vector<unsigned char> used;

  // ---- padded geometry
  int Dp = 0, Stot = 0, Stot_x = 0, Wmax = 0;
  std::vector<int> Wp, col;  // per level j = 0..K

  // ---- weight buffers (fixed)
  float *BtIn = nullptr, *BtZ = nullptr, *wout = nullptr, *bout = nullptr;
  std::vector<float*> Bf, Bb, beta, rtr, abar;
  double* norms = nullptr;
  long long* d_woffs = nullptr;   // NAIS: W_j offsets in the flat params
  float** d_rtr = nullptr;
  float** d_abar = nullptr;
  float** d_wsnap = nullptr;      // NAIS: W_j as of rtr_params_kernel (read by the projection adjoint)
  double* proj_part = nullptr;
  double* dot_part = nullptr;     // <Abar_j, R_j> partials from the gradient finalize (one per 64 elements)
  int dot_nblk = 0;               // partials slots per block (stride)
  int dot_nused = 0;              // partials the finalize writes (tilefin: one per 256 tile elements)
  // hidden widths above NAIS_LMAX: the matrix-core projection kernels
  // (projw.hpp) with one reduced |R_j|_F^2 / <Abar_j, R_j> per block
  bool proj_wide = false;
  double* proj_sq = nullptr;      // [K] |R_j|_F^2
  float** d_sbuf = nullptr;       // S_j = Rbar_j + Rbar_j^T of the wide adjoint
  double* proj_dot = nullptr;     // [K] <Abar_j, R_j>
  unsigned char* d_used = nullptr;
  PackDesc* d_prep = nullptr;
  int n_prep = 0;
  // fused contexts: the BtZ packs the phase kernels' images stand in for, run
  // only where BtZ itself is read (dbsde_net_u_xvjp's input cotangent)
  PackDesc* d_prepz = nullptr;
  int n_prepz = 0, prepz_blocks = 1;
  // fused contexts: the fp32 BtIn / Bf copies the jet kernels read (jet.hpp),
  // packed only by dbsde_net_u_jet / dbsde_pde_residual
  PackDesc* d_prepj = nullptr;
  int n_prepj = 0, prepj_blocks = 1;
  // jet rows per launch and per direction workspace (0: the default; DBSDE_JET_CAP)
  long long jet_cap = 0;
  // dbsde_pde_residual workspace: u / Du of the points, one chunk's directions
  // and its (d1, d2)
  float *jet_u = nullptr, *jet_du = nullptr, *jet_V = nullptr, *jet_d = nullptr;
  size_t jet_u_cap = 0, jet_du_cap = 0, jet_V_cap = 0, jet_d_cap = 0;
  unsigned* jet_img = nullptr;   // the weights as split-bf16 fragments (jet.hip jet_split_kernel)
  size_t jet_img_cap = 0;

  int prep_blocks = 1;   // pack_tagged_kernel grid.x: one element per thread
  PackDesc* d_fin = nullptr;
  int n_fin = 0;
  TileFinTable* d_fintab = nullptr;   // tilefin_kernel: d_fin's windows grouped by problem tile
  std::vector<float*> slab;  // TN problem slabs (0 = x-stack, j = block j)
  std::vector<int> slab_mt, slab_nt, slab_mv, slab_nv;
  double* opt_part = nullptr;
  int opt_nparts = 0;
  double* vec_part = nullptr;     // L-BFGS reductions: VEC_RED_BLOCKS partials + the result

  // ---- row buffers (grow with Rp)
  int cap_rows = 0, cap_n = 0;
  float *xin = nullptr, *sdw = nullptr, *zbar = nullptr, *zfull = nullptr;
  float *Abuf = nullptr, *Adot = nullptr, *Delta = nullptr, *Alpha = nullptr, *H = nullptr, *Hdot = nullptr,
        *G = nullptr;
  float* Pbuf[2] = {nullptr, nullptr};
  float *u = nullptr, *rres = nullptr, *lossrow = nullptr, *ubar = nullptr, *q3S = nullptr, *umask = nullptr;
  float* dphidy = nullptr;               // [Rp] pen != 0, per-layer path: d phi / d Y of each interior row
  float *u16 = nullptr, *o16 = nullptr;  // [Rp,16]: col 0 = ubar / 1 (output-layer TN operands)
  double* loss_part = nullptr;
  float* loss_tmp = nullptr;

  std::vector<void*> allocs;      // fixed-size buffers
  std::vector<void*> row_allocs;  // buffers sized by the row count (regrown)

  float* rowsum = nullptr;        // [Rp, 8] residual row sums (fused path)
  bool fused = false;             // wave-level fused phase kernels usable for this net
  bool x3 = false;                // ... in their split-bf16 form (phase.hpp)
  int fv = -1;                    // the fused variant (kFused index) or -1
  bool x3chain = false;           // per-layer chain GEMMs in split-bf16 form (chainx3.hpp)
  bool tnx3 = false;              // the split-K weight-gradient tiles in split-bf16 form (tnx3.hpp; !tnw layouts)
  // fragment images (phase.hpp) of every operand matrix: X_j = [W_in|b] / [V_j|b_j+c_j]
  // (out W, in Dp), Z_j = its transpose (out Dp, in W), F_j = B_j, Bk_j = B_j^T
  std::vector<float*> imgX, imgZ, imgF, imgB;
  int tn_splits = 96;              // weight-gradient GEMM row splits (A/B: 64..128 best on MI355X): slab capacity
  int tn_splits_cur = 96;          // the splits of the last weight-gradient launch (<= tn_splits)
  // wave-owned weight-gradient tiles (tnw.hpp): NAIS layouts with Dp == Wp
  bool tnw = false;
  int tnw_nb = 0, tnw_P = 0, tnw_S = 128;  // P * S = 1024 waves = one per SIMD at K = 3
  int tnw_Smax = 128;                       // slab capacity; tnw_S is set per batch (loss_grad_impl)
  bool tnw_x3 = false;                     // split-bf16 weight-gradient kernel (tnwx3.hip)
  bool rollout2 = true;                    // two-pass device-mode diagonal rollout (paths.hpp)
  float* slabW = nullptr;
  int fin_blocks = 1;             // slabsum grid.x

  // ---- profiling
  bool prof = false;
  std::vector<ProfAgg> agg;
  std::map<std::string, int> agg_idx;
  std::vector<ProfRec> pending;
  std::vector<hipEvent_t> ev_pool;
};

// ---- net.hip
int fail(dbsde_ctx* c, int code, const std::string& msg);
int dalloc(dbsde_ctx* c, void** p, size_t bytes);
int ensure_rows(dbsde_ctx* c, int Rp, int N);
hipEvent_t get_event(dbsde_ctx* c);
int prof_id(dbsde_ctx* c, const std::string& name);
dbsde_ctx* free_call_ctx();   // the profiling store of dbsde_profile_*(NULL, ...)

#define HIPC(ctx, expr)                                                                        \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return fail(ctx, DBSDE_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
  } while (0)

template <typename T>
int dalloc_t(dbsde_ctx* c, T** p, size_t n) {
  return dalloc(c, (void**)p, n * sizeof(T));
}

// Cross-stream order points: order_mark(slot, from) marks `from`'s current
// queue position and returns its token; order_wait(slot, token, to) holds
// `to` until `from` has passed that mark.  A wait takes the token of a mark
// already enqueued, so it never lacks its write.  Slots: the chunk fork and
// join, the prefetch stream after the caller's stream and back, the two
// prefetch buffers' rollouts.
enum { ORD_FORK = 0, ORD_JOIN = 1, ORD_PF_AFTER_MAIN = 2, ORD_MAIN_AFTER_PF = 3, ORD_PEND0 = 4, ORD_SWITCH = 6 };
int order_mark(dbsde_ctx* c, int slot, hipStream_t from, unsigned long long& token);
int order_wait(dbsde_ctx* c, int slot, unsigned long long token, hipStream_t to);
// `to` waits until `from` has reached this point of its queue
int stream_order(dbsde_ctx* c, hipStream_t from, hipStream_t to, int slot);

// Launch wrapper: per-kernel HIP events, on the stream the launch goes to,
// when profiling is on.
template <typename F>
int run(dbsde_ctx* c, hipStream_t s, const char* name, double flops, double bytes, F&& launch) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (c->prof) {
    e0 = get_event(c);
    e1 = get_event(c);
    if (e0) (void)hipEventRecord(e0, s);
  }
  launch();
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, DBSDE_EHIP, std::string(name) + ": " + hipGetErrorString(e));
  if (c->prof && e0 && e1) {
    (void)hipEventRecord(e1, s);
    c->pending.push_back(ProfRec{prof_id(c, name), e0, e1, flops, bytes});
  }
  return DBSDE_OK;
}

#define RUN(ctx, s, name, fl, by, ...)                        \
  do {                                                        \
    int rc_ = run(ctx, s, name, fl, by, [&]() { __VA_ARGS__; }); \
    if (rc_) return rc_;                                      \
  } while (0)

// ---------------------------------------------------------------------------
// fused phase-kernel instantiations: (level tiles T, D tiles TD, blocks K)
struct FusedVariant {
  int T, TD, K, act, hv, x3;
  int rows;     // rows per workgroup: 64 (phase.hpp, or phase2 with one tile per wave) or 128 (phase2, two)
  int adot;     // phase C keeps adot_j in memory (phase2 ADOT)
  int xfirst;   // phase C image order: every x-stack image first (X0, X1..XK, F1..FK, B_K..B1)
  void (*A)(FusedArgs);
  void (*C)(FusedArgs);
};
// ---- step.hip (the unit that instantiates the phase kernels)
// (its table kFused stays internal to the unit: with external linkage the
// device pass would emit it too, kernel addresses and all)
const FusedVariant& fused_at(int fv);
int fused_variant(int T, int TD, int K, int act, bool hv, bool x3, bool cs = false);
int fill_col0(dbsde_ctx* c, float* buf, int ld, long long rows, float v);   // buf[r * ld] = v
// the fp32 weights the jet kernels read (jet.hip): full = the whole weight prep
// first (NAIS projection, every pack), else only what a prep already run left out
int jet_pack_weights(dbsde_ctx* c, const float* params, bool full);

// rows per 64-row phase-kernel workgroup (a multiple of the chain-GEMM tile,
// 64, and of the column-split workgroup, 16)
constexpr int ROW_PAD = P3_ROWS;
static_assert(ROW_PAD % CS_ROWS == 0, "row padding");
inline int pad_rows(int R) { return (R + ROW_PAD - 1) / ROW_PAD * ROW_PAD; }

// ---- rollout.hip: batches, path kernels and the path scheduler
int validate_batch(dbsde_ctx* c, const dbsde_batch* b);
int issue_rollout(dbsde_ctx* c, const dbsde_batch& b, int j, hipStream_t st, bool side);
int flush_deferred(dbsde_ctx* c, const float* avoid = nullptr, const dbsde_batch* only = nullptr);
int launch_deferred_on(dbsde_ctx* c, hipStream_t st);
int join_pending(dbsde_ctx* c, hipStream_t via, hipStream_t into);
int select_paths(dbsde_ctx* c, const dbsde_batch* b, bool& from_pf);
int q3_sum(dbsde_ctx* c, int M, int N);
