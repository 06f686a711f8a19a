// rollout.hip -- the X paths of a batch: the path kernels' dispatch
// (paths.hpp), the scheduler of the two path buffers and of the rollouts
// prefetched into them, and the C ABI that drives it (dbsde_prefetch*,
// dbsde_set_corr, dbsde_brownian).
// Correlated device mode: rollout_corr_kernel up to nb = 128 (L in registers),
// above it the increment GEMM rollout_corrw_kernel followed by the Euler chains.
// Correlated Heston (L between the k assets): the increment GEMM at every k,
// then rollout_heston_chain_kernel.
// Two-factor Heston (DBSDE_PROB_HESTON2): rollout_heston2_kernel for everything.
// Arithmetic average (DBSDE_PROB_ASIAN): rollout_asian_chain_kernel (behind the
// increment GEMM when a factor is set), then rollout_asian_avg_kernel.
// Geometric average (DBSDE_PROB_GEO_ASIAN): the same two launches, the second
// its geometric instance.
// Knock-out (DBSDE_PROB_BARRIER): DIAG's launches, then rollout_barrier_stop_kernel.
#include <hip/hip_runtime.h>

// a prefetched rollout runs on the next chunked step's second stream
#ifndef DBSDE_DEFER_PF
#define DBSDE_DEFER_PF 1
#endif
// device-mode diagonal rollout: in-step by default the two-pass form (parallel
// draws into the sdw rows, then the Euler chains: rollout_draw_kernel +
// rollout_chain_kernel, ctx rollout2; DBSDE_ROLLOUT2=0 turns it off: M = 128
// 0.146 vs 0.156 ms/step, profiles/r6_ab_rollout.txt 4); prefetched, and else,
// one thread per (path, column group) for all steps (rollout4_kernel).
#define DBSDE_DEVICE_HELPERS_ONLY
#include "ctx.hpp"
#include "paths.hpp"

int validate_batch(dbsde_ctx* c, const dbsde_batch* b) {
  if (!b) return fail(c, DBSDE_EINVAL, "batch is NULL");
  if (b->M < 1 || b->N < 1) return fail(c, DBSDE_EINVAL, "M and N must be >= 1");
  if ((long long)b->M * (b->N + 1) > (1LL << 30)) return fail(c, DBSDE_EINVAL, "M*(N+1) too large");
  if (!b->Xi) return fail(c, DBSDE_EINVAL, "Xi is NULL");
  if (b->xi_rows != 1 && b->xi_rows != b->M) return fail(c, DBSDE_EINVAL, "Xi must have 1 or M rows");
  if (b->W && !b->t) return fail(c, DBSDE_EINVAL, "t is required with W");
  if (b->path0 < 0 || b->path0 + b->M > (1LL << 32)) return fail(c, DBSDE_EINVAL, "path0 out of range");
  // the path kernels count (path, 16-byte column group) pairs in an int, and a
  // row buffer of Rp x max(Dp, Stot) floats must be addressable by the launch grids
  if ((long long)b->M * c->Dp > 0x7fffffffLL) return fail(c, DBSDE_EINVAL, "M * Dp too large");
  if ((long long)pad_rows(b->M * (b->N + 1)) * std::max(c->Dp, c->Stot) > (1LL << 38))
    return fail(c, DBSDE_EINVAL, "M*(N+1) rows of this width cannot be indexed");
  return DBSDE_OK;
}

// The increment pass of dbsde_mc_value's correlated Heston (mc.hip): the
// UNSCALED L z of samples [k0, k0 + count) as paths, ws [count, n_steps, k].
// T = N makes the kernel's own sqrtf(T / N) exactly 1; each point of the call
// applies its sqrt(dt_p) afterwards.  rollout_corrw_kernel counts (path, dim)
// in ints, so the samples go in slices of at most 2^31 / k (a multiple of
// CW_PATHS) per launch.  pc: the profiling store of the context-free calls.
int mc_corr_increments(dbsde_ctx* pc, hipStream_t s, const float* Lt, int k, int n_steps, unsigned long long seed,
                       unsigned long long offset, long long k0, long long count, float* ws) {
  if (k < 1 || k > CW_OB * 8 * 16 / 2 || n_steps < 1 || count < 1)
    return fail(pc, DBSDE_EINVAL, "internal: correlated Heston increment geometry");
  const long long slice = (0x7fffffffLL / k) / CW_PATHS * CW_PATHS;
  for (long long m0 = 0; m0 < count; m0 += slice) {
    RolloutArgs ra{};
    ra.M = (int)std::min(slice, count - m0);
    ra.N = n_steps;
    ra.D = 2 * k;
    ra.nb = k;
    ra.T = (float)n_steps;
    ra.seed = seed;
    ra.offset = offset;
    ra.path0 = k0 + m0;
    ra.Lt = Lt;
    ra.out = PATH_FETCH_DW;
    ra.W_out = ws + (size_t)m0 * n_steps * k;
    const dim3 g((ra.M + CW_PATHS - 1) / CW_PATHS, (n_steps + 3) / 4);
    const double steps = (double)ra.M * n_steps;
    RUN(pc, s, "corr_increments", 2.0 * steps * k * k / 2, 4.0 * steps * k,
        rollout_corrw_kernel<<<g, CW_THREADS, 0, s>>>(ra));
  }
  return DBSDE_OK;
}

namespace {

// batch b's paths into the rows of (xin, sdw)
RolloutArgs rollout_args(dbsde_ctx* c, const dbsde_batch* b, float* xin, float* sdw) {
  const dbsde_problem& pr = c->cfg.problem;
  RolloutArgs ra{};
  ra.M = b->M;
  ra.N = b->N;
  ra.D = c->D;
  ra.ldx = c->Dp;
  ra.nb = c->nb;
  ra.t = b->t;
  ra.W = b->W;
  ra.Xi = b->Xi;
  ra.xi_rows = b->xi_rows;
  ra.T = c->cfg.T;
  ra.seed = b->seed;
  ra.offset = b->offset;
  ra.path0 = b->path0;
  ra.mu_a = pr.mu_a;
  ra.sig_a = pr.sig_a;
  ra.sig_b = pr.sig_b;
  ra.kappa = pr.h_kappa;
  ra.theta = pr.h_theta;
  ra.hsig = pr.h_sigma;
  ra.rho = pr.h_rho;
  ra.rhob = c->rhob;
  ra.Lt = c->Lt;
  ra.xin = xin;
  ra.sdw = sdw;
  return ra;
}

// the correlated path kernel for ceil(nb / 16) output blocks
void launch_corr(const RolloutArgs& ra, hipStream_t s) {
  const dim3 g((ra.M + CP_PATHS - 1) / CP_PATHS);
  switch ((ra.nb + 15) / 16) {
    case 1: rollout_corr_kernel<1><<<g, CP_THREADS, 0, s>>>(ra); break;
    case 2: rollout_corr_kernel<2><<<g, CP_THREADS, 0, s>>>(ra); break;
    case 3: rollout_corr_kernel<3><<<g, CP_THREADS, 0, s>>>(ra); break;
    case 4: rollout_corr_kernel<4><<<g, CP_THREADS, 0, s>>>(ra); break;
    case 5: rollout_corr_kernel<5><<<g, CP_THREADS, 0, s>>>(ra); break;
    case 6: rollout_corr_kernel<6><<<g, CP_THREADS, 0, s>>>(ra); break;
    case 7: rollout_corr_kernel<7><<<g, CP_THREADS, 0, s>>>(ra); break;
    default: rollout_corr_kernel<8><<<g, CP_THREADS, 0, s>>>(ra); break;
  }
}

// workgroup size of rollout_heston_chain_kernel: HC_THREADS; DBSDE_HC_THREADS =
// 64 or 128 (read once) is the measurement switch of tools/heston_corr_profile.py
int heston_chain_threads() {
  static const int n = [] {
    const char* e = getenv("DBSDE_HC_THREADS");
    const int v = e ? atoi(e) : HC_THREADS;
    return v == 64 || v == 128 ? v : HC_THREADS;
  }();
  return n;
}

// workgroup size of rollout_heston2_kernel: H2_THREADS; DBSDE_H2_THREADS = 64 or
// 128 (read once) is the measurement switch of tools/heston2_profile.py
int heston2_threads() {
  static const int n = [] {
    const char* e = getenv("DBSDE_H2_THREADS");
    const int v = e ? atoi(e) : H2_THREADS;
    return v == 64 || v == 128 ? v : H2_THREADS;
  }();
  return n;
}

// Euler-Maruyama paths (ra.out == PATH_ROLLOUT) or the device fetch_minibatch
// (PATH_FETCH_*): Heston, Cholesky-correlated device mode, or diagonal
// side: a prefetched rollout running beside other work (the two-pass form's
// 1456-workgroup draw pass floods the CUs the phase section runs on: 0.451 vs
// 0.443 ms/step prefetched at M = 1024, so it serves in-step rollouts only)
int launch_paths(dbsde_ctx* c, RolloutArgs& ra, hipStream_t s, bool side = false) {
  const char* name = ra.out == PATH_ROLLOUT ? "rollout" : "brownian";
  const double steps = (double)ra.M * ra.N;
  const double bytes = ra.out == PATH_ROLLOUT ? 4.0 * steps * (2.0 * ra.D + (ra.W ? ra.nb : 0)) : 4.0 * steps * ra.nb;
  // the rollouts store whole float4 columns of the rows (ldx = Dp = pad16(D + 2))
  if (ra.ldx % 4 != 0) return fail(c, DBSDE_EINVAL, "internal: path row stride is not a multiple of 4 floats");
  if (c->asian) {
    // arithmetic-average problems (paths.hpp): the S chains -- behind the
    // increment GEMM when a factor is set -- then the averaging pass; one form
    // in-step and prefetched, on the device grid and on the caller's t / W
    const int k = ra.nb;
    if (k != ra.D - 1 || k < 1 || k > CW_OB * 8 * 16) return fail(c, DBSDE_EINVAL, "internal: Asian rollout geometry");
    const bool corr = c->Lt && !ra.W;
    const dim3 gw((ra.M + CW_PATHS - 1) / CW_PATHS, (ra.N + 3) / 4);
    const double fl = 2.0 * steps * k * k / 2;
    if (ra.out != PATH_ROLLOUT) {
      // the fetch is that of a diagonal problem with D = k
      if (corr) {
        RUN(c, s, "corr_increments", fl, 4.0 * steps * k, rollout_corrw_kernel<<<gw, CW_THREADS, 0, s>>>(ra));
        const long long nthr = (long long)ra.M * k;
        RUN(c, s, name, 0.0, bytes, corrw_fetch_kernel<<<(unsigned)((nthr + 255) / 256), 256, 0, s>>>(ra));
      } else {
        RolloutArgs fa = ra;
        fa.D = k;
        const int nthr = ra.M * k;
        RUN(c, s, name, 0.0, bytes, fetch_diag_kernel<<<(nthr + 255) / 256, 256, 0, s>>>(fa));
      }
      return DBSDE_OK;
    }
    const int chains = ra.M * (ra.ldx / 4);
    if (corr) {
      // coordinate i's increments into xin[row, 2 + i], the S_i column the chain then overwrites
      RolloutArgs ia = ra;
      ia.sdw = ra.xin + 1;
      RUN(c, s, "corr_increments", fl, 4.0 * steps * k, rollout_corrw_kernel<<<gw, CW_THREADS, 0, s>>>(ia));
      RUN(c, s, "asian_chain", 0.0, bytes + 4.0 * steps * k,
          rollout_asian_chain_kernel<true><<<(unsigned)((chains + RC_THREADS - 1) / RC_THREADS), RC_THREADS, 0, s>>>(ra));
    } else {
      RUN(c, s, "asian_chain", 0.0, bytes, rollout_asian_chain_kernel<false><<<(chains + 255) / 256, 256, 0, s>>>(ra));
    }
    // reads the k S columns and t of every row, writes the A column
    const int groups = ra.M * ASIAN_LANES;
    if (c->geo)
      RUN(c, s, "geo_asian_avg", 3.0 * steps * k, 4.0 * steps * (k + 2.0),
          rollout_asian_avg_kernel<true><<<(groups + AA_THREADS - 1) / AA_THREADS, AA_THREADS, 0, s>>>(ra));
    else
      RUN(c, s, "asian_avg", 3.0 * steps * k, 4.0 * steps * (k + 2.0),
          rollout_asian_avg_kernel<false><<<(groups + AA_THREADS - 1) / AA_THREADS, AA_THREADS, 0, s>>>(ra));
  } else if (c->heston2) {
    // two-factor Heston (never with a factor: dbsde_set_corr refuses it): one
    // kernel for device- and parity-mode batches, in-step and prefetched, and
    // for the fetch; thread per (path, asset)
    if (ra.nb != ra.D || (ra.D & 1)) return fail(c, DBSDE_EINVAL, "internal: two-factor Heston rollout geometry");
    const int nthr = ra.M * (ra.D / 2), ht = heston2_threads();
    RUN(c, s, name, 0.0, bytes, rollout_heston2_kernel<<<(nthr + ht - 1) / ht, ht, 0, s>>>(ra));
  } else if (c->Lt && !ra.W && (c->heston || ra.nb > CP_NBMAX)) {
    // wide correlated device mode, and correlated Heston at every k (paths.hpp):
    // the triangular GEMM dW = L (sqrt(dt) z) over (path group, step block),
    // then the Euler chains or the fetch sums
    if (ra.nb > CW_OB * 8 * 16 || ra.nb * (c->heston ? 2 : 1) != ra.D)
      return fail(c, DBSDE_EINVAL, "internal: wide correlated rollout geometry");
    const dim3 g((ra.M + CW_PATHS - 1) / CW_PATHS, (ra.N + 3) / 4);
    const double fl = 2.0 * steps * ra.nb * ra.nb / 2;
    RUN(c, s, "corr_increments", fl, 4.0 * steps * ra.nb, rollout_corrw_kernel<<<g, CW_THREADS, 0, s>>>(ra));
    if (ra.out == PATH_ROLLOUT && c->heston) {
      // reads the k increments, writes the 2k columns of xin and of sdw
      const int nthr = ra.M * ra.nb, hc = heston_chain_threads();
      const unsigned gb = (unsigned)((nthr + hc - 1) / hc);
      if (ra.t)
        RUN(c, s, name, 0.0, bytes + 4.0 * steps * ra.nb, rollout_heston_chain_kernel<true><<<gb, hc, 0, s>>>(ra));
      else
        RUN(c, s, name, 0.0, bytes + 4.0 * steps * ra.nb, rollout_heston_chain_kernel<false><<<gb, hc, 0, s>>>(ra));
    } else if (ra.out == PATH_ROLLOUT) {
      const int chains = ra.M * (ra.ldx / 4);
      const unsigned gb = (unsigned)((chains + RC_THREADS - 1) / RC_THREADS);
      if (ra.t)
        RUN(c, s, name, 0.0, bytes + 4.0 * steps * ra.D, rollout_chain_kernel<true><<<gb, RC_THREADS, 0, s>>>(ra));
      else
        RUN(c, s, name, 0.0, bytes + 4.0 * steps * ra.D, rollout_chain_kernel<false><<<gb, RC_THREADS, 0, s>>>(ra));
    } else {
      const long long nthr = (long long)ra.M * ra.nb;
      RUN(c, s, name, 0.0, bytes, corrw_fetch_kernel<<<(unsigned)((nthr + 255) / 256), 256, 0, s>>>(ra));
    }
  } else if (c->heston) {
    // parity-mode batches (the caller's W), and contexts without a factor
    const int nthr = ra.M * ra.nb;
    RUN(c, s, name, 0.0, bytes, rollout_heston_kernel<<<(nthr + 255) / 256, 256, 0, s>>>(ra));
  } else if (c->Lt && !ra.W) {
    if (ra.ldx > cp_srow((ra.nb + 15) / 16))
      return fail(c, DBSDE_EINVAL, "internal: correlated rollout row staging");
    RUN(c, s, name, 2.0 * steps * ra.nb * ra.nb / 2, bytes,
        launch_corr(ra, s));
  } else if (c->rollout2 && !side && ra.out == PATH_ROLLOUT && !ra.W && !ra.t) {
    // device-mode increments: parallel draws, then the Euler chains (paths.hpp)
    const long long draws = (long long)ra.M * ((ra.N + 3) / 4) * (ra.ldx / 4);
    const int chains = ra.M * (ra.ldx / 4);
    RUN(c, s, name, 0.0, bytes,
        rollout_draw_kernel<<<(unsigned)((draws + 255) / 256), 256, 0, s>>>(ra);
        rollout_chain_kernel<false><<<(unsigned)((chains + RC_THREADS - 1) / RC_THREADS), RC_THREADS, 0, s>>>(ra));
  } else if (ra.out == PATH_ROLLOUT) {
    const int nthr = ra.M * (ra.ldx / 4);
    RUN(c, s, name, 0.0, bytes, rollout4_kernel<<<(nthr + 255) / 256, 256, 0, s>>>(ra));
  } else {
    const int nthr = ra.M * ra.D;
    RUN(c, s, name, 0.0, bytes, fetch_diag_kernel<<<(nthr + 255) / 256, 256, 0, s>>>(ra));
  }
  if (c->barrier && ra.out == PATH_ROLLOUT) {
    // knock-out problems: the rows above are DIAG's, whichever form wrote them; the
    // stop pass (paths.hpp) follows on the same stream.  It reads the payoff's
    // columns of every row up to the hit and rewrites the rows behind it.
    const dbsde_problem& pr = c->cfg.problem;
    BarrierArgs ba{};
    ba.B = pr.h_kappa;
    ba.gsign = pr.g_kind >= DBSDE_G_PUT_SUM ? -1.f : 1.f;
    ba.cols = c->gcols;
    ba.mean = pr.g_kind == DBSDE_G_CALL_MEAN || pr.g_kind == DBSDE_G_PUT_MEAN;
    if (ba.cols < 1 || ba.cols > ra.D || c->asian || c->heston || c->heston2)
      return fail(c, DBSDE_EINVAL, "internal: barrier stop pass geometry");
    const long long groups = (long long)ra.M * ASIAN_LANES;
    RUN(c, s, "barrier_stop", 1.0 * ra.M * (ra.N + 1.0) * ba.cols, 4.0 * ra.M * (ra.N + 1.0) * ba.cols,
        rollout_barrier_stop_kernel<<<(unsigned)((groups + BS_THREADS - 1) / BS_THREADS), BS_THREADS, 0, s>>>(ra, ba));
  }
  return DBSDE_OK;
}

bool same_batch(const dbsde_batch& a, const dbsde_batch& b) {
  return a.M == b.M && a.N == b.N && a.t == b.t && a.W == b.W && a.seed == b.seed && a.offset == b.offset &&
         a.path0 == b.path0 && a.Xi == b.Xi && a.xi_rows == b.xi_rows;
}

// ---------------------------------------------------------------------------
// The path scheduler (c->ps): which of the two buffers a rollout goes to, and
// how a stream is ordered after the rollouts still pending in them
// ---------------------------------------------------------------------------

// a buffer no pending prefetch holds, else the older one's (reused or replaced
// once its rollout is done); never `avoid`
int pick_buffer(const dbsde_ctx* c, const float* avoid = nullptr) {
  const auto* p = c->ps.pend;
  int j = !p[0].valid ? 0 : (!p[1].valid ? 1 : (p[0].seq <= p[1].seq ? 0 : 1));
  if (avoid && c->ps.xin_b[j] == avoid) j = 1 - j;
  return j;
}

// order the context stream after pending rollout i: its ready mark, or, for a
// rollout joined into another stream (dbsde_set_stream changed it since), the
// latest chunk join (written on pipe2 after the rollout was ordered there)
int wait_pending(dbsde_ctx* c, int i) {
  const auto& p = c->ps.pend[i];
  if (!p.joined) return order_wait(c, ORD_PEND0 + i, p.ready_v, c->stream);
  if (p.joined_to == c->stream) return DBSDE_OK;
  return order_wait(c, ORD_JOIN, c->order_epoch[ORD_JOIN], c->stream);
}

// dbsde_prefetch's rollout on pf_stream, ordered after everything queued so
// far on the caller's stream (Xi ready, the buffer's previous readers done);
// work queued later overlaps it.  A replaced older rollout is earlier on the
// same stream.
int issue_prefetch(dbsde_ctx* c, const dbsde_batch& next, const float* avoid) {
  const int j = pick_buffer(c, avoid);
  const int rc = stream_order(c, c->stream, c->ps.pf_stream, ORD_PF_AFTER_MAIN);
  return rc ? rc : issue_rollout(c, next, j, c->ps.pf_stream, true);
}

// Forget every pending and held-back rollout.  The rollouts already issued
// still run to completion, so the context stream is ordered after each of
// them, whichever stream it runs on, and after pf_stream: what the stream does
// next may rewrite their buffers and what they read (Xi, the Cholesky factor).
int drop_all(dbsde_ctx* c) {
  int rc;
  for (int i = 0; i < 2; ++i)
    if (c->ps.pend[i].valid && (rc = wait_pending(c, i))) return rc;
  if (c->ps.pf_stream && (rc = stream_order(c, c->ps.pf_stream, c->stream, ORD_MAIN_AFTER_PF))) return rc;
  c->ps.clear();   // (a held-back prefetch has issued no work)
  return DBSDE_OK;
}

}  // namespace

// The one place a rollout is enqueued: batch b's paths into path buffer j on
// stream st, after the buffer's pad rows (past M (N + 1)) are cleared.
// side: a prefetch, running beside other work -- launch_paths takes the kernel
// form for that, and the rollout's ready mark and batch go into pend[j].
int issue_rollout(dbsde_ctx* c, const dbsde_batch& b, int j, hipStream_t st, bool side) {
  PathSched& ps = c->ps;
  const int R = b.M * (b.N + 1), Rp = pad_rows(R);
  float* xin = ps.xin_b[j];
  if (Rp > R) HIPC(c, hipMemsetAsync(xin + (size_t)R * c->Dp, 0, (size_t)(Rp - R) * c->Dp * 4, st));
  RolloutArgs ra = rollout_args(c, &b, xin, ps.sdw_b[j]);
  ra.out = PATH_ROLLOUT;
  int rc = launch_paths(c, ra, st, side);
  if (rc || !side) return rc;
  auto& p = ps.pend[j];
  if ((rc = order_mark(c, ORD_PEND0 + j, st, p.ready_v))) return rc;
  p.valid = true;
  p.joined = false;
  p.b = b;
  p.seq = ++ps.pf_seq;
  return DBSDE_OK;
}

// issue a held-back prefetch on pf_stream now; avoid = the path buffer of a
// step whose kernels are already queued (mid-step), which it must not
// overwrite; only = issue it only if it is this batch (its consumer has come)
int flush_deferred(dbsde_ctx* c, const float* avoid, const dbsde_batch* only) {
  PathSched& ps = c->ps;
  if (!ps.deferred || (only && !same_batch(ps.defer_b, *only))) return DBSDE_OK;
  ps.deferred = false;
  const dbsde_batch b = ps.defer_b;
  return issue_prefetch(c, b, avoid);
}

// the held-back prefetch on stream st (the chunked step's second stream, after
// its weight-gradient slices and its join into the main stream), into the path
// buffer the current step does not use: it runs beside the step's tail
// (finalize, projection adjoint, repack: a few latency-bound workgroups) and
// only the next step's phase A waits for it (its ready mark, wait_pending).
int launch_deferred_on(dbsde_ctx* c, hipStream_t st) {
  PathSched& ps = c->ps;
  if (!ps.deferred) return DBSDE_OK;
  const int j = pick_buffer(c, c->xin);
  // no free buffer: issue it on pf_stream, never into the buffer this step's
  // queued kernels read (the older pending buffer is replaced instead)
  if (ps.pend[j].valid) return flush_deferred(c, c->xin);
  ps.deferred = false;
  const dbsde_batch b = ps.defer_b;
  return issue_rollout(c, b, j, st, true);
}

// the pending rollouts are waited for on `via` (the second chunk stream, just
// before its join into `into`), so that join orders `into` after them too
int join_pending(dbsde_ctx* c, hipStream_t via, hipStream_t into) {
  for (int i = 0; i < 2; ++i) {
    auto& p = c->ps.pend[i];
    if (!p.valid) continue;
    // (a rollout joined before is already behind `via`)
    if (!p.joined) {
      const int rc = order_wait(c, ORD_PEND0 + i, p.ready_v, via);
      if (rc) return rc;
    }
    p.joined = true;
    p.joined_to = into;
  }
  return DBSDE_OK;
}

// Point c->xin / c->sdw at the path buffer this call uses.  A device-mode
// batch that dbsde_prefetch already rolled out takes that buffer (the main
// stream waits for the prefetch; from_pf = true); anything else takes a
// buffer no pending prefetch writes (both pending and neither is this batch:
// the older one's, once its rollout is done).
int select_paths(dbsde_ctx* c, const dbsde_batch* b, bool& from_pf) {
  PathSched& ps = c->ps;
  from_pf = false;
  int use = -1;
  if (b && !b->W)
    for (int i = 0; i < 2 && use < 0; ++i)
      if (ps.pend[i].valid && same_batch(ps.pend[i].b, *b)) {
        use = i;
        from_pf = true;
      }
  if (use < 0) use = pick_buffer(c);
  if (ps.pend[use].valid) {
    const int rc = wait_pending(c, use);
    if (rc) return rc;
  }
  ps.pend[use].valid = false;
  ps.cur = use;
  c->xin = ps.xin_b[use];
  c->sdw = ps.sdw_b[use];
  return DBSDE_OK;
}

// Q3's per-step sums of the current buffer's increments
int q3_sum(dbsde_ctx* c, int M, int N) {
  RUN(c, c->stream, "q3_sum", 0.0, 4.0 * M * N,
      q3_sum_kernel<<<N, 256, 0, c->stream>>>(c->sdw, c->Dp, M, N, c->q3S));
  return DBSDE_OK;
}

extern "C" {

int dbsde_brownian_dim(const dbsde_ctx* c) { return c ? c->nb : -1; }

int dbsde_set_corr(dbsde_ctx* c, const float* L, int n) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  if (c->heston2 && L)
    return fail(c, DBSDE_EINVAL,
                "dbsde_set_corr: the two-factor Heston problem takes no factor (correlation between assets is out "
                "of scope for it)");
  HIPC(c, hipSetDevice(c->device));
  // a prefetched rollout read the old factor: drop it and let it finish (the
  // host waits for pf_stream here, and below, before the factor changes, for
  // the context stream, which drop_all ordered after every other rollout)
  int rc = drop_all(c);
  if (rc) return rc;
  if (c->ps.pf_stream) HIPC(c, hipStreamSynchronize(c->ps.pf_stream));
  if (!L) {
    if (c->Lt) {
      HIPC(c, hipStreamSynchronize(c->stream));
      (void)hipFree(c->Lt);
      c->allocs.erase(std::find(c->allocs.begin(), c->allocs.end(), (void*)c->Lt));
      c->Lt = nullptr;
    }
    return DBSDE_OK;
  }
  // (Heston: nb = k = D / 2 <= 511, the assets' Brownian motions)
  if (n != c->nb) return fail(c, DBSDE_EINVAL, "dbsde_set_corr: L must be [nb, nb], nb = the Brownian dimension");
  std::vector<float> lt((size_t)n * n, 0.f);
  for (int d = 0; d < n; ++d)
    for (int k = 0; k <= d; ++k) lt[(size_t)k * n + d] = L[(size_t)d * n + k];   // L^T, lower part of L only
  if (!c->Lt && (rc = dalloc_t(c, &c->Lt, (size_t)n * n))) return rc;
  HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, hipMemcpy(c->Lt, lt.data(), lt.size() * sizeof(float), hipMemcpyHostToDevice));
  return DBSDE_OK;
}

int dbsde_prefetch(dbsde_ctx* c, const dbsde_batch* next) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  int rc = validate_batch(c, next);
  if (rc) return rc;
  if (next->W || next->t) return fail(c, DBSDE_EINVAL, "dbsde_prefetch: device-mode batches only (t and W NULL)");
  HIPC(c, hipSetDevice(c->device));
  if ((rc = ensure_rows(c, pad_rows(next->M * (next->N + 1)), next->N))) return rc;
  PathSched& ps = c->ps;
  for (int i = 0; i < 2; ++i)
    if (ps.pend[i].valid && same_batch(ps.pend[i].b, *next)) return DBSDE_OK;   // already queued
  if (ps.deferred && same_batch(ps.defer_b, *next)) return DBSDE_OK;
  if ((rc = flush_deferred(c))) return rc;
  if (DBSDE_DEFER_PF && c->pipe2) {
    ps.deferred = true;
    ps.defer_b = *next;
    return DBSDE_OK;
  }
  return issue_prefetch(c, *next, nullptr);
}

int dbsde_prefetch_cancel(dbsde_ctx* c) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  HIPC(c, hipSetDevice(c->device));
  return drop_all(c);
}

int dbsde_brownian(dbsde_ctx* c, const dbsde_batch* b, float* t, float* W, int increments) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  int rc = validate_batch(c, b);
  if (rc) return rc;
  if (b->W || b->t) return fail(c, DBSDE_EINVAL, "dbsde_brownian draws a device-mode batch (W and t must be NULL)");
  if (!t || !W) return fail(c, DBSDE_EINVAL, "t and W outputs are required");
  HIPC(c, hipSetDevice(c->device));
  RolloutArgs ra = rollout_args(c, b, c->xin, c->sdw);
  ra.out = increments ? PATH_FETCH_DW : PATH_FETCH_W;
  ra.t_out = t;
  ra.W_out = W;
  return launch_paths(c, ra, c->stream);
}

}  // extern "C"
