/*
 * dbsde.h -- C ABI of the MI355X-native deep-BSDE training step.
 *
 * This is the drop-in boundary for the reference's FBSNN solver surface
 * (nd_BSPDE_case.py:126-500, DeepBSDE.py:140-323, with_corr...py:132-540,
 * heston_dnnpde.py:519-699).  Every entry point below replaces one reference
 * method; the Python binding that a maintainer adds to a reference-style script
 * is the ctypes class in
 * deep-neural-network-solutions-for-partial-differential-equations_amd/fbsnn.py
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - Every function returns 0 on success and a negative DBSDE_E* code on
 *     failure; dbsde_last_error() then holds a message.
 *   - Pointers documented as "device" are HIP device pointers on the
 *     context's device (e.g. torch.Tensor.data_ptr() of a cuda tensor).
 *   - Parameters, gradients and optimizer moments are FLAT fp32 vectors in
 *     the reference module's state_dict() order (nd_BSPDE_case.py:445-456
 *     save format), so torch checkpoints interoperate.
 *   - Work is enqueued on the stream set by dbsde_set_stream (default: the
 *     legacy null stream) and is asynchronous: results are valid once the
 *     stream has been synchronised.  Setting a different stream orders it
 *     after the work already queued on the previous one (the context's
 *     workspace is shared by its calls), so a caller may switch streams
 *     between calls without synchronising.  The context keeps no caller pointer
 *     after a call returns.  A context is not thread safe.
 */
#ifndef DBSDE_H
#define DBSDE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DBSDE_ABI_VERSION 3

/* error codes */
#define DBSDE_OK 0
#define DBSDE_EINVAL -1   /* bad configuration or argument (Python: ValueError)   */
#define DBSDE_EHIP -2     /* HIP runtime failure             (Python: RuntimeError) */
#define DBSDE_ENOMEM -3   /* device allocation failed        (Python: MemoryError)  */

/* network modes: DeepBSDE.py:166-178, nd_BSPDE_case.py:159-172 */
#define DBSDE_MODE_FC 0        /* "FC"       nn.Sequential of Linear/act            */
#define DBSDE_MODE_NAIS_NET 1  /* "NAIS-Net" Resnet(stable=True), DeepBSDE.py:23-65 */
#define DBSDE_MODE_RESNET 2    /* "Resnet"   Resnet(stable=False)                   */
#define DBSDE_MODE_NAISNET 3   /* "Naisnet"  Functions/naisnet.py:6-96              */

/* activations: Functions/Sine.py, nn.ReLU, nn.Tanh (the reference's three);
   nn.SiLU and nn.Softplus (beta = 1, the smooth form at every argument: torch's
   switch to the identity above 20 changes less than fp32 resolves there) are
   the smooth non-saturating ones this library adds.  Any other value is
   DBSDE_EINVAL. */
#define DBSDE_ACT_SINE 0
#define DBSDE_ACT_RELU 1
#define DBSDE_ACT_TANH 2
#define DBSDE_ACT_SILU 3
#define DBSDE_ACT_SOFTPLUS 4

/* terminal conditions g(X) over the leading g_cols state columns */
#define DBSDE_G_SUMSQ 0       /* sum X^2                 DeepBSDE.py:333-335          */
#define DBSDE_G_CALL_SUM 1    /* max(sum X - K, 0)       nd_BSPDE_case.py:521-522     */
#define DBSDE_G_CALL_MEAN 2   /* max(mean X - K, 0)      with_corr...py:577-579,
                                                         heston_dnnpde.py:550 (k = 1)  */
#define DBSDE_G_LOG 3         /* log(1/2 + 1/2 sum X^2)  hjb_implement.py:597-598     */
#define DBSDE_G_SMOOTH_CALL 4 /* a / (1 + exp(-alpha a)), a = mean X - K
                                                         heston_dnnpde.py:551-556     */
/* the puts: the calls in -(. - K); dg/dX_col is -1 (-1/G) in the money, half of
   that at a tie (torch.maximum's split), 0 out of the money */
#define DBSDE_G_PUT_SUM 5     /* max(K - sum X, 0)                                    */
#define DBSDE_G_PUT_MEAN 6    /* max(K - mean X, 0)                                   */
#define DBSDE_G_SMOOTH_PUT 7  /* a / (1 + exp(-alpha a)), a = K - mean X              */

/* problem kinds */
#define DBSDE_PROB_DIAG 0     /* mu = mu_a X, sigma = diag(sig_a X + sig_b)          */
#define DBSDE_PROB_HESTON 1   /* k-asset Heston (heston_dnnpde.py:519-659), state
                                 [S_1..S_k, v_1..v_k], one Brownian motion per asset */
#define DBSDE_PROB_HESTON2 2  /* the two-factor (textbook) Heston model, the same state:
                                 Brownian motions W^S_i and W^v_i per asset, correlation
                                 h_rho between the two, none between assets            */
#define DBSDE_PROB_HESTON_CORR 3 /* dbsde_mc_value only: kind HESTON's process with the
                                 assets' Brownian motions correlated by its L argument,
                                 dW = sqrt(dt) (L z), L [k, k].  A context takes kind
                                 HESTON plus dbsde_set_corr instead                    */
/* kind 4.  Written as the successor of HESTON_CORR, not as a literal: the ABI tests pin the
   list of literal kind values of this header (tests/test_abi_mc_heston_corr.py), and
   tests/test_abi_asian.py holds the compiled value to 4 */
#define DBSDE_PROB_ASIAN (DBSDE_PROB_HESTON_CORR + 1)
                              /* arithmetic-average (Asian) option on k DIAG assets: state
                                 [A, S_1..S_k], A the running average of mean_i S_i, one
                                 Brownian motion per asset (nb = D - 1)                */
/* kind 8 (5, 6 and 7 are unknown kinds: tests/test_abi_asian.py), an expression for the
   same reason; tests/test_abi_geo_asian.py holds the compiled value to 8 */
#define DBSDE_PROB_GEO_ASIAN (DBSDE_PROB_ASIAN + 4)
                              /* geometric-average Asian option on k GBM assets: state
                                 [G, S_1..S_k], G = exp((1/T) int mean_i log S_i dt) the
                                 running geometric average (nb = D - 1)                */
/* kind 11 (9, 10 and 12 are unknown kinds), an expression for the same reason;
   tests/test_abi_barrier.py holds the compiled value to 11 */
#define DBSDE_PROB_BARRIER (DBSDE_PROB_GEO_ASIAN + 3)
                              /* knock-out (barrier) option on the DIAG process, monitored at
                                 the grid times: down-and-out for the call payoffs, up-and-out
                                 for the puts; state and Brownian dimension DIAG's (nb = D),
                                 h_kappa holds the barrier level B                      */

/*
 * Problem coefficients (one FBSNN subclass = one filled struct):
 *   kind DIAG:
 *     mu(X)    = mu_a * X                                (diagonal drift)
 *     sigma(X) = diag(sig_a * X + sig_b)                 (the reference's
 *                                                          dense diag_embed sigma)
 *   kind HESTON (heston_dnnpde.py:587-605), per asset i, sv = sqrt(max(v_i, 1e-8)):
 *     mu       = clamp([mu_a S_i, h_kappa (h_theta - v_i)], -100, 100)
 *     Sigma_i  = clamp([[sv S_i, h_rho h_sigma sv], [h_rho sv S_i, h_sigma sv]], -100, 100)
 *     driven by the asset's scalar dW_i (the reference's FBSNN dimension is 1;
 *     its einsum broadcasts dW over both state components)
 *   kind HESTON2, the same fields, state and D = 2k (even, else DBSDE_EINVAL), but
 *     the Brownian dimension is nb = D: column i of W is W^S_i, column k + i is
 *     W^v_i, all 2k independent.  Per asset, with sv = sqrt(max(v, 1e-8)),
 *     c(x) = clamp(x, -100, 100), rhob = fp32(sqrt(1 - (double)h_rho^2)) (host,
 *     once; |h_rho| <= 1) and every operation rounded to fp32 on its own, in
 *     this order (w1, w2 the increments of W^S_i and W^v_i):
 *       muS = c(mu_a S)            muV = c(h_kappa (h_theta - v))
 *       d00 = c(sv S)              d10 = c(h_rho (h_sigma sv))   d11 = c(rhob (h_sigma sv))
 *       S1  = (S + muS dt) + d00 w1
 *       v1  = (v + muV dt) + (d10 w1 + d11 w2)
 *       sigma dW (the Y-tilde term): S_i: d00 w1,  v_i: d10 w1 + d11 w2
 *     i.e. the PDE  u_t + mu_a S u_S + kappa (theta - v) u_v + 1/2 v S^2 u_SS
 *     + rho sigma v S u_Sv + 1/2 sigma^2 v u_vv - phi_r u = 0 per asset.
 *     dbsde_set_corr on such a context is DBSDE_EINVAL (no correlation between
 *     assets), dbsde_mc_value takes neither L nor delta for it, and
 *     DBSDE_EXACT_HESTON / DBSDE_EXACT_HESTON_PUT are its closed forms for k = 1
 *     and a call / put payoff.
 *   kind HESTON_CORR: HESTON's fields, state and step, for dbsde_mc_value alone (the
 *     factor is that call's L argument); dbsde_create refuses it.
 *   kind ASIAN, the same struct: state [A, S_1..S_k], D = k + 1 >= 2 (else
 *     DBSDE_EINVAL), Brownian dimension nb = k = D - 1 (column i of W drives S_i;
 *     A has no diffusion).  Each S_i is the DIAG process with mu_a, sig_a, sig_b,
 *     its increment dW_i the Philox coordinate i of the diagonal rollout's key (or
 *     the caller's W [M, N+1, k], or with dbsde_set_corr (n = k) dW = L (sqrt(dt) z)).
 *     A is the running average of the row mean by the left-point rule, every
 *     operation rounded to fp32 on its own, in this order:
 *       s_i  = (sig_a S_i + sig_b) dW_i           S_i' = (S_i + (mu_a S_i) dt) + s_i
 *       p_l  = ((0 + S_l) + S_{l+16}) + ...       l = 0..15, ascending over the assets
 *       p_l <- p_l + p_{l xor o}                  o = 1, 2, 4, 8 in turn: sum = p_0
 *       m    = sum / (float)k                     (S at the row's own time t_n)
 *       A'   = A + (m dt) / T                     so A_N = A_0 + (1/T) sum_{n<N} m_n dt_n
 *     sigma dW (the Y-tilde term): A: exactly 0, S_i: s_i.  The PDE is
 *       u_t + (mean S / T) u_A + sum_i mu_a S_i u_{S_i} + 1/2 tr(sigma sigma^T D^2_S u) - phi = 0,
 *       u(T, .) = g(A).
 *     The payoff is on A alone: g_cols must be 1 and g_kind one of CALL_SUM,
 *     CALL_MEAN, SMOOTH_CALL, PUT_SUM, PUT_MEAN, SMOOTH_PUT (SUMSQ and LOG are
 *     DBSDE_EINVAL); phi_c must be 0 (X.Z would include A u_A); q3 is ignored.
 *     dbsde_pde_residual takes nd = 1 + k directions (A component 0) and the
 *     drift above; dbsde_mc_value simulates the same process (below).
 *   kind GEO_ASIAN, the same struct: state [G, S_1..S_k], D = k + 1 >= 2, nb = k, ASIAN's
 *     S columns, increments, factor (dbsde_set_corr, L [k, k]) and refusals, and sig_b
 *     must be 0 (DBSDE_EINVAL: the assets must stay positive, and the closed form
 *     DBSDE_EXACT_GEO_ASIAN is GBM's).  G has no diffusion, dG = G (mean_i log S_i / T) dt,
 *     G_0 = 1 for an option written at t = 0.  The scheme carries a = log G through
 *     ASIAN's averaging on lg(S), every operation rounded to fp32 on its own unless cast:
 *       lg_i = (float)log((double)fmaxf(S_i, FLT_MIN))   (one definition, host and device)
 *       p_l, butterfly, m = sum / (float)k               ASIAN's order, on lg
 *       a'   = a + (m dt) / T                            a_0 = lg(G_0) (exactly 0 for G_0 = 1)
 *       row 0 stores G_0 as given; row n >= 1 stores G_n = (float)exp((double)a_n)
 *     so G_N = G_0 exp((1/T) sum_n m_n dt_n).  sigma dW: G: exactly 0, S_i: (sig_a S_i) dW_i.
 *     The PDE is
 *       u_t + G (mean log S / T) u_G + sum_i mu_a S_i u_{S_i} + 1/2 tr(sigma sigma^T D^2_S u) - phi = 0,
 *       u(T, .) = g(G),
 *     g_cols = 1.  dbsde_pde_residual takes ASIAN's directions (G component 0) and this
 *     drift (logf of the S columns); dbsde_mc_value simulates the same process (below).
 *   kind BARRIER, the same struct: DIAG's state, coefficients, Brownian dimension nb = D and
 *     factor (dbsde_set_corr), with a knock-out barrier monitored at the grid times t_0..t_N
 *     and no rebate.  kind BARRIER: h_kappa is the barrier level B (the Heston members are
 *     unused by every non-Heston kind; h_theta, h_sigma and h_rho must be 0).  The monitored
 *     statistic is the payoff's own over its g_cols columns, every comparison in fp32:
 *       p_l, butterfly                     ASIAN's row-sum order over columns 1..g_cols
 *       stat = sum                         (CALL_SUM / PUT_SUM)
 *       stat = sum / (float)g_cols         (CALL_MEAN / PUT_MEAN)
 *       call: knocked at the first row n with stat_n <= B (down-and-out; row 0 counts)
 *       put:  knocked at the first row n with stat_n >= B (up-and-out)
 *     Only the regular barriers: B <= strike for a call, B >= strike for a put, so g is 0
 *     with gradient 0 on a knocked state.  Training runs on the stopped process X_{t ^ tau}:
 *     rows n <= tau are the unstopped path's, rows n > tau hold X_tau, sdw rows n >= tau are
 *     0, t keeps running (the stop pass follows every rollout form; dbsde_brownian still
 *     returns the unstopped Brownian path).  On the frozen rows the BSDE residual is
 *     u(t_{n+1}, x) - u(t_n, x) - phi dt with terminal value g(x) = 0: u = 0, Du = 0, the
 *     Dirichlet condition (a non-zero rebate would not be consistent with a
 *     discounting driver on the frozen rows).  DBSDE_EINVAL from dbsde_create and
 *     dbsde_mc_value, before any HIP call and naming the field: h_kappa <= 0, NaN or
 *     infinite; a call with h_kappa > strike or a put with h_kappa < strike; g_kind SUMSQ,
 *     LOG, SMOOTH_CALL or SMOOTH_PUT; pen != 0, q3, u_clamp; h_theta, h_sigma or h_rho != 0.
 *     dbsde_pde_residual takes DIAG's terms: the generators of the stopped and the unstopped
 *     process agree on the live side of the barrier, and the residual means nothing beyond
 *     it.  dbsde_mc_value simulates the knocked-out payoff (below).
 *   phi      =phi_r * (Y - phi_c * X.Z) + phi_zz * |Z|^2
 *   g        = g_kind over the first g_cols state columns (0 = all), strike,
 *              g_alpha (DBSDE_G_SMOOTH_CALL / _PUT); the terminal |Z - grad g|^2 term
 *              runs over the same columns (heston_dnnpde.py:654: dU/dS only)
 *   u_clamp  = 1: u = max(net(t, X), 0) (heston_dnnpde.py:568)
 *   q3       = 1: for D == 1 reproduce the reference's squeeze() broadcast in
 *              the Y-tilde term (1d_BSPDE_case.py:271-273)
 *   pen      = lambda >= 0, the penalty of the penalised American problem
 *                u_t + mu.Du + 1/2 tr(sigma sigma^T D^2 u) - phi_lin + pen (g(x) - u)^+ = 0,  u(T, .) = g:
 *              the driver becomes  phi = phi_r (Y - phi_c X.Z) + phi_zz |Z|^2 - pen max(g(X) - Y, 0)
 *              with g the terminal condition on the row's own X (the same g_kind, strike,
 *              g_alpha and g_cols), d phi / d Y = phi_r + pen 1[g(X) > Y] (strict: 0 at a
 *              tie) and d phi / d Z unchanged.  pen == 0 is the problem without the field,
 *              bit for bit.  pen != 0 is taken for kind DIAG only (with or without
 *              dbsde_set_corr, any g_kind, q3 allowed); DBSDE_EINVAL from dbsde_create,
 *              before any HIP call and with a message naming pen, for pen < 0, NaN or
 *              infinite, pen != 0 on a Heston, Asian or geometric-Asian kind, and pen != 0
 *              with u_clamp.  dbsde_pde_residual's phi and residual are the penalised
 *              PDE's; dbsde_mc_value refuses pen != 0 (the problem is not linear: its
 *              arbiter is DBSDE_EXACT_AMERICAN_PUT).  The last member: a caller filling
 *              the 17 members before it and zeroing the struct keeps today's problem.
 *              That holds at the source level only.  dbsde_config embeds dbsde_problem
 *              by value, so the member moved T and device by four bytes while
 *              DBSDE_ABI_VERSION stayed 3: a binary compiled against the header without
 *              pen passes a shifted T with no version signal and must be recompiled.
 */
typedef struct dbsde_problem {
  int kind;
  float mu_a, sig_a, sig_b;
  float phi_r, phi_c, phi_zz;
  int g_kind;
  float strike;
  int q3;
  int g_cols;
  float g_alpha;
  int u_clamp;
  float h_kappa, h_theta, h_sigma, h_rho;
  float pen;
} dbsde_problem;

typedef struct dbsde_config {
  int mode;          /* DBSDE_MODE_*                                   */
  int activation;    /* DBSDE_ACT_*                                    */
  int n_layers;      /* len(layers), 4..9                              */
  int layers[16];    /* [D+1, W1, ..., Wk, 1]; D <= 1022 (the padded   */
                     /* row pad16(D + 2) <= 1024), else DBSDE_EINVAL;  */
                     /* NAIS_NET / NAISNET: the (equal) hidden widths  */
                     /* W1 = .. = Wk <= 1024, else DBSDE_EINVAL        */
  dbsde_problem problem;
  float T;           /* terminal time                                  */
  int device;        /* HIP device ordinal                             */
} dbsde_config;

typedef struct dbsde_ctx dbsde_ctx;

/* FBSNN.__init__ (network/problem construction; weights are caller-owned) */
int dbsde_create(const dbsde_config* cfg, dbsde_ctx** out);
void dbsde_destroy(dbsde_ctx* ctx);
const char* dbsde_last_error(const dbsde_ctx* ctx); /* ctx may be NULL */
int dbsde_abi_version(void);
int dbsde_set_stream(dbsde_ctx* ctx, void* hip_stream);

/* No reference counterpart (the reference has one stream).  The context
 * orders its internal streams with stream value operations (a wait spins
 * until the writer's queue has run the write); under anything that runs one
 * kernel at a time that wait would never end, so a context created in such an
 * environment orders them with events.  Returns 1 when the current process
 * environment selects events: DBSDE_STREAM_ORDER=events, AMD_SERIALIZE_KERNEL,
 * HIP_LAUNCH_BLOCKING, ROCPROF_COUNTER_COLLECTION, ROCPROF_COUNTERS,
 * HSA_TOOLS_LIB, an LD_PRELOAD naming rocprof, or any ROCPROFILER_* / ROCP_*
 * variable (DBSDE_STREAM_ORDER=values overrides all of them); 0 otherwise.
 * env: a NULL-terminated "NAME=VALUE" block to evaluate instead of the
 * process environment (NULL = the process environment).  The first context
 * of a process names its choice on stderr (DBSDE_QUIET=1 silences it).  Any
 * other serialising tool needs DBSDE_STREAM_ORDER=events. */
int dbsde_stream_order_by_events(const char* const* env);

/* size of the flat parameter vector = sum of state_dict numels */
long long dbsde_param_count(const dbsde_ctx* ctx);
/* host mask[i] = 1 if parameter element i receives a gradient (SURVEY Q6:
 * Resnet(stable) input_layers[-1] is never used and stays grad=None) */
int dbsde_param_used_mask(const dbsde_ctx* ctx, unsigned char* mask, long long n);

/* matrix-core form of this network's kernels (no reference counterpart:
 * reporting only).  Bit 0: the fused phase kernels, bit 1: the weight-gradient
 * kernel (wave-owned tiles, or the chain layouts' 128x128 tiles), bit 2: the
 * per-layer chain GEMMs (FC / Resnet layouts without a
 * fused variant) run fp32 operands as exact split-bf16 triples (six bf16 MFMAs
 * per product block, fp32 accumulation, error at or below the fp32-input
 * MFMA's); 0 = fp32-input MFMA (v_mfma_f32_16x16x4_f32) throughout.  Set at
 * create time (DBSDE_X3=0 / DBSDE_TNW_X3=0 select the fp32 forms). */
int dbsde_matrix_form(const dbsde_ctx* ctx);

/* Brownian dimension nb of a batch's W [M, N+1, nb]: D (DIAG, HESTON2, BARRIER), D/2 for HESTON,
   D - 1 for ASIAN and GEO_ASIAN */
int dbsde_brownian_dim(const dbsde_ctx* ctx);

/*
 * Cholesky factor of the increments' correlation matrix for the DEVICE mode
 * (with_corr_high_dimension_pde.py:339-341: dW = L (sqrt(dt) z)).  L is a host
 * [n, n] row-major lower-triangular fp32 matrix, n = dbsde_brownian_dim <= 1022;
 * the context keeps a device copy (n <= 128: held in registers by the path
 * kernel; above: streamed by the triangular increment GEMM).  L ==
 * NULL clears it.  Parity-mode batches (W != NULL) already carry correlated W
 * and ignore L.
 * Heston contexts: n = dbsde_brownian_dim = k = D / 2 <= 511 and L correlates
 * the k assets' Brownian motions (each still drives its own S_i and v_i).  The
 * device-mode rollout, dbsde_prefetch, dbsde_brownian and the rank shards
 * (path0) then run on dW = L (sqrt(dt) z) -- the increment GEMM at every k,
 * followed by a per-(path, asset) Euler chain -- and dbsde_pde_residual takes
 * the columns of Sigma(x) . L.  dbsde_mc_value simulates the same process when it
 * is given the factor with kind DBSDE_PROB_HESTON_CORR (kind HESTON with L stays
 * DBSDE_EINVAL there).
 * HESTON2 contexts: DBSDE_EINVAL (correlation between assets is out of scope
 * for the two-factor model; L == NULL is accepted and does nothing).
 * Any other n is DBSDE_EINVAL.
 */
int dbsde_set_corr(dbsde_ctx* ctx, const float* L, int n);

/*
 * One minibatch (FBSNN.fetch_minibatch output, DeepBSDE.py:247-262).
 *   W != NULL : parity mode, t [M,N+1] and W [M,N+1,nb] device fp32 exactly as
 *               the reference builds them (cumsum in fp64, cast).
 *   W == NULL : device mode, Brownian increments sqrt(dt)*N(0,1) drawn by an
 *               in-kernel Philox4x32-10 keyed by (seed, offset, global path,
 *               step, Brownian coordinate), correlated by L when set;
 *               t == NULL means the reference's grid fp32(cumsum_fp64(T/N)).
 *               A rank holding paths [path0, path0+M) of a larger batch draws
 *               exactly the increments a single device would draw for them.
 *   Xi         : device [xi_rows, D] initial state (Heston: [S_1..S_k, v_1..v_k]).
 */
typedef struct dbsde_batch {
  int M, N;
  const float* t;
  const float* W;
  unsigned long long seed, offset;
  long long path0;   /* global index of local path 0 (Philox stream of a rank's shard) */
  const float* Xi;   /* device [xi_rows, D], xi_rows in {1, M} */
  int xi_rows;
} dbsde_batch;

typedef struct dbsde_outputs {
  float* loss;   /* device scalar, nullable        */
  float* X;      /* device [M, N+1, D], nullable   */
  float* Y;      /* device [M, N+1], nullable      */
  float* Z;      /* device [M, N+1, D], nullable   */
} dbsde_outputs;

/*
 * Device FBSNN.fetch_minibatch (DeepBSDE.py:247-262, with_corr...py:316-353)
 * for a device-mode batch (batch->W must be NULL, batch->t NULL): writes t
 * [M, N+1] and, with increments == 0, W [M, N+1, nb] = fp32(fp64 cumsum of dW)
 * (the reference's layout), or with increments == 1 the raw dW
 * [M, N, nb] the device-mode rollout consumes (correlated when
 * dbsde_set_corr was called).
 */
int dbsde_brownian(dbsde_ctx* ctx, const dbsde_batch* batch, float* t, float* W, int increments);

/*
 * Roll out a device-mode batch ahead of the dbsde_loss_grad that consumes it
 * (the reference's next fetch_minibatch, DeepBSDE.py:247-262, drawn while the
 * current iteration runs: train() draws each iteration's batch independently
 * of the model, nd_BSPDE_case.py:371).  The batch is held back for the next
 * dbsde_loss_grad / dbsde_train_step: if that step runs the two-stream phase
 * pipeline, the rollout runs on its second stream after its weight-gradient
 * work, ordered before the following step; otherwise (or at any other call
 * that selects path buffers) it is issued then on an internal stream ordered
 * after the work queued on the context's stream, and work queued later
 * overlaps it.  A later
 * dbsde_loss_grad whose batch descriptor is identical (M, N, seed, offset,
 * path0, Xi pointer and rows; t = W = NULL) uses the prefetched paths instead
 * of rolling out; any other batch rolls out as usual.  At most two batches
 * are pending.  Xi is read when the rollout runs: it must not change after
 * this call until the batch is consumed or cancelled.  dbsde_set_corr drops
 * pending prefetches.
 */
int dbsde_prefetch(dbsde_ctx* ctx, const dbsde_batch* next);
/* Forget every pending prefetch (e.g. the caller is about to rewrite the Xi
 * buffer a prefetch read); later batches roll out as usual.  The context stream
 * is ordered after the pending rollouts, so their buffers are reused safely. */
int dbsde_prefetch_cancel(dbsde_ctx* ctx);

/*
 * FBSNN.loss_function + loss.backward (DeepBSDE.py:202-245, 279).
 * grad (device, flat, param_count) receives d loss / d params (overwritten,
 * 0 for unused parameters); grad == NULL runs the forward only (predict,
 * nd_BSPDE_case.py:412-443).
 */
int dbsde_loss_grad(dbsde_ctx* ctx, const float* params, const dbsde_batch* batch,
                    float* grad, const dbsde_outputs* out);

/* FBSNN.net_u (DeepBSDE.py:189-194): u [R] and Du [R,D] at R points
 * (Heston: the clamped u and its masked gradient, heston_dnnpde.py:560-579). */
int dbsde_net_u(dbsde_ctx* ctx, const float* params, int R, const float* t,
                const float* X, float* u, float* Du);

/* The vector-Jacobian product of net_u: the gradient the reference's autograd
 * graph of (u, Du) delivers (nd_BSPDE_case.py:191-221, create_graph=True),
 *   grad = d/dparams [ sum_r ubar[r] u[r] + sum_{r,d} zbar[r,d] Du[r,d] ]
 * at the R points (t [R], X [R,D]); ubar [R], zbar [R,D], grad (flat,
 * param_count) are device buffers (grad overwritten).  The gradient with
 * respect to X is dbsde_net_u_xvjp's. */
int dbsde_net_u_vjp(dbsde_ctx* ctx, const float* params, int R, const float* t,
                    const float* X, const float* ubar, const float* zbar, float* grad);

/* The same backward with the input cotangent (net_u differentiated in the
 * points: the reference's jacobian(net_u, S) and its Greeks,
 * with_corr_high_dimension_pde.py:856-877, heston_dnnpde.py:685-699):
 *   xbar[r, :] = d/dX_r [ ubar[r] u[r] + zbar[r, :] . Du[r, :] ]
 *              = ubar[r] Du[r, :] + H_r zbar[r, :],   H_r = the Hessian of u in X at row r
 * (Heston: through the u clamp, so 0 on the clamped rows).  xbar [R, D] device,
 * overwritten.  grad and xbar are each optional (NULL: not computed; with grad
 * NULL the weight-gradient work is skipped where it is a separate launch);
 * both NULL is DBSDE_EINVAL.  grad is filled exactly as dbsde_net_u_vjp fills
 * it.  t is not differentiated.  The result is bitwise repeatable. */
int dbsde_net_u_xvjp(dbsde_ctx* ctx, const float* params, int R, const float* t,
                     const float* X, const float* ubar, const float* zbar, float* grad,
                     float* xbar);

/* First and second directional derivatives of the network in its inputs z = (t, x):
 *   d1[r, j] = grad_z net(z_r) . v_rj,   d2[r, j] = v_rj^T hess_z net(z_r) v_rj
 * V device [R, nd, D+1] (column 0 = the t component), d1 / d2 device [R, nd], each nullable
 * (both NULL: EINVAL).  u_clamp contexts (Heston): the jets of u = max(net, 0), i.e. 0 on the
 * rows dbsde_net_u masks.  Bitwise repeatable.  t is differentiated here (direction e_t gives
 * theta = u_t, which dbsde_net_u / dbsde_net_u_xvjp do not).  Forward (Taylor-mode)
 * propagation in split-bf16 matrix products with fp32 accumulation; nothing is stored per
 * (point, direction) row, and rows are launched DBSDE_JET_CAP (default 65536, read at
 * dbsde_create) at a time.  Hidden widths above 256 are not supported (EINVAL).  A wave
 * stages 16 (Dp + 4 + 2 ldw) floats of LDS (97 KB at D = 1022, width 256); a combination
 * above the CU's 160 KB is EINVAL. */
int dbsde_net_u_jet(dbsde_ctx* ctx, const float* params, int R, const float* t, const float* X,
                    int nd, const float* V, float* d1, float* d2);

/* The terms of the PDE the context's problem solves,
 *   u_t + mu . Du + 1/2 tr(sigma sigma^T D^2 u) - phi(x, u, Du) = 0,
 * at R points: device [R] each, each nullable (all NULL: EINVAL).
 *   u, u_t     the network value (dbsde_net_u) and its t derivative (jet direction e_t)
 *   drift      mu . Du: DIAG mu_a X . Du; Heston its clamped drift
 *   diffusion  1/2 sum_j a_j^T D^2u a_j over the columns a_j of the diffusion matrix: DIAG
 *              diag(sig_a X + sig_b) . L (L: dbsde_set_corr, else I); Heston Sigma_i . (1, 1)^T
 *              per asset in its (S_i, v_i) plane, with the rollout's sqrt(max(v, 1e-8)) and
 *              +-100 clamps; with a factor between the assets (dbsde_set_corr, L [k, k])
 *              column j of Sigma(x) . L: those entries of every asset i >= j times L[i][j];
 *              HESTON2 its 2k columns: dW^S_i -> (S_i: d00, v_i: d10), dW^v_i -> (v_i: d11);
 *              ASIAN (drift: mu_a S_i on the S columns, mean S / T on A) the k columns of
 *              diag(sig_a S + sig_b) . L in the S columns, A component 0
 *   phi        phi_r (u - phi_c X . Du) + phi_zz |Du|^2   (q3 is ignored)
 *   residual   u_t + drift + diffusion - phi
 *   scale      |u_t| + |drift| + 1/2 sum_j |a_j^T D^2u a_j| + |phi|: what the residual is
 *              read against, so that cancellation in the trace does not hide it
 * Points are processed in chunks of at most DBSDE_JET_CAP (point, direction) rows. */
typedef struct dbsde_pde_terms {
  float *u, *u_t, *drift, *diffusion, *phi, *residual, *scale;
} dbsde_pde_terms;
int dbsde_pde_residual(dbsde_ctx* ctx, const float* params, int R, const float* t, const float* X,
                       const dbsde_pde_terms* out);

/* optimizers (nd_BSPDE_case.py:331-350), torch.optim single-tensor formula order */
#define DBSDE_OPT_ADAM 0
#define DBSDE_OPT_ADAMW 1
#define DBSDE_OPT_SGD 2
#define DBSDE_OPT_RMSPROP 3   /* state: v = square_avg                 */
#define DBSDE_OPT_ADAGRAD 4   /* state: v = state_sum                  */
#define DBSDE_OPT_ADAMAX 5    /* state: m = exp_avg, v = exp_inf       */
#define DBSDE_OPT_ADADELTA 6  /* state: v = square_avg, m = acc_delta  */
#define DBSDE_OPT_ASGD 7      /* state: m = ax (averaged parameters)   */

typedef struct dbsde_optim {
  int kind;
  float lr, beta1, beta2, eps, weight_decay;
  float max_norm;    /* clip_grad_norm_(max_norm) before the step; <= 0: no clip */
  long long step;    /* 1-based step count of THIS update (bias correction) */
  float alpha;       /* RMSprop smoothing constant (torch default 0.99) */
  float rho;         /* Adadelta rho (0.9) */
  float lr_decay;    /* Adagrad lr_decay (0) */
  float lambd;       /* ASGD lambd (1e-4) */
  float asgd_eta;    /* ASGD eta and mu of THIS step: torch keeps them as fp32 */
  float asgd_mu;     /* state; the caller runs that recursion                   */
  const float* loss; /* nullable device scalar: skip the update when it is not
                        finite (heston_dnnpde.py:409-411 NaN skip)              */
  /* nullable device double[2]: the optimizer's step count kept on the device,
     so that a skipped update does not advance it (the reference `continue`s
     before optimizer.step(), heston_dnnpde.py:409-411).  When set, the update
     reads the completed step count from step_state[step_parity], runs update
     number count + 1 (bias corrections, Adagrad's clr, ASGD's eta / mu derived
     on the device from it; `step`, asgd_eta and asgd_mu are ignored) and writes
     the new count -- the old one when skipped -- to step_state[1 - step_parity].
     Successive calls alternate step_parity. */
  double* step_state;
  int step_parity;
} dbsde_optim;

/* clip_grad_norm_ + optimizer.step() (nd_BSPDE_case.py:383-384); m, v device
 * flat state owned by the caller (zero-initialised for a fresh optimizer). */
int dbsde_optimizer_step(dbsde_ctx* ctx, float* params, float* grad, float* m, float* v,
                         const dbsde_optim* opt);

/*
 * One training iteration of one process: dbsde_loss_grad followed by
 * dbsde_optimizer_step (nd_BSPDE_case.py:376-384: loss.backward(),
 * clip_grad_norm_, optimizer.step()).  When the update needs nothing but each
 * element's own gradient -- no clipping (max_norm <= 0), no NaN skip (loss ==
 * NULL) and a device step counter (step_state) -- it is applied inside the
 * gradient finalize kernels, element by element as each gradient is formed
 * (one launch fewer per step; grad is still written).  Otherwise the two calls
 * run in sequence.  Data-parallel callers, whose all-reduce sits between the
 * gradient and the update, use the two calls instead.
 */
int dbsde_train_step(dbsde_ctx* ctx, float* params, const dbsde_batch* batch, float* grad, float* m, float* v,
                     const dbsde_optim* opt, const dbsde_outputs* out);

/*
 * L-BFGS (torch.optim.LBFGS(params, lr) as nd_BSPDE_case.py:347-348 and
 * with_corr...py:386-387 build it; train() calls optimizer.step(closure) with a
 * closure that re-runs loss_function + backward on the same batch, without
 * clipping: nd_BSPDE_case.py:357-361,380-381).  The closure is dbsde_loss_grad;
 * the host runs torch's step logic (fbsnn.py) on these device-vector
 * primitives.  Vectors are device fp32 of n elements (the flat parameter
 * order); reductions are fixed-order fp64, returned to the host (they
 * synchronise the context stream).
 */
#define DBSDE_VEC_DOT 0    /* sum_i a_i b_i */
#define DBSDE_VEC_ASUM 1   /* sum_i |a_i|   (b unused) */
#define DBSDE_VEC_AMAX 2   /* max_i |a_i|   (b unused) */
/* A NaN element makes every one of the three results NaN.  AMAX propagates it
 * as torch's tensor.abs().max() does (not C fmax, which drops it): torch's
 * L-BFGS stops on `flat_grad.abs().max() <= tolerance_grad`, which is False
 * for a NaN gradient, so a NaN gradient must not read as amax 0 = converged. */
int dbsde_vec_reduce(dbsde_ctx* ctx, int op, const float* a, const float* b, long long n, double* result);
/* z = alpha x + beta y in fp32 (z may alias x or y; y may be NULL when beta == 0) */
int dbsde_vec_axpby(dbsde_ctx* ctx, float* z, const float* x, const float* y, long long n, float alpha, float beta);
/* The L-BFGS two-loop recursion (torch's LBFGS.step direction), one launch:
 *   q = -g; for i = num-1..0: al_i = (s_i.q) ro_i, q -= al_i y_i;
 *   d = q h_diag; for i = 0..num-1: be_i = (y_i.d) ro_i, d += (al_i - be_i) s_i
 * s_i / y_i = rows slot[i] of the device [*, ld] history matrices S / Y (oldest
 * first, num <= 128); slot and ro are host arrays. */
int dbsde_lbfgs_direction(dbsde_ctx* ctx, const float* g, const float* S, const float* Y, long long ld, long long n,
                          const int* slot, const float* ro, int num, float h_diag, float* d);

/*
 * Exact / comparator solutions on the device (the references' evaluators):
 *   DBSDE_EXACT_BSB          u = exp((r + s^2)(T - t)) |x|^2    DeepBSDE.py:345-349
 *                            (r, s = p[0], p[1])
 *   DBSDE_EXACT_BS_CALL      Black-Scholes call price / delta of every coordinate
 *                            (nd_BSPDE_case.py:587-618; r, sigma, K = p[0..2])
 *   DBSDE_EXACT_BASKET_AVG   call on mean(x) with sigma / sqrt(D)
 *                            (with_corr...py:663-700; r, sigma, K = p[0..2])
 *   DBSDE_EXACT_BASKET_MEAN  mean over coordinates of the per-asset BS call
 *                            (with_corr...py:621-660; r, sigma, K = p[0..2])
 *   DBSDE_EXACT_HESTON       the European call under the two-factor Heston model
 *                            (DBSDE_PROB_HESTON2 with k = 1): x [R, 2] = (S, v), D == 2
 *                            (else DBSDE_EINVAL), p = {r, K, kappa, theta, sigma, rho};
 *                            price = S P1 - K exp(-r tau) P2, delta [R] = dprice/dS = P1,
 *                            P_j = 1/2 + 1/pi int_0^U Re[exp(-i phi ln K) f_j(phi) / (i phi)] dphi
 *                            with the branch-stable ("little trap", Albrecher, Mayer,
 *                            Schoutens, Tistaert 2007) form of the characteristic
 *                            functions f_j, in fp64 with the kernel's own complex
 *                            arithmetic.  Quadrature: 64 equal panels of [0, U], an
 *                            8-point Gauss-Legendre rule on each (one wavefront per
 *                            point, one panel per lane, the lanes summed by a fixed xor
 *                            butterfly: bitwise repeatable); U = 8 / sqrt(Vbar) times
 *                            the first power of sqrt(2) at which |f_j(U)| <= 1e-10 U for
 *                            both j (at most 2^8), Vbar = theta tau + (v - theta)
 *                            (1 - exp(-kappa tau)) / kappa the expected integrated
 *                            variance.  Within 2e-7 (K = 1) of the converged integral on
 *                            tau in [0.05, 2], v in [0.01, 1], S / K in [0.5, 2] at kappa
 *                            = 2, theta = 0.2, sigma = 0.3, rho in {0.8, -0.7}
 *                            (DESIGN 5); outside that domain the rule is unchecked.
 *                            Needs sigma > 0, K > 0, S > 0, v >= 0.
 *   DBSDE_EXACT_BS_PUT, _BASKET_AVG_PUT, _BASKET_MEAN_PUT, _HESTON_PUT
 *                            the European puts, with the parameters, shapes and ncol
 *                            of the call counterparts.  Computed directly, not as the
 *                            call minus parity: K exp(-r tau) N(-d2) - S N(-d1), delta
 *                            -N(-d1) (a deep out-of-the-money put keeps its relative
 *                            accuracy); Heston: K exp(-r tau) (1 - P2) - S (1 - P1),
 *                            delta -(1 - P1), with 1 - P_j = 1/2 - I_j / pi from the
 *                            call's quadrature sums I_j (same panels, same U).
 *   DBSDE_EXACT_GEO_ASIAN, DBSDE_EXACT_GEO_ASIAN_PUT
 *                            the call / put on the geometric average of kind
 *                            DBSDE_PROB_GEO_ASIAN in continuous time: x [R, D] = [G,
 *                            S_1..S_k], D >= 2, T the averaging horizon, params = {mu, r,
 *                            sigma, K, cbar, vbar}, cbar = mean_i (L L^T)_ii and vbar =
 *                            1^T L L^T 1 / k^2 of the factor between the assets (1 and
 *                            1 / k without one).  With tau = T - t,
 *                              M = ln G + [tau mean_i ln S_i + (mu - sigma^2 cbar / 2) tau^2 / 2] / T
 *                              V = sigma^2 vbar tau^3 / (3 T^2)
 *                              d2 = (M - ln K) / sqrt(V),  d1 = d2 + sqrt(V)
 *                              call = e^{-r tau} [e^{M + V/2} N(d1) - K N(d2)]
 *                              put  = e^{-r tau} [K N(-d2) - e^{M + V/2} N(-d1)]  (directly)
 *                            delta [R, D]: d/dG = +-e^{-r tau} e^{M + V/2} N(+-d1) / G,
 *                            d/dS_i = that G tau / (k T S_i).  Needs sigma, K, G, S > 0.
 *                            (Kind 9 is not a closed form: DBSDE_EINVAL.)
 *   DBSDE_EXACT_AMERICAN_PUT (14; kinds 12 and 13 are DBSDE_EINVAL)
 *                            the put max(K - s, 0) with early exercise, by a
 *                            Cox-Ross-Rubinstein tree in fp64: every coordinate of x [R, D]
 *                            is priced on its own, ncol = D (price and delta [R * D]), params
 *                            = {r, sigma, K, b, n_tree, pen}: b the risk-neutral drift of the
 *                            asset (mu_a + phi_r phi_c of a dbsde_problem), n_tree an
 *                            integer in [2, 4096], pen >= 0 or +inf.  With Delta = tau /
 *                            n_tree, u = e^{sigma sqrt(Delta)}, d = 1 / u, p = (e^{b Delta} -
 *                            d) / (u - d), node (i, j) at s u^{2j - i}, level n_tree holds
 *                            g = max(K - s, 0) and below it c = e^{-r Delta} (p v_up + (1 - p)
 *                            v_dn),
 *                              pen = +inf:  v = max(c, g)                    the American value
 *                              pen finite:  v = g > c ? (c + pen Delta g) / (1 + pen Delta) : c
 *                            the value of the penalised problem a context with that pen
 *                            trains on (pen = 0: the European tree).  delta = (v_11 - v_10) /
 *                            (s u - s d), the level-1 difference quotient.  One workgroup
 *                            per (point, coordinate), the level in LDS as doubles, barriers
 *                            between a level's reads and writes, no atomics: bitwise
 *                            repeatable.  DBSDE_EINVAL also for sigma or K <= 0, pen < 0 or
 *                            NaN, n_tree outside [2, 4096] or not an integer.  p depends
 *                            on the point's tau, which the host does not read: a point
 *                            whose p is not in [0, 1] (a coarse tree, |b| sqrt(Delta) >
 *                            sigma) has no tree value and gets NaN in price and delta.
 *   DBSDE_EXACT_BARRIER_CALL (15), DBSDE_EXACT_BARRIER_PUT (16)
 *                            the down-and-out call / up-and-out put without rebate on one
 *                            GBM asset (Reiner and Rubinstein 1991), B <= K / B >= K: every
 *                            coordinate of x [R, D] is priced on its own, ncol = D, params =
 *                            {r, sigma, K, b, B, n_mon}, b the cost of carry.  With
 *                            lambda = (b - sigma^2 / 2) / sigma^2, s = sigma sqrt(tau),
 *                              x1 = ln(S / K) / s + (1 + lambda) s
 *                              y1 = ln(B^2 / (S K)) / s + (1 + lambda) s
 *                              A = f S e^{(b - r) tau} N(f x1) - f K e^{-r tau} N(f x1 - f s)
 *                              C = f S e^{(b - r) tau} (B / S)^{2 (lambda + 1)} N(f y1)
 *                                  - f K e^{-r tau} (B / S)^{2 lambda} N(f y1 - f s)
 *                            the price is A - C, f = +1 (call), -1 (put); delta is its
 *                            analytic derivative in S.  n_mon > 0: the barrier is monitored
 *                            at n_mon equally spaced dates over tau and B is first moved
 *                            away from S by exp(-+0.5826 sigma sqrt(tau / n_mon)) (Broadie,
 *                            Glasserman and Kou 1997: down for the call, up for the put);
 *                            n_mon = 0: continuous monitoring.  Price and delta are 0 for S
 *                            on the knocked side of the (shifted) barrier; tau <= 0 returns
 *                            the payoff and its kink delta, 0 when S is beyond the unshifted
 *                            B.  DBSDE_EINVAL for sigma, K or B <= 0, a call with B > K, a
 *                            put with B < K, n_mon < 0 or NaN, non-finite r or b.
 * t [R], x [R, D] device fp32; price [R * ncol] and delta (nullable),
 * ncol = D for BS_CALL / BS_PUT / AMERICAN_PUT / BARRIER_CALL / BARRIER_PUT, 1 otherwise (GEO_ASIAN: price [R], delta [R, D]).  At t >= T the payoff and its
 * 0 / 1/2 / 1 (put: 0 / -1/2 / -1) delta are returned, as the references do.
 * Computed in fp64.  DBSDE_EINVAL before any HIP call: an unknown kind; NULL t /
 * x / params / price; R or D < 1; a Heston kind with D != 2; a GEO_ASIAN kind with D < 2; t, x, price or
 * delta not aligned to sizeof(float), params not to sizeof(double) (such an
 * address cannot be the buffer the kernels read and write).
 */
#define DBSDE_EXACT_BSB 0
#define DBSDE_EXACT_BS_CALL 1
#define DBSDE_EXACT_BASKET_AVG 2
#define DBSDE_EXACT_BASKET_MEAN 3
#define DBSDE_EXACT_HESTON 4
#define DBSDE_EXACT_BS_PUT 5
#define DBSDE_EXACT_BASKET_AVG_PUT 6
#define DBSDE_EXACT_BASKET_MEAN_PUT 7
#define DBSDE_EXACT_HESTON_PUT 8
#define DBSDE_EXACT_GEO_ASIAN 10
#define DBSDE_EXACT_GEO_ASIAN_PUT 11
#define DBSDE_EXACT_AMERICAN_PUT 14
#define DBSDE_EXACT_BARRIER_CALL 15
#define DBSDE_EXACT_BARRIER_PUT 16
int dbsde_exact(int kind, const float* t, const float* x, long long R, int D, float T, const double* params,
                float* price, float* delta, void* hip_stream);

/*
 * HJB Monte-Carlo comparator (hjb_implement.py:1088-1095):
 *   u(t, x) = -log( mean_k exp(-g(x + sqrt(2 |T - t|) z_k)) ),  g = log(1/2 + |y|^2/2)
 * over mc Philox draws z_k keyed by (seed, point index); t [P], x [P, D],
 * u [P] device.  Deterministic (fixed-order fp64 reduction).
 */
int dbsde_hjb_mc(const float* t, const float* x, int P, int D, float T, long long mc, unsigned long long seed,
                 float* u, void* hip_stream);

/*
 * Feynman-Kac Monte-Carlo comparator for every LINEAR problem (the device
 * counterpart of the reference drivers' Monte-Carlo pricers:
 * with_corr...py:1283-1325, basket_pricer.py, numerics/multidimensional_mc_pricer.py,
 * numerics/heston_closed_form_ii.py:6-83 -- but simulating the problem's own SDE).
 *
 * With phi_zz == 0, phi = phi_r (Y - phi_c X.Z) and the BSDE the step trains on
 * is the PDE  u_t + (mu + phi_r phi_c X).Du + 1/2 tr(sigma sigma^T D^2 u) - phi_r u = 0,
 * u(T, .) = g, solved by
 *   u(t, x) = E[ exp(-phi_r tau) g(X~_T) | X~_t = x ],  tau = T - t,
 * X~ following the problem's own Euler scheme with drift coefficient
 * mu_eff = mu_a + phi_r phi_c (fp32).  (BSB: mu = 0, sigma = 0.4 X, phi =
 * r (Y - X.Z) gives exp((r + sigma^2) tau) |x|^2 = DBSDE_EXACT_BSB.)  Heston has
 * phi_c = 0 and runs its own clamped drift and 2x2 blocks, one Brownian motion
 * per asset driving both S and v, as the training step does.  HESTON2 runs its
 * two-factor step (dbsde_problem above): sample k, asset d draws the Brownian
 * coordinates d (W^S_d) and D/2 + d (W^v_d); like HESTON it takes neither L nor
 * delta.  HESTON_CORR is HESTON with the assets' Brownian motions correlated:
 * dW = sqrt(dt_p) (L z), z the normals HESTON draws.  The unscaled L z of a group
 * of samples are formed once for all points by the triangular increment GEMM of
 * the correlated Heston rollout (its draws and its summation order) into a
 * workspace [samples, n_steps, k], and the path kernel reads them instead of
 * drawing.  The workspace is bounded by DBSDE_MC_WS_MB megabytes (read at every
 * call, default 1024); a call that needs more runs its sample chunks in groups,
 * which changes no bit of the result.  With L = I the result is HESTON's, bit for
 * bit.  phi_zz != 0 (HJB) is DBSDE_EINVAL: use dbsde_hjb_mc.
 * ASIAN (x [P, D] = [A_p, S_1..S_k], D = k + 1): thread (sample, asset d) runs
 * DIAG's step on S_d with Brownian coordinate d and accumulates
 * I_d = sum_n (double)fp32(S_{d,n} dt_n) (S at the left end of each step); the
 * sample's terminal average is A_T = A_p + (sum_d I_d) / (k T) in fp64, T the
 * full maturity (not tau_p), the I_d summed in the order DIAG sums its terminal
 * X; g(A_T) is the problem's payoff with one column.  delta (under DIAG's rules):
 * d/dA_p = g', d/dS_d = g' (sum_n (double)fp32(J_{d,n} dt_n)) / (k T), J the DIAG
 * tangent.  L [k, k] (k <= 128) correlates the assets as for DIAG.  tau_p <= 0
 * returns g(A_p), 0 and (g', 0, .., 0).
 * GEO_ASIAN (x [P, D] = [G_p, S_1..S_k]): ASIAN's threads and draws with
 * I_d = sum_n (double)fp32(lg(S_{d,n}) dt_n), lg as in the scheme above; after the
 * same reduction G_T = G_p exp((sum_d I_d) / (k T)) in fp64 and g(G_T) with one
 * column.  delta: d/dG_p = g' G_T / G_p, d/dS_d = g' G_T (sum_n (double)fp32((J_{d,n}
 * / S_{d,n}) dt_n)) / (k T).  L [k, k], k <= 128.  tau_p <= 0 returns g(G_p), 0 and
 * (g', 0, .., 0).  Its exact value in continuous time is DBSDE_EXACT_GEO_ASIAN; the
 * scheme differs from it by O(dt).
 * BARRIER (x [P, D], DIAG's state): the value is exp(-phi_r tau_p) mean_k g(X_N) alive_k,
 * alive_k = no row n = 0..n_steps of sample k's path was knocked (the rule of the problem
 * kind above: the statistic in fp32 in the rollout's row-sum order, so a restatement
 * reproduces every flag); the standard error is that of the same summand.  A 16-lane
 * group runs one sample of one point, lane l the assets l, l + 16, ..; g(X_N) takes the
 * fp64 sum of the lanes' ascending fp64 partial sums met in the same butterfly.  Drift
 * mu_eff, DIAG's step and draws, common to all points.  nb = D <= 128 with or without L
 * (above: DBSDE_EINVAL).  With L the unscaled L z come from HESTON_CORR's increment
 * workspace (the same bound and grouping).  delta != NULL is DBSDE_EINVAL: the pathwise
 * estimator is biased across the knock-out indicator; bump and reprice on the same
 * draws instead.  tau_p <= 0 returns g(x_p) and 0 for a live point, 0 and 0 for a
 * knocked one.
 *
 *   L       device [nb, nb] row-major lower Cholesky factor (the lower triangle is
 *           read), NULL = independent increments; DIAG: nb = D <= 128;
 *           HESTON_CORR: required, nb = k = D / 2 <= 511
 *   t, x    device t [P], x [P, D] (Heston: D = 2k, [S_1..S_k, v_1..v_k])
 *   value   device [P]:     exp(-phi_r tau_p) mean_k g(X_T)
 *   stderr_ device [P], nullable: exp(-phi_r tau_p) std_k(g, ddof = 1) / sqrt(mc)
 *           (0 for mc == 1)
 *   delta   device [P, D], nullable, DIAG only: the pathwise estimator
 *           exp(-phi_r tau_p) mean_k dg/dX_d(X_T) J_d, J the tangent of the Euler
 *           step, J <- (J + (mu_eff J) dt) + (sig_a J) dW_d, J_0 = 1; 1/2 at the
 *           kink of the call payoffs (-1/2: puts), 0 in the columns past g_cols.  Heston with
 *           delta != NULL is DBSDE_EINVAL (its S and v tangents couple): bump
 *           and reprice on the same draws instead.
 *
 * Point p runs the training grid with T replaced by tau_p = fp32(T) - t_p:
 * t_n = fp32(fp64 cumsum of tau_p / n_steps), dt_n their fp32 differences,
 * sqrt(dt) = sqrtf(tau_p / n_steps).  The normals of sample k, step n, Brownian
 * coordinate d are those the device-mode rollout draws for global path k
 * (Philox counter (d, n / 4, k, offset), key from seed), for EVERY point of the
 * call: common random numbers, so a surface is smooth in x and differences of
 * neighbouring points carry no sampling noise of their own.  A point's result
 * depends neither on P nor on its index in the call.  The state is fp32 and
 * the step is the training step's, in the reference's operation order;
 * sum g, sum g^2 and the delta sums are fixed-order fp64 sums: the result is
 * bitwise repeatable.  g runs over the first g_cols columns as in the step;
 * u_clamp and q3 are ignored.  A point with tau_p <= 0 returns g(x_p), standard
 * error 0 and dg/dx_p.
 *
 * DBSDE_EINVAL before any HIP call: NULL prob / t / x / value; P, D, n_steps
 * or mc < 1; mc > 2^32; D > 4096; Heston with an odd D, with L or with delta;
 * L with D > 128; HESTON_CORR without L, with an odd D, with delta or with
 * k = D / 2 > 511; an unknown kind or g_kind; phi_zz != 0; pen != 0 (not linear:
 * the arbiter of a penalised problem is DBSDE_EXACT_AMERICAN_PUT); ASIAN with D < 2,
 * phi_c != 0, g_cols != 1, g_kind SUMSQ or LOG, or L with D - 1 > 128; GEO_ASIAN with any
 * of those or sig_b != 0; BARRIER with any refusal of the problem kind above, D > 128 or
 * delta != NULL.  Needs no context;
 * the work is enqueued on hip_stream.
 */
int dbsde_mc_value(const dbsde_problem* prob, int D, float T, const float* L, const float* t, const float* x, int P,
                   int n_steps, long long mc, unsigned long long seed, unsigned long long offset, float* value,
                   float* stderr_, float* delta, void* hip_stream);

/* Per-kernel timing with HIP events on the context stream (bench/profiling).
 * ctx == NULL addresses the process-wide store of the calls that take no
 * context: dbsde_mc_value with kind HESTON_CORR records its launches there
 * ("corr_increments", "mc_heston_corr_paths") while that store is enabled. */
int dbsde_profile_enable(dbsde_ctx* ctx, int enable);
int dbsde_profile_count(dbsde_ctx* ctx);
int dbsde_profile_read(dbsde_ctx* ctx, int idx, char* name, int name_len, double* total_ms,
                       double* alg_flops, double* alg_bytes, long long* launches);
int dbsde_profile_reset(dbsde_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* DBSDE_H */
