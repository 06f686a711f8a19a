// net.hip -- what a context is made of: the network layout and its padded
// geometry, the weight / gradient / row buffers and their pack descriptors,
// the streams and the order points between them, the profiling store, and
// the C ABI for creating, destroying and inspecting a context.
#include <hip/hip_runtime.h>

// the events that order the context's streams need no system-scope fence
// (device work only; kernels carry their own device-scope release / acquire):
// 0.4625 vs 0.4663 ms/step, M = 128 0.1448 vs 0.1474 (profiles/r5_ab_streams.txt)
#ifndef DBSDE_EVF
#define DBSDE_EVF (hipEventDisableTiming | hipEventDisableSystemFence)
#endif
// chunk fork / join through stream memory operations (stream_order)
#ifndef DBSDE_MEMOPS
#define DBSDE_MEMOPS 1
#endif
#define DBSDE_DEVICE_HELPERS_ONLY
#include "ctx.hpp"

namespace {
thread_local std::string g_last_error;
}

int fail(dbsde_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  g_last_error = msg;
  return code;
}

int dalloc(dbsde_ctx* c, void** p, size_t bytes) {
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) return fail(c, DBSDE_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  e = hipMemset(*p, 0, bytes);
  if (e != hipSuccess) return fail(c, DBSDE_EHIP, std::string("hipMemset: ") + hipGetErrorString(e));
  c->allocs.push_back(*p);
  return DBSDE_OK;
}

// ---------------------------------------------------------------------------
// stream ordering
// ---------------------------------------------------------------------------
namespace {

// A value wait is a kernel that spins until the value arrives, so it needs
// the writer's queue to make progress beside it: anything that runs one kernel
// at a time (kernel serialisation, launch blocking, rocprofv3 counter
// collection) would never run the write.  Those environments, any profiler /
// tool library the runtime loads (HSA_TOOLS_LIB, a preloaded rocprof library,
// ROCPROFILER_* / ROCP_* settings) and DBSDE_STREAM_ORDER=events order the
// streams with events instead; DBSDE_STREAM_ORDER=values forces value ops.
// Returns the reason (nullptr: value operations).
// (env: a NULL-terminated NAME=VALUE block, nullptr = the process environment)
const char* env_get(const char* const* env, const char* n) {
  if (!env) return getenv(n);
  const size_t k = strlen(n);
  for (; *env; ++env)
    if (!strncmp(*env, n, k) && (*env)[k] == '=') return *env + k + 1;
  return nullptr;
}
bool env_set(const char* n, const char* const* env = nullptr) {
  const char* v = env_get(env, n);
  return v && v[0] && strcmp(v, "0") != 0 && strcasecmp(v, "false") != 0;
}
extern "C" char** environ;
const char* events_reason(const char* const* env = nullptr) {
  if (const char* v = env_get(env, "DBSDE_STREAM_ORDER")) {
    if (strcmp(v, "events") == 0) return "DBSDE_STREAM_ORDER=events";
    if (strcmp(v, "values") == 0) return nullptr;
  }
  static const char* const serial[] = {"AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING", "ROCPROF_COUNTER_COLLECTION",
                                       "ROCPROF_COUNTERS", "HSA_TOOLS_LIB"};
  for (const char* n : serial)
    if (env_set(n, env)) return n;
  if (const char* p = env_get(env, "LD_PRELOAD"))
    if (strstr(p, "rocprof")) return "LD_PRELOAD (rocprof)";
  for (const char* const* e = env ? env : environ; e && *e; ++e)
    if (!strncmp(*e, "ROCPROFILER_", 12) || !strncmp(*e, "ROCP_", 5)) return "ROCPROFILER_* / ROCP_* setting";
  return nullptr;
}
bool order_by_events() { return events_reason() != nullptr; }
// stderr line naming the ordering the first context chose (once per process)
void log_ordering(bool memops) {
  static bool done = false;
  if (done || env_set("DBSDE_QUIET")) return;
  done = true;
  const char* why = events_reason();
  fprintf(stderr, "dbsde: cross-stream order by %s%s%s\n", memops ? "stream value operations" : "events",
          why ? " -- " : (memops ? "" : " -- value waits unsupported by the device"), why ? why : "");
}

hipEvent_t order_event(dbsde_ctx* c, int slot) {
  switch (slot) {
    case ORD_FORK: return c->ev_pipe[0];
    case ORD_JOIN: return c->ev_pipe[1];
    case ORD_PF_AFTER_MAIN:
    case ORD_MAIN_AFTER_PF: return c->ev_pf_order;
    case ORD_SWITCH: return c->ev_switch;
    default: return c->ps.pend[slot - ORD_PEND0].ready;
  }
}

}  // namespace

// order points (ctx.hpp)
int order_mark(dbsde_ctx* c, int slot, hipStream_t from, unsigned long long& token) {
  if (c->memops) {
    token = ++c->order_epoch[slot];
    HIPC(c, hipStreamWriteValue64(from, c->d_order + slot, token, 0));
  } else {
    token = 0;
    HIPC(c, hipEventRecord(order_event(c, slot), from));
  }
  return DBSDE_OK;
}
int order_wait(dbsde_ctx* c, int slot, unsigned long long token, hipStream_t to) {
  if (c->memops)
    HIPC(c, hipStreamWaitValue64(to, c->d_order + slot, token, hipStreamWaitValueGte, ~0ull));
  else
    HIPC(c, hipStreamWaitEvent(to, order_event(c, slot), 0));
  return DBSDE_OK;
}
// `to` waits until `from` has reached this point of its queue
int stream_order(dbsde_ctx* c, hipStream_t from, hipStream_t to, int slot) {
  unsigned long long v = 0;
  int rc = order_mark(c, slot, from, v);
  return rc ? rc : order_wait(c, slot, v, to);
}

hipEvent_t get_event(dbsde_ctx* c) {
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// the profiling store of the calls that take no context (dbsde_mc_value): a
// context that is never created on a device -- only its profiling members and
// its stream are used -- made at first use and kept for the process
dbsde_ctx* free_call_ctx() {
  static dbsde_ctx* const c = new dbsde_ctx();
  return c;
}

int prof_id(dbsde_ctx* c, const std::string& name) {
  auto it = c->agg_idx.find(name);
  if (it != c->agg_idx.end()) return it->second;
  int id = (int)c->agg.size();
  c->agg.push_back(ProfAgg{name});
  c->agg_idx[name] = id;
  return id;
}

namespace {

// ---------------------------------------------------------------------------
// network layout (state_dict order; oracle/timeparallel.param_layout mirrors it)
// ---------------------------------------------------------------------------
int build_net(dbsde_ctx* c) {
  const dbsde_config& g = c->cfg;
  if (g.n_layers < 4 || g.n_layers > 9) return fail(c, DBSDE_EINVAL, "len(layers) must be in [4, 9]");
  c->L.assign(g.layers, g.layers + g.n_layers);
  for (int v : c->L)
    if (v <= 0) return fail(c, DBSDE_EINVAL, "layer widths must be positive");
  const int n = g.n_layers;
  c->D = c->L[0] - 1;
  if (c->L.back() != 1) return fail(c, DBSDE_EINVAL, "last layer width must be 1 (u is a scalar)");
  if (c->D < 1) return fail(c, DBSDE_EINVAL, "layers[0] must be D+1 >= 2");
  c->K = n - 3;   // 1..6 hidden blocks
  c->mode = g.mode;
  c->act = g.activation;
  if (c->act < DBSDE_ACT_SINE || c->act > DBSDE_ACT_SOFTPLUS) return fail(c, DBSDE_EINVAL, "unknown activation");
  long long off = 0;
  auto lin = [&](int o, int i) {
    Lin l;
    l.out = o;
    l.in = i;
    l.w = off;
    off += (long long)o * i;
    l.b = off;
    off += o;
    return l;
  };
  c->B.clear();
  c->V.clear();
  const auto& L = c->L;
  if (g.mode == DBSDE_MODE_FC) {
    c->has_v = false;
    c->proj = false;
    c->rho = 0.f;
    c->in = lin(L[1], L[0]);
    for (int j = 1; j <= c->K; ++j) c->B.push_back(lin(L[j + 1], L[j]));
    c->out = lin(L[n - 1], L[n - 2]);
  } else if (g.mode == DBSDE_MODE_NAIS_NET || g.mode == DBSDE_MODE_RESNET) {
    const bool st = g.mode == DBSDE_MODE_NAIS_NET;
    c->has_v = st;
    c->proj = st;
    c->rho = 1.f;
    c->in = lin(L[1], L[0]);
    for (int j = 1; j <= c->K; ++j) c->B.push_back(lin(L[j + 1], L[j]));
    c->out = lin(L[n - 1], L[n - 2]);
    if (st)
      for (int i = 1; i <= n - 2; ++i) {
        Lin v = lin(L[i], L[0]);
        if (i <= c->K) c->V.push_back(v);  // input_layers[K] is never used (Q6)
      }
  } else if (g.mode == DBSDE_MODE_NAISNET) {
    if (n < 4 || n > 6) return fail(c, DBSDE_EINVAL, "Naisnet supports len(layers) in {4,5,6}");
    c->has_v = true;
    c->proj = true;
    c->rho = 1.f;
    c->in = lin(L[1], L[0]);
    for (int j = 1; j <= c->K; ++j) {
      c->B.push_back(lin(L[j + 1], L[j]));
      c->V.push_back(lin(L[j + 1], L[0]));
    }
    c->out = lin(L[n - 1], L[n - 2]);
  } else {
    return fail(c, DBSDE_EINVAL, "unknown mode");
  }
  if (c->rho != 0.f)
    for (int j = 2; j < n - 1; ++j)
      if (L[j] != L[1]) return fail(c, DBSDE_EINVAL, "residual modes need equal hidden widths");
  if (c->proj && L[1] > NAIS_WIDE_LMAX)
    return fail(c, DBSDE_EINVAL, "NAIS projection supports hidden width <= 1024");
  c->proj_wide = c->proj && L[1] > NAIS_LMAX;
  c->nparams = off;
  c->used.assign(off, 1);
  if (g.mode == DBSDE_MODE_NAIS_NET) {
    // input_layers[K] occupies the tail of the flat vector
    const long long tail = (long long)L[n - 2] * L[0] + L[n - 2];
    std::fill(c->used.end() - tail, c->used.end(), 0);
  }
  // padded geometry
  c->Dp = pad16(c->D + 2);
  if (c->Dp > DP_MAX) return fail(c, DBSDE_EINVAL, "D > 1022 is not supported (Dp = pad16(D + 2) must be <= 1024)");
  c->Wp.resize(c->K + 1);
  c->col.resize(c->K + 1);
  c->Stot = 0;
  c->Wmax = 0;
  for (int j = 0; j <= c->K; ++j) {
    c->Wp[j] = padw(L[j + 1]);
    c->col[j] = c->Stot;
    c->Stot += c->Wp[j];
    c->Wmax = std::max(c->Wmax, c->Wp[j]);
  }
  c->Stot_x = c->has_v ? c->Stot : c->Wp[0];
  bool uniform = true;
  for (int j = 1; j <= c->K; ++j) uniform = uniform && c->Wp[j] == c->Wp[0];
  const char* env = getenv("DBSDE_FUSED");
  const bool allow = !(env && env[0] == '0');
  const char* ex3 = getenv("DBSDE_X3");
  const bool want_x3 = !(ex3 && ex3[0] == '0');
  c->x3 = want_x3 && fused_variant(c->Wp[0] / 16, c->Dp / 16, c->K, c->act, c->has_v, true) >= 0;
  c->fused = allow && uniform && fused_variant(c->Wp[0] / 16, c->Dp / 16, c->K, c->act, c->has_v, c->x3) >= 0;
  c->x3 = c->x3 && c->fused;
  c->fv = c->fused ? fused_variant(c->Wp[0] / 16, c->Dp / 16, c->K, c->act, c->has_v, c->x3) : -1;
  // the column-split form for small batches (DBSDE_CS=0 never, =1 always,
  // default when the 64-row kernels would fill at most half the chip's slots)
  {
    const char* ecs = getenv("DBSDE_CS");
    c->cs_mode = !ecs ? 2 : (ecs[0] == '0' ? 0 : 1);
    c->fv_cs = (c->fv >= 0 && c->cs_mode && fused_at(c->fv).rows == P3_ROWS && c->x3)
                   ? fused_variant(c->Wp[0] / 16, c->Dp / 16, c->K, c->act, c->has_v, true, true)
                   : -1;
  }
  // FC / Resnet layouts the fused kernels do not cover: split-bf16 chain GEMMs
  // (uniform hidden width, output blocks a multiple of the column tile)
  // (the same layouts' weight-gradient tiles run split-bf16 behind the fused
  // phase kernels too: tnx3)
  c->tnx3 = want_x3 && !c->has_v && uniform && c->Dp <= 128;
  for (int j = 0; j <= c->K && c->tnx3; ++j) c->tnx3 = (c->Wp[j] / 16) % nt_for(c->Wp[j]) == 0;
  c->x3chain = c->tnx3 && !c->fused;
  // problem kind: Brownian dimension, g columns, u clamp
  const dbsde_problem& pr = g.problem;
  if (pr.kind == DBSDE_PROB_HESTON_CORR)
    return fail(c, DBSDE_EINVAL,
                "DBSDE_PROB_HESTON_CORR is dbsde_mc_value's kind: a context takes kind DBSDE_PROB_HESTON plus "
                "dbsde_set_corr");
  if (pr.kind != DBSDE_PROB_DIAG && pr.kind != DBSDE_PROB_HESTON && pr.kind != DBSDE_PROB_HESTON2 &&
      pr.kind != DBSDE_PROB_ASIAN && pr.kind != DBSDE_PROB_GEO_ASIAN && pr.kind != DBSDE_PROB_BARRIER)
    return fail(c, DBSDE_EINVAL, "unknown problem kind");
  if (pr.g_kind < 0 || pr.g_kind > DBSDE_G_SMOOTH_PUT) return fail(c, DBSDE_EINVAL, "unknown terminal condition");
  c->heston = pr.kind == DBSDE_PROB_HESTON;
  c->heston2 = pr.kind == DBSDE_PROB_HESTON2;
  c->geo = pr.kind == DBSDE_PROB_GEO_ASIAN;
  c->asian = pr.kind == DBSDE_PROB_ASIAN || c->geo;   // the geometric problem runs the arithmetic one's launches
  if (c->asian) {
    if (const char* why = c->geo ? geo_asian_refusal(pr, c->D) : asian_refusal(pr, c->D))
      return fail(c, DBSDE_EINVAL, why);
  }
  c->barrier = pr.kind == DBSDE_PROB_BARRIER;   // DIAG's state, rollouts and coefficients, plus the stop pass
  if (c->barrier)
    if (const char* why = barrier_refusal(pr)) return fail(c, DBSDE_EINVAL, why);
  if (const char* why = pen_refusal(pr)) return fail(c, DBSDE_EINVAL, why);
  if ((c->heston || c->heston2) && c->D % 2 != 0)
    return fail(c, DBSDE_EINVAL, "Heston state is [S_1..S_k, v_1..v_k]: layers[0] - 1 must be even");
  // two-factor Heston: |rho| <= 1, and the v-column weight of the second Brownian motion
  if (c->heston2 && !(std::fabs((double)pr.h_rho) <= 1.0))
    return fail(c, DBSDE_EINVAL, "two-factor Heston needs |h_rho| <= 1");
  c->rhob = c->heston2 ? (float)std::sqrt(1.0 - (double)pr.h_rho * (double)pr.h_rho) : 0.f;
  c->nb = c->heston ? c->D / 2 : (c->asian ? c->D - 1 : c->D);
  c->gcols = pr.g_cols > 0 ? pr.g_cols : c->D;
  if (c->gcols > c->D) return fail(c, DBSDE_EINVAL, "g_cols exceeds the state dimension");
  c->u_clamp = pr.u_clamp != 0;
  return DBSDE_OK;
}

PackDesc mk_desc(const float* src, int src_ld, float* dst, int dst_ld, int rows, int cols, int transpose,
                 int mode, float scale = 1.f) {
  PackDesc d{};
  d.src = src;
  d.src_ld = src_ld;
  d.dst = dst;
  d.dst_ld = dst_ld;
  d.rows = rows;
  d.cols = cols;
  d.transpose = transpose;
  d.mode = mode;
  d.scale = scale;
  return d;
}

// Pack descriptors use "relative" pointers: a src/dst value < 2^40 with bit
// flags is awkward, so instead we encode param/grad-relative addresses as
// offsets from a null base and fix them up per call (see fixup_descs).
constexpr uintptr_t kParamTag = (uintptr_t)1 << 62;
constexpr uintptr_t kGradTag = (uintptr_t)1 << 61;
inline float* ptag(long long off) { return (float*)(kParamTag | (uintptr_t)(off * 4)); }
inline float* gtag(long long off) { return (float*)(kGradTag | (uintptr_t)(off * 4)); }

int build_buffers(dbsde_ctx* c) {
  const int K = c->K, D = c->D, Dp = c->Dp;
  int rc;
  if ((rc = dalloc_t(c, &c->BtIn, (size_t)c->Stot_x * Dp))) return rc;
  if ((rc = dalloc_t(c, &c->BtZ, (size_t)(Dp + (Dp > 128 ? ZG_PAD : 0)) * c->Stot_x))) return rc;
  if ((rc = dalloc_t(c, &c->wout, (size_t)c->Wp[K]))) return rc;
  if ((rc = dalloc_t(c, &c->bout, 16))) return rc;
  c->Bf.assign(K + 1, nullptr);
  c->Bb.assign(K + 1, nullptr);
  c->beta.assign(K + 1, nullptr);
  c->rtr.assign(K + 1, nullptr);
  c->abar.assign(K + 1, nullptr);
  for (int j = 1; j <= K; ++j) {
    if ((rc = dalloc_t(c, &c->Bf[j], (size_t)c->Wp[j] * c->Wp[j - 1]))) return rc;
    if ((rc = dalloc_t(c, &c->Bb[j], (size_t)c->Wp[j - 1] * c->Wp[j]))) return rc;
    if ((rc = dalloc_t(c, &c->beta[j], (size_t)c->Wp[j]))) return rc;
  }
  const int LW = c->L[1];
  if (c->proj) {
    if ((rc = dalloc_t(c, &c->norms, (size_t)K + 1))) return rc;
    std::vector<float*> hr(K), ha(K), hs(K), hb(K, nullptr);
    std::vector<long long> hw(K);
    for (int j = 1; j <= K; ++j) {
      if ((rc = dalloc_t(c, &c->rtr[j], (size_t)LW * LW))) return rc;
      if ((rc = dalloc_t(c, &c->abar[j], (size_t)LW * LW))) return rc;
      if ((rc = dalloc_t(c, &hs[j - 1], (size_t)LW * LW))) return rc;
      if (c->proj_wide && (rc = dalloc_t(c, &hb[j - 1], (size_t)LW * LW))) return rc;
      hr[j - 1] = c->rtr[j];
      ha[j - 1] = c->abar[j];
      hw[j - 1] = c->B[j - 1].w;
    }
    // (the wide kernels' triangle of 64 x 64 tiles is the smaller count)
    if ((rc = dalloc_t(c, &c->proj_part, (size_t)K * std::max((LW * LW + 255) / 256, ((LW + 15) / 16) * ((LW + 15) / 16)))))
      return rc;
    if (c->proj_wide) {
      if ((rc = dalloc_t(c, &c->proj_sq, K))) return rc;
      if ((rc = dalloc_t(c, &c->proj_dot, K))) return rc;
      if ((rc = dalloc_t(c, &c->d_sbuf, K))) return rc;
      HIPC(c, hipMemcpy(c->d_sbuf, hb.data(), K * sizeof(float*), hipMemcpyHostToDevice));
    }
    c->dot_nblk = (LW * LW + 63) / 64;
    c->dot_nused = c->dot_nblk;   // tnw layouts override below
    if ((rc = dalloc_t(c, &c->dot_part, (size_t)K * c->dot_nblk))) return rc;
    if ((rc = dalloc_t(c, &c->d_rtr, K))) return rc;
    if ((rc = dalloc_t(c, &c->d_abar, K))) return rc;
    if ((rc = dalloc_t(c, &c->d_wsnap, K))) return rc;
    if ((rc = dalloc_t(c, &c->d_woffs, K))) return rc;
    HIPC(c, hipMemcpy(c->d_rtr, hr.data(), K * sizeof(float*), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->d_abar, ha.data(), K * sizeof(float*), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->d_wsnap, hs.data(), K * sizeof(float*), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->d_woffs, hw.data(), K * sizeof(long long), hipMemcpyHostToDevice));
  }
  if ((rc = dalloc_t(c, &c->d_used, (size_t)c->nparams))) return rc;
  HIPC(c, hipMemcpy(c->d_used, c->used.data(), c->nparams, hipMemcpyHostToDevice));
  c->opt_nparts = 256;
  if ((rc = dalloc_t(c, &c->opt_part, c->opt_nparts))) return rc;

  // ---- fragment images for the phase kernels (phase.hpp)
  const int TW = c->Wp[0] / 16, TDp = Dp / 16;
  c->imgX.assign(K + 1, nullptr);
  c->imgZ.assign(K + 1, nullptr);
  c->imgF.assign(K + 1, nullptr);
  c->imgB.assign(K + 1, nullptr);
  // floats of an image with tout output / tin input blocks of 16: fp32
  // fragments (1 KiB each), or split-bf16 fragments (3 KiB per 32-wide block)
  const bool img_x3 = c->x3 || c->x3chain;
  auto img_floats = [&](int tout, int tin) -> size_t {
    return img_x3 ? (size_t)tout * ((tin + 1) / 2) * 768 : (size_t)tout * tin * 256;
  };
  if (c->fused || c->x3chain) {
    for (int j = 0; j <= (c->has_v ? K : 0); ++j) {
      if ((rc = dalloc_t(c, &c->imgX[j], img_floats(TW, TDp)))) return rc;
      if ((rc = dalloc_t(c, &c->imgZ[j], img_floats(TDp, TW)))) return rc;
    }
    for (int j = 1; j <= K; ++j) {
      if ((rc = dalloc_t(c, &c->imgF[j], img_floats(TW, TW)))) return rc;
      if ((rc = dalloc_t(c, &c->imgB[j], img_floats(TW, TW)))) return rc;
    }
  }
  const int fsplit = img_x3 ? 1 : 0;
  // the fused phase kernels read only the fragment images: their contexts skip
  // the fp32 copies the per-layer chain GEMMs use (half the pack writes, and
  // all of its transposed ones)
  const bool images_only = c->fused;
  auto frag = [fsplit, images_only](PackDesc d, float* img, int tin, int tout, int row0, int col0) {
    if (images_only) d.dst = nullptr;
    d.fdst = img;
    d.ftin = tin;
    d.ftout = tout;
    d.frow0 = row0;
    d.fcol0 = col0;
    d.fsplit = fsplit;
    return d;
  };

  // ---- prep descriptors: flat params -> packed weight buffers
  std::vector<PackDesc> P, PZ, PJ;   // PJ: the fp32 copies a fused context skips, for the jet kernels
  auto keep = [&](const PackDesc& d) {
    if (images_only) PJ.push_back(d);
    return d;
  };
  auto add_x_level = [&](int j, const Lin& w, const Lin* b2) {
    float* dst = c->BtIn + (size_t)c->col[j] * Dp;
    P.push_back(frag(keep(mk_desc(ptag(w.w), D + 1, dst, Dp, w.out, D + 1, 0, PK_COPY)), c->imgX[j], TDp, TW, 0, 0));
    if (b2) {
      PackDesc d = mk_desc(ptag(w.b), 1, dst + D + 1, Dp, w.out, 1, 0, PK_ADD2);
      d.src2 = ptag(b2->b);
      d.src2_ld = 1;
      P.push_back(frag(keep(d), c->imgX[j], TDp, TW, 0, D + 1));
    } else {
      P.push_back(frag(keep(mk_desc(ptag(w.b), 1, dst + D + 1, Dp, w.out, 1, 0, PK_COPY)), c->imgX[j], TDp, TW, 0, D + 1));
    }
    const PackDesc z = mk_desc(ptag(w.w), D + 1, c->BtZ + c->col[j], c->Stot_x, w.out, D + 1, 1, PK_COPY);
    P.push_back(frag(z, c->imgZ[j], TW, TDp, 0, 0));
    if (images_only) PZ.push_back(z);
  };
  add_x_level(0, c->in, nullptr);
  if (c->has_v)
    for (int j = 1; j <= K; ++j) add_x_level(j, c->V[j - 1], &c->B[j - 1]);
  for (int j = 1; j <= K; ++j) {
    const Lin& b = c->B[j - 1];
    if (c->proj) {
      // |R_j|_F^2: this block's rtr partials, or (wide) the one sum
      // projw_forward_launch reduced them to, as a single partial
      const int nblk = c->proj_wide ? 1 : ((LW + 15) / 16) * ((LW + 15) / 16);
      const double* pn = c->proj_wide ? c->proj_sq + (j - 1) : c->proj_part + (size_t)(j - 1) * nblk;
      PackDesc d = mk_desc(c->rtr[j], LW, c->Bf[j], c->Wp[j - 1], LW, LW, 0, PK_NEGPROJ);
      d.proj = pn;
      d.proj_n = nblk;
      d.proj_norm = nullptr;
      keep(d);
      d.proj_norm = c->norms + (j - 1);
      P.push_back(frag(d, c->imgF[j], TW, TW, 0, 0));
      d = mk_desc(c->rtr[j], LW, c->Bb[j], c->Wp[j], LW, LW, 1, PK_NEGPROJ);
      d.proj = pn;
      d.proj_n = nblk;
      d.proj_norm = nullptr;
      P.push_back(frag(d, c->imgB[j], TW, TW, 0, 0));
    } else {
      P.push_back(frag(keep(mk_desc(ptag(b.w), b.in, c->Bf[j], c->Wp[j - 1], b.out, b.in, 0, PK_COPY)), c->imgF[j],
                       TW, TW, 0, 0));
      P.push_back(frag(mk_desc(ptag(b.w), b.in, c->Bb[j], c->Wp[j], b.out, b.in, 1, PK_COPY), c->imgB[j], TW, TW, 0,
                       0));
      P.push_back(mk_desc(ptag(b.b), 1, c->beta[j], 1, b.out, 1, 0, PK_COPY));
    }
  }
  P.push_back(mk_desc(ptag(c->out.w), 1, c->wout, 1, c->out.in, 1, 0, PK_COPY));
  P.push_back(mk_desc(ptag(c->out.b), 1, c->bout, 1, 1, 1, 0, PK_COPY));
  c->n_prep = (int)P.size();
  c->prep_blocks = 1;
  for (const PackDesc& d : P) c->prep_blocks = std::max(c->prep_blocks, (d.rows * d.cols + 255) / 256);

  // ---- gradient slabs and finalize descriptors
  bool uniformW = true;
  for (int j = 0; j <= K; ++j) uniformW = uniformW && c->Wp[j] == c->Wp[0];
  // P = 2K + 2 problems in 4-wave workgroups: K odd
  c->tnw = c->has_v && uniformW && c->Wp[0] == Dp && Dp <= 128 && K <= 6 && (2 * K + 2) % 4 == 0;
  if (const char* e = getenv("DBSDE_TNW")) c->tnw = c->tnw && atoi(e) != 0;
  if (const char* e = getenv("DBSDE_ROLLOUT2")) c->rollout2 = atoi(e) != 0;
  std::vector<PackDesc> F;
  if (c->tnw) {
    const int T = Dp, P = 2 * K + 2, S = c->tnw_Smax;
    c->tnw_nb = T / 16;
    c->tnw_P = P;
    const char* ex = getenv("DBSDE_TNW_X3");
    c->tnw_x3 = c->x3 && c->tnw_nb == 7 && !(ex && ex[0] == '0');
    if (c->proj) {
      c->dot_nused = (T * T + TF_ELEMS - 1) / TF_ELEMS;
      if (c->dot_nused > c->dot_nblk) return fail(c, DBSDE_EINVAL, "internal: dot partials");
    }
    if ((rc = dalloc_t(c, &c->slabW, (size_t)S * P * T * T))) return rc;
    auto wsum = [&](int p, int r0, int c0, int rows, int cols, float* dst, int dst_ld, float scale) {
      PackDesc d = mk_desc(c->slabW + (size_t)p * T * T + (size_t)r0 * T + c0, T, dst, dst_ld, rows, cols, 0,
                           PK_SLABSUM, scale);
      d.nslab = S;
      d.slab_stride = (long long)P * T * T;
      d.sp = p;
      d.sr0 = r0;
      d.sc0 = c0;
      F.push_back(d);
    };
    // x-stack problems p = j (input layer, V_j), block problems p = K + j (B_j)
    wsum(0, 0, 0, c->in.out, D + 1, gtag(c->in.w), D + 1, 1.f);
    wsum(0, 0, D + 1, c->in.out, 1, gtag(c->in.b), 1, 1.f);
    for (int j = 1; j <= K; ++j) {
      const Lin& v = c->V[j - 1];
      wsum(j, 0, 0, v.out, D + 1, gtag(v.w), D + 1, 1.f);
      wsum(j, 0, D + 1, v.out, 1, gtag(v.b), 1, 1.f);
      wsum(j, 0, D + 1, v.out, 1, gtag(c->B[j - 1].b), 1, 1.f);
      const Lin& b = c->B[j - 1];
      wsum(K + j, 0, 0, b.out, b.in, c->abar[j], LW, -1.f);  // Abar = -Bbar
      F.back().dotR = c->rtr[j];
      F.back().dot_part = c->dot_part + (size_t)(j - 1) * c->dot_nblk;
    }
    // output layer: row 0 of problem 2K+1 is w_out, element (1, 0) is b_out
    wsum(2 * K + 1, 0, 0, 1, c->out.in, gtag(c->out.w), 1, 1.f);
    wsum(2 * K + 1, 1, 0, 1, 1, gtag(c->out.b), 1, 1.f);
  } else {
    c->slab.assign(K + 1, nullptr);
    c->slab_mt.assign(K + 1, 0);
    c->slab_nt.assign(K + 1, 0);
    c->slab_mv.assign(K + 2, 0);
    c->slab_nv.assign(K + 2, 0);
    auto mkslab = [&](int j, int m, int n) -> int {
      c->slab_mv[j] = m;
      c->slab_nv[j] = n;
      c->slab_mt[j] = (m + 63) / 64;
      c->slab_nt[j] = (n + 63) / 64;
      return dalloc_t(c, &c->slab[j], (size_t)c->tn_splits * c->slab_mt[j] * 64 * c->slab_nt[j] * 64);
    };
    c->slab.resize(K + 2, nullptr);
    c->slab_mt.resize(K + 2, 0);
    c->slab_nt.resize(K + 2, 0);
    c->slab_mv.resize(K + 2, 0);
    c->slab_nv.resize(K + 2, 0);
    if ((rc = mkslab(0, c->Stot_x, Dp))) return rc;
    for (int j = 1; j <= K; ++j)
      if ((rc = mkslab(j, c->Wp[j], c->Wp[j - 1] + (c->has_v ? 0 : 1)))) return rc;
    if ((rc = mkslab(K + 1, 16, c->Wp[K] + 1))) return rc;  // output layer: [w_out | b_out]

    auto slabsum = [&](int j, int r0, int c0, int rows, int cols, float* dst, int dst_ld, float scale) {
      const int ld = c->slab_nt[j] * 64;
      PackDesc d = mk_desc(c->slab[j] + (size_t)r0 * ld + c0, ld, dst, dst_ld, rows, cols, 0, PK_SLABSUM, scale);
      d.nslab = c->tn_splits;
      d.slab_stride = (long long)c->slab_mt[j] * 64 * ld;
      F.push_back(d);
    };
    slabsum(0, 0, 0, c->in.out, D + 1, gtag(c->in.w), D + 1, 1.f);
    slabsum(0, 0, D + 1, c->in.out, 1, gtag(c->in.b), 1, 1.f);
    if (c->has_v)
      for (int j = 1; j <= K; ++j) {
        const Lin& v = c->V[j - 1];
        slabsum(0, c->col[j], 0, v.out, D + 1, gtag(v.w), D + 1, 1.f);
        slabsum(0, c->col[j], D + 1, v.out, 1, gtag(v.b), 1, 1.f);
        slabsum(0, c->col[j], D + 1, v.out, 1, gtag(c->B[j - 1].b), 1, 1.f);
      }
    for (int j = 1; j <= K; ++j) {
      const Lin& b = c->B[j - 1];
      if (c->proj) {
        slabsum(j, 0, 0, b.out, b.in, c->abar[j], LW, -1.f);  // Abar = -Bbar
        F.back().dotR = c->rtr[j];
        F.back().dot_part = c->dot_part + (size_t)(j - 1) * c->dot_nblk;
      } else {
        slabsum(j, 0, 0, b.out, b.in, gtag(b.w), b.in, 1.f);
        slabsum(j, 0, c->Wp[j - 1], b.out, 1, gtag(b.b), 1, 1.f);
      }
    }
    slabsum(K + 1, 0, 0, 1, c->out.in, gtag(c->out.w), 1, 1.f);
    slabsum(K + 1, 0, c->Wp[K], 1, 1, gtag(c->out.b), 1, 1.f);
  }
  if (c->mode == DBSDE_MODE_NAIS_NET) {
    // Q6: input_layers[K] never receives a gradient; its slots are written as
    // zeros here so the gradient buffer needs no clearing memset
    const long long tail = (long long)c->L[c->cfg.n_layers - 2] * c->L[0] + c->L[c->cfg.n_layers - 2];
    PackDesc d = mk_desc(gtag(c->nparams - tail), 1, gtag(c->nparams - tail), (int)tail, 1, (int)tail, 0,
                         PK_SLABSUM, 1.f);
    d.nslab = 0;
    F.push_back(d);
  }
  c->n_fin = (int)F.size();
  c->fin_blocks = 1;
  for (const PackDesc& d : F) c->fin_blocks = std::max(c->fin_blocks, (d.rows * d.cols + 63) / 64);
  if (c->tnw) {
    // the windows of each problem tile (and, row P, the zero windows)
    TileFinTable tab{};
    const int Pn = c->tnw_P;
    if (Pn > TNW_PMAX_FIN) return fail(c, DBSDE_EINVAL, "internal: finalize table");
    for (const PackDesc& d : F) {
      const int row = d.nslab != 0 ? d.sp : Pn;
      if (row < 0 || row > Pn || tab.n[row] >= TF_WMAX) return fail(c, DBSDE_EINVAL, "internal: finalize windows");
      tab.w[row][tab.n[row]++] = d;
    }
    if ((rc = dalloc_t(c, &c->d_fintab, 1))) return rc;
    HIPC(c, hipMemcpy(c->d_fintab, &tab, sizeof(tab), hipMemcpyHostToDevice));
  }
  if ((rc = dalloc_t(c, &c->d_prep, P.size()))) return rc;
  c->n_prepz = (int)PZ.size();
  if (c->n_prepz) {
    for (const PackDesc& d : PZ) c->prepz_blocks = std::max(c->prepz_blocks, (d.rows * d.cols + 255) / 256);
    if ((rc = dalloc_t(c, &c->d_prepz, PZ.size()))) return rc;
    HIPC(c, hipMemcpy(c->d_prepz, PZ.data(), PZ.size() * sizeof(PackDesc), hipMemcpyHostToDevice));
  }
  c->n_prepj = (int)PJ.size();
  if (c->n_prepj) {
    for (const PackDesc& d : PJ) c->prepj_blocks = std::max(c->prepj_blocks, (d.rows * d.cols + 255) / 256);
    if ((rc = dalloc_t(c, &c->d_prepj, PJ.size()))) return rc;
    HIPC(c, hipMemcpy(c->d_prepj, PJ.data(), PJ.size() * sizeof(PackDesc), hipMemcpyHostToDevice));
  }
  if ((rc = dalloc_t(c, &c->d_fin, F.size()))) return rc;
  // descriptors are stored with tagged pointers; the kernel arguments carry the
  // real params/grad bases (pack_kernel_tagged below).
  HIPC(c, hipMemcpy(c->d_prep, P.data(), P.size() * sizeof(PackDesc), hipMemcpyHostToDevice));
  HIPC(c, hipMemcpy(c->d_fin, F.data(), F.size() * sizeof(PackDesc), hipMemcpyHostToDevice));
  return DBSDE_OK;
}

}  // namespace

int ensure_rows(dbsde_ctx* c, int Rp, int N) {
  if (Rp <= c->cap_rows && N <= c->cap_n) return DBSDE_OK;
  const int nr = std::max(Rp, c->cap_rows), nn = std::max(N, c->cap_n);
  if (!c->row_allocs.empty()) {
    HIPC(c, hipStreamSynchronize(c->stream));
    if (c->ps.pf_stream) HIPC(c, hipStreamSynchronize(c->ps.pf_stream));
    if (c->pipe2) HIPC(c, hipStreamSynchronize(c->pipe2));
    c->ps.clear();
    for (void* p : c->row_allocs) {
      (void)hipFree(p);
      c->allocs.erase(std::find(c->allocs.begin(), c->allocs.end(), p));
    }
    c->row_allocs.clear();
  }
  const size_t first = c->allocs.size();
  const size_t R = nr;
  int rc;
  const int ldx = c->Dp, S = c->Stot;
  for (int i = 0; i < 2; ++i) {
    if ((rc = dalloc_t(c, &c->ps.xin_b[i], R * ldx))) return rc;
    if ((rc = dalloc_t(c, &c->ps.sdw_b[i], R * ldx))) return rc;
  }
  c->ps.cur = 0;
  c->xin = c->ps.xin_b[0];
  c->sdw = c->ps.sdw_b[0];
  if ((rc = dalloc_t(c, &c->zbar, R * ldx))) return rc;
  if ((rc = dalloc_t(c, &c->zfull, R * ldx))) return rc;
  if ((rc = dalloc_t(c, &c->Abuf, R * S))) return rc;
  if ((rc = dalloc_t(c, &c->Adot, R * S))) return rc;
  if ((rc = dalloc_t(c, &c->Delta, R * S))) return rc;
  if ((rc = dalloc_t(c, &c->Alpha, R * S))) return rc;
  if ((rc = dalloc_t(c, &c->H, R * S))) return rc;
  if ((rc = dalloc_t(c, &c->Hdot, R * S))) return rc;
  if ((rc = dalloc_t(c, &c->G, R * S))) return rc;
  if ((rc = dalloc_t(c, &c->Pbuf[0], R * c->Wmax))) return rc;
  if ((rc = dalloc_t(c, &c->Pbuf[1], R * c->Wmax))) return rc;
  if ((rc = dalloc_t(c, &c->u, R + 64))) return rc;
  if ((rc = dalloc_t(c, &c->rres, R))) return rc;
  if ((rc = dalloc_t(c, &c->lossrow, R))) return rc;
  if (c->cfg.problem.pen != 0.f && (rc = dalloc_t(c, &c->dphidy, R))) return rc;
  if ((rc = dalloc_t(c, &c->ubar, R))) return rc;
  if ((rc = dalloc_t(c, &c->umask, R))) return rc;
  if ((rc = dalloc_t(c, &c->u16, R * 16))) return rc;
  if ((rc = dalloc_t(c, &c->o16, R * 16))) return rc;
  if ((rc = fill_col0(c, c->o16, 16, (long long)R, 1.f))) return rc;
  if ((rc = dalloc_t(c, &c->loss_part, R / 16 + 2))) return rc;
  if ((rc = dalloc_t(c, &c->rowsum, R * 8))) return rc;
  if ((rc = dalloc_t(c, &c->loss_tmp, 16))) return rc;
  if ((rc = dalloc_t(c, &c->q3S, (size_t)nn + 1))) return rc;
  c->row_allocs.assign(c->allocs.begin() + first, c->allocs.end());
  c->cap_rows = nr;
  c->cap_n = nn;
  return DBSDE_OK;
}

extern "C" {

int dbsde_abi_version(void) { return DBSDE_ABI_VERSION; }

int dbsde_matrix_form(const dbsde_ctx* c) {
  if (!c) return 0;
  // bit 1: the wave-tile weight-gradient kernel in split-bf16 form, or the
  // chain layouts' weight-gradient tiles (tnx3.hpp, split-bf16 with x3chain)
  const bool tn_x3 = c->tnw ? c->tnw_x3 : c->tnx3;
  return (c->x3 ? 1 : 0) | (tn_x3 ? 2 : 0) | (c->x3chain ? 4 : 0);
}

const char* dbsde_last_error(const dbsde_ctx* ctx) {
  if (ctx && !ctx->err.empty()) return ctx->err.c_str();
  return g_last_error.c_str();
}

int dbsde_create(const dbsde_config* cfg, dbsde_ctx** out) {
  if (!cfg || !out) return fail(nullptr, DBSDE_EINVAL, "cfg/out is NULL");
  *out = nullptr;
  dbsde_ctx* c = new dbsde_ctx();
  c->cfg = *cfg;
  c->device = cfg->device;
  int rc = build_net(c);
  if (!rc) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) rc = fail(c, DBSDE_EHIP, "no HIP device available");
    else if (cfg->device < 0 || cfg->device >= ndev) rc = fail(c, DBSDE_EINVAL, "bad device ordinal");
    else if ((e = hipSetDevice(cfg->device)) != hipSuccess) rc = fail(c, DBSDE_EHIP, hipGetErrorString(e));
    else if ((e = hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, cfg->device)) != hipSuccess)
      rc = fail(c, DBSDE_EHIP, hipGetErrorString(e));
    if (const char* ec = getenv("DBSDE_CHUNKS")) c->chunks = std::max(0, atoi(ec));
    if (const char* ej = getenv("DBSDE_JET_CAP")) c->jet_cap = std::max(16, atoi(ej));
  }
  if (!rc) rc = build_buffers(c);
  if (!rc) {
    hipError_t e = hipStreamCreateWithFlags(&c->pipe2, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
      e = hipEventCreateWithFlags(&c->ev_pipe[i], DBSDE_EVF);
      if (e == hipSuccess) e = hipEventCreate(&c->ev_prof[i]);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->ps.pf_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_pf_order, DBSDE_EVF);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_switch, DBSDE_EVF);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&c->ps.pend[i].ready, DBSDE_EVF);
    if (e != hipSuccess) rc = fail(c, DBSDE_EHIP, std::string("side stream: ") + hipGetErrorString(e));
    int wv = 0;
    if (!rc && DBSDE_MEMOPS && !order_by_events() &&
        hipDeviceGetAttribute(&wv, hipDeviceAttributeCanUseStreamWaitValue, c->device) == hipSuccess && wv)
      c->memops = (rc = dalloc_t(c, &c->d_order, 8)) == DBSDE_OK;
    if (!rc) log_ordering(c->memops);
  }
  if (rc) {
    g_last_error = c->err;
    dbsde_destroy(c);
    return rc;
  }
  // (dbsde_last_error(NULL) is the message of the last FAILED call without a
  // context: a context that exists has none, so an earlier refusal's text must
  // not read as this call's)
  g_last_error.clear();
  *out = c;
  return DBSDE_OK;
}

void dbsde_destroy(dbsde_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->pipe2) (void)hipStreamSynchronize(c->pipe2);
  if (c->ps.pf_stream) {
    (void)hipStreamSynchronize(c->ps.pf_stream);
    (void)hipStreamDestroy(c->ps.pf_stream);
  }
  if (c->ev_pf_order) (void)hipEventDestroy(c->ev_pf_order);
  if (c->ev_switch) (void)hipEventDestroy(c->ev_switch);
  for (int i = 0; i < 2; ++i) {
    if (c->ps.pend[i].ready) (void)hipEventDestroy(c->ps.pend[i].ready);
    if (c->ev_pipe[i]) (void)hipEventDestroy(c->ev_pipe[i]);
    if (c->ev_prof[i]) (void)hipEventDestroy(c->ev_prof[i]);
  }
  if (c->pipe2) (void)hipStreamDestroy(c->pipe2);
  for (auto& r : c->pending) {
    c->ev_pool.push_back(r.e0);
    c->ev_pool.push_back(r.e1);
  }
  for (auto e : c->ev_pool) (void)hipEventDestroy(e);
  for (void* p : c->allocs) (void)hipFree(p);
  delete c;
}

int dbsde_set_stream(dbsde_ctx* c, void* s) {
  if (!c) return fail(nullptr, DBSDE_EINVAL, "ctx is NULL");
  const hipStream_t ns = (hipStream_t)s;
  if (ns != c->stream && c->ev_switch) {
    // the context's workspace (row buffers, pending rollouts, slabs) is
    // written by the work already queued on the old stream: the new stream
    // starts after it, so a caller may switch streams between calls without
    // ordering them itself (no cost while the stream stays the same)
    HIPC(c, hipSetDevice(c->device));
    const int rc = stream_order(c, c->stream, ns, ORD_SWITCH);
    if (rc) return rc;
  }
  c->stream = ns;
  return DBSDE_OK;
}

int dbsde_stream_order_by_events(const char* const* env) { return events_reason(env) ? 1 : 0; }

long long dbsde_param_count(const dbsde_ctx* c) { return c ? c->nparams : -1; }

int dbsde_param_used_mask(const dbsde_ctx* c, unsigned char* mask, long long n) {
  if (!c || !mask || n != c->nparams) return fail(nullptr, DBSDE_EINVAL, "bad mask buffer");
  memcpy(mask, c->used.data(), (size_t)n);
  return DBSDE_OK;
}

}  // extern "C"

extern "C" {

int dbsde_profile_enable(dbsde_ctx* c, int enable) {
  if (!c) c = free_call_ctx();
  c->prof = enable != 0;
  return DBSDE_OK;
}

static int collect(dbsde_ctx* c) {
  if (c->pending.empty()) return DBSDE_OK;
  HIPC(c, hipStreamSynchronize(c->stream));
  for (auto& r : c->pending) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.e0, r.e1);
    ProfAgg& a = c->agg[r.id];
    a.ms += ms;
    a.flops += r.flops;
    a.bytes += r.bytes;
    a.n += 1;
    c->ev_pool.push_back(r.e0);
    c->ev_pool.push_back(r.e1);
  }
  c->pending.clear();
  return DBSDE_OK;
}

int dbsde_profile_count(dbsde_ctx* c) {
  if (!c) c = free_call_ctx();
  int rc = collect(c);
  if (rc) return rc;
  return (int)c->agg.size();
}

int dbsde_profile_read(dbsde_ctx* c, int idx, char* name, int name_len, double* total_ms, double* flops,
                       double* bytes, long long* launches) {
  if (!c) c = free_call_ctx();
  int rc = collect(c);
  if (rc) return rc;
  if (idx < 0 || idx >= (int)c->agg.size()) return fail(c, DBSDE_EINVAL, "profile index out of range");
  const ProfAgg& a = c->agg[idx];
  if (name && name_len > 0) {
    strncpy(name, a.name.c_str(), name_len - 1);
    name[name_len - 1] = 0;
  }
  if (total_ms) *total_ms = a.ms;
  if (flops) *flops = a.flops;
  if (bytes) *bytes = a.bytes;
  if (launches) *launches = a.n;
  return DBSDE_OK;
}

int dbsde_profile_reset(dbsde_ctx* c) {
  if (!c) c = free_call_ctx();
  int rc = collect(c);
  if (rc) return rc;
  for (auto& a : c->agg) {
    a.ms = a.flops = a.bytes = 0;
    a.n = 0;
  }
  return DBSDE_OK;
}

}  // extern "C"
