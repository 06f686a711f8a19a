"""dbsde_mc_value of the correlated k-asset Heston (DBSDE_PROB_HESTON_CORR) at the
shape of tools/mc_value_profile.py's Heston row: k = 50, P = 51 points,
mc = 65536 samples, 50 steps.  One process times, with HIP events (median of 10
calls after 2 warm-ups):
  * the correlated call at the default workspace bound, and at each bound of
    WS_MB (DBSDE_MC_WS_MB is read at every call), with the number of groups;
  * the uncorrelated kind-1 call of the same session -- the yardstick;
  * the per-launch split of the correlated call (increment GEMM, path kernel)
    from the library's profile of the context-free calls, in separate calls
    (recording events around every launch is not part of the timed calls).
Needs a GPU.
    python tools/mc_heston_corr_profile.py [out.json]   (default profiles/mc_heston_corr_times.json)"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mc_heston_corr_times.json")
pkg = importlib.import_module("deep-neural-network-solutions-for-partial-differential-equations_amd")
dev = torch.device("cuda:0")
P, MC, N, K = 51, 65536, 50, 50
WARM, CALLS = 2, 10
WS_MB = ["32", "128", "256", "512"]          # against the default, which holds the whole call (625 MB)

rs = np.random.RandomState(0)                 # a random correlation matrix (unit diagonal) and its factor
A = rs.normal(size=(K, K))
C = A @ A.T + K * np.eye(K)
L = np.linalg.cholesky(C / np.sqrt(np.outer(np.diag(C), np.diag(C)))).astype(np.float32)
scale = np.linspace(0.5, 1.5, P, dtype=np.float32)[:, None]        # a 51-point moneyness surface at t = 0
t = torch.zeros(P, device=dev)
X = torch.from_numpy(np.concatenate([scale * np.ones((1, K), np.float32), np.full((P, K), 0.2, np.float32)], 1)).to(dev)
spec = pkg.ProblemSpec(kind="heston", mu_a=0.05, phi_r=0.05, g="call_mean", strike=1.0, g_alpha=10.0, g_cols=K,
                       u_clamp=True, q3=False, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8)


def call(L_):
    return pkg.mc_value(spec, t, X, 1.0, N, mc=MC, seed=1, L=L_)


def timed(L_):
    for _ in range(WARM):
        call(L_)
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        v, e, _ = call(L_)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    return dict(ms_median=med, ms_min=float(min(ms)), ms_max=float(max(ms)), triples_per_s=P * MC * N / (med * 1e-3),
                value_mid=float(v[P // 2, 0]), stderr_mid=float(e[P // 2, 0]), finite=bool(torch.isfinite(v).all())), v


def split():
    """Per-launch times of CALLS correlated calls (after the warm-ups above)."""
    pkg.free_call_profile(enable=True, reset=True)
    for _ in range(CALLS):
        call(L)
    prof = pkg.free_call_profile(enable=False)
    return {name: dict(ms_per_call=r["ms"] / CALLS, launches_per_call=r["launches"] / CALLS,
                       gflops=r["flops"] / (r["ms"] * 1e6) if r["ms"] else 0.0,
                       gbytes_per_s=r["bytes"] / (r["ms"] * 1e6) if r["ms"] else 0.0) for name, r in prof.items()}


os.environ.pop("DBSDE_MC_WS_MB", None)
out = {"shape": dict(P=P, k=K, mc=MC, n_steps=N, warmups=WARM, calls=CALLS),
       "workspace": dict(default_mb=1024, call_mb=MC * N * K * 4 / 2 ** 20), "cases": {}}
out["cases"]["heston_k50"], v_ind = timed(None)
out["cases"]["heston_corr_k50"], v_def = timed(L)
out["cases"]["heston_corr_k50"]["launches"] = split()
for mb in WS_MB:
    os.environ["DBSDE_MC_WS_MB"] = mb
    r, v = timed(L)
    r["launches"] = split()
    r["bitwise_equal_to_default"] = bool(torch.equal(v, v_def))
    out["cases"]["heston_corr_k50_ws%s" % mb] = r
os.environ.pop("DBSDE_MC_WS_MB", None)
out["ratio_corr_over_uncorrelated"] = out["cases"]["heston_corr_k50"]["ms_median"] / out["cases"]["heston_k50"]["ms_median"]
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
print(json.dumps(out, indent=1))
