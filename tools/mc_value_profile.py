"""dbsde_mc_value at surface size: P = 51 points, mc = 65536 samples, 50 steps,
for BSB D = 100 (value only, and with the pathwise delta), config 3's
correlated basket (D = 100) and config 5's Heston (k = 50).  Each call is timed
with HIP events: the median of 10 calls after 2 warm-ups; the rate is (point,
sample, step) triples per second.  Needs a GPU.
    python tools/mc_value_profile.py [out.json]   (default profiles/mc_value_times.json)"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mc_value_times.json")
pkg = importlib.import_module("deep-neural-network-solutions-for-partial-differential-equations_amd")
dev = torch.device("cuda:0")
P, MC, N, D, K = 51, 65536, 50, 100, 50
WARM, CALLS = 2, 10

S = pkg.ProblemSpec
np.random.seed(0)
L = np.linalg.cholesky(pkg.FBSNN._random_corr(D, False)).astype(np.float32)
scale = np.linspace(0.5, 1.5, P, dtype=np.float32)[:, None]        # a 51-point moneyness surface at t = 0
t = torch.zeros(P, device=dev)
Xd = torch.from_numpy(scale * np.ones((1, D), np.float32)).to(dev)
Xh = torch.from_numpy(np.concatenate([scale * np.ones((1, K), np.float32), np.full((P, K), 0.2, np.float32)], 1)).to(dev)
cases = {
    "bsb_D100": dict(spec=S(sig_a=0.4, phi_r=0.05, phi_c=1.0, g="sumsq"), X=Xd),
    "bsb_D100_delta": dict(spec=S(sig_a=0.4, phi_r=0.05, phi_c=1.0, g="sumsq"), X=Xd, delta=True),
    "basket_D100_corr": dict(spec=S(mu_a=0.05, sig_a=0.20, phi_r=0.05, g="call_mean", strike=1.0), X=Xd, L=L),
    "heston_k50": dict(spec=S(kind="heston", mu_a=0.05, phi_r=0.05, g="call_mean", strike=1.0, g_alpha=10.0, g_cols=K,
                              u_clamp=True, q3=False, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8), X=Xh),
}
out = {"shape": dict(P=P, mc=MC, n_steps=N, warmups=WARM, calls=CALLS), "cases": {}}
for name, c in cases.items():
    def call():
        return pkg.mc_value(c["spec"], t, c["X"], 1.0, N, mc=MC, seed=1, L=c.get("L"), delta=c.get("delta", False))
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        v, e, d = call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    out["cases"][name] = dict(ms_median=med, ms_min=float(min(ms)), ms_max=float(max(ms)),
                              triples_per_s=P * MC * N / (med * 1e-3),
                              value_mid=float(v[P // 2, 0]), stderr_mid=float(e[P // 2, 0]),
                              finite=bool(torch.isfinite(v).all() and (d is None or torch.isfinite(d).all())))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
print(json.dumps(out, indent=1))
