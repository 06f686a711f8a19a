"""Timings of the geometric-average Asian problem (ProblemSpec(average="geometric"),
DBSDE_PROB_GEO_ASIAN: rollout_asian_chain_kernel + the geometric instance of
rollout_asian_avg_kernel) beside the arithmetic-average problem (kind 4) of the
same shape in one session.  Needs a GPU.

  * steps: GeometricAsianBasketCallOption and AsianBasketCallOption at k = 100
    assets (D = 101), NAIS-Net 4x110 Sine, M = 1024, N = 50, Adam, device mode;
    medians of 20 event-timed device steps after 5 warm-ups, prefetched and
    in-step;
  * rollout: forward-only device-mode calls under the library's profiler: the
    S-chain and the averaging launch of both problems at k = 100, each with its
    algorithmic bytes over time against the MI355X HBM peak (8 TB/s); the
    geometric averaging launch takes one fp64 log per (row, asset) and one fp64
    exp per row on top of the arithmetic one's loads and adds;
  * mc_value: one call at P = 51 points, mc = 65536, 50 steps at k = 100 (value
    only, and with the pathwise delta) of both problems; the median of 10
    event-timed calls after 2 warm-ups.  The geometric comparator takes one
    fp64 log per (sample, asset, step) (and one fp32 division with the delta).
    python tools/geo_asian_profile.py [out.json] [commit]   (default profiles/geo_asian_times.json)"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "geo_asian_times.json")
COMMIT = sys.argv[2] if len(sys.argv) > 2 else None
M, N, K, WARM, STEPS = 1024, 50, 100, 5, 20
HBM_BPS = 8.0e12

pkg = importlib.import_module("deep-neural-network-solutions-for-partial-differential-equations_amd")
dev = torch.device("cuda:0")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def step_case(make, prefetch):
    torch.manual_seed(0)
    np.random.seed(0)
    m = make()
    opt = m.new_optimizer_state("Adam", 1e-3)
    it = [0]

    def step():
        m.device_step(opt, seed=it[0], next_seed=it[0] + 1 if prefetch else None)
        it[0] += 1

    for _ in range(WARM):
        step()
    torch.cuda.synchronize()
    ms = [timed(step) for _ in range(STEPS)]
    m.solver.prefetch_drop()
    loss = float(m._gradbuf[-1])
    return dict(state_dim=m.state_dim, brownian_dim=m.solver.nb, prefetched=prefetch, matrix_form=m.solver.matrix_form,
                ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)),
                path_steps_per_s=M * N / (np.median(ms) * 1e-3), last_loss=loss, finite=bool(np.isfinite(loss)))


def launches(spec, D, xi, names):
    """Per-launch time of the named profile rows of forward-only device-mode calls."""
    s = pkg.NativeSolver("NAIS-Net", [D + 1, 16, 16, 16, 16, 1], "Sine", spec, 1.0, dev)
    params = torch.zeros(s.nparams, device=dev)
    Xi = torch.as_tensor(xi, dtype=torch.float32).to(dev)
    loss = torch.empty(1, device=dev)
    for i in range(WARM):
        s.loss_grad(params, M, N, Xi, seed=i, loss=loss)
    s.profile(True)
    s.profile_reset()
    for i in range(10):
        s.loss_grad(params, M, N, Xi, seed=100 + i, loss=loss)
    torch.cuda.synchronize()
    rows = s.profile_read()
    s.profile(False)
    out = {}
    for name in names:
        v = rows[name]
        us, mbyte = 1e3 * v["ms"] / v["launches"], v["bytes"] / v["launches"] / 1e6
        bw = mbyte * 1e6 / (us * 1e-6)
        out[name] = dict(us=us, mbyte=mbyte, gbyte_per_s=bw / 1e9, hbm_fraction=bw / HBM_BPS)
    return out


def call_times(fn, warm=2, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = [timed(fn) for _ in range(reps)]
    return dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)))


LAYERS = 4 * [110] + [1]
res = {"commit": COMMIT,
       "shape": dict(k=K, M=M, N=N, hidden="4 x 110", mode="NAIS-Net", activation="Sine", optimizer="Adam", warmups=WARM,
                     steps=STEPS),
       "peaks": dict(hbm_bytes_per_s=HBM_BPS), "steps": {}, "rollout": {}, "mc_value": {}}

asian = pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, g="call_mean", strike=1.0, g_cols=1, q3=False, average=True)
geo = pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, g="call_mean", strike=1.0, g_cols=1, q3=False, average="geometric")
res["rollout"]["geo_asian_k100"] = launches(geo, K + 1, np.ones(K + 1), ("asian_chain", "geo_asian_avg"))
res["rollout"]["asian_k100"] = launches(asian, K + 1, np.concatenate([[0.0], np.ones(K)]), ("asian_chain", "asian_avg"))
for name, rows in res["rollout"].items():
    print(f"rollout {name}: " + ", ".join(f"{n} {v['us']:.1f} us ({100 * v['hbm_fraction']:.1f}% HBM)" for n, v in rows.items()),
          file=sys.stderr, flush=True)

makers = {
    "geo_asian_k100": lambda: pkg.GeometricAsianBasketCallOption(np.ones((1, K)), 1.0, M, N, K, None, [K + 1] + LAYERS,
                                                                 "NAIS-Net", "Sine", device=dev),
    "asian_k100": lambda: pkg.AsianBasketCallOption(np.ones((1, K)), 1.0, M, N, K, None, [K + 1] + LAYERS, "NAIS-Net", "Sine",
                                                    device=dev),
}
for name, make in makers.items():
    for prefetch in (True, False):
        key = name + ("_prefetched" if prefetch else "_in_step")
        res["steps"][key] = step_case(make, prefetch)
        print(f"step {key}: {res['steps'][key]['ms_median']:.3f} ms", file=sys.stderr, flush=True)

P, MC, STEPS_MC = 51, 65536, 50
rs = np.random.RandomState(0)
tm = torch.tensor(np.linspace(0.0, 0.9, P), dtype=torch.float32, device=dev)
Xa = torch.tensor(np.concatenate([np.linspace(0.0, 0.9, P)[:, None], rs.uniform(0.8, 1.3, (P, K))], 1), dtype=torch.float32,
                  device=dev)
Xg = Xa.clone()
Xg[:, 0] = 1.0
cases = {"geo_asian_k100": (geo, Xg, False), "geo_asian_k100_delta": (geo, Xg, True), "asian_k100": (asian, Xa, False),
         "asian_k100_delta": (asian, Xa, True)}
for name, (sp, X, delta) in cases.items():
    res["mc_value"][name] = dict(P=P, mc=MC, n_steps=STEPS_MC, **call_times(
        lambda: pkg.mc_value(sp, tm, X, 1.0, STEPS_MC, mc=MC, seed=1, delta=delta)))
    print(f"mc_value {name}: {res['mc_value'][name]['ms_median']:.3f} ms", file=sys.stderr, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(res, open(OUT, "w"), indent=1)
print(json.dumps(res, indent=1))
