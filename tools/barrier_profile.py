"""Timings of the knock-out problem (ProblemSpec(barrier=B), DBSDE_PROB_BARRIER:
the diagonal rollouts followed by rollout_barrier_stop_kernel) beside the same
problem without the barrier in one session.  Needs a GPU.

  * steps: BarrierBasketCallOption against BasketCallOption at D = 100 assets,
    NAIS-Net 4x110 Sine, M = 1024, N = 50, Adam, device mode, prefetched and
    in-step: per mode the two cases side by side, five windows of 20
    event-timed device steps per case, the cases alternating window by window
    after 5 warm-up steps each; per case the median of its five window
    medians, and every window median;
  * rollout: forward-only device-mode calls under the library's profiler: the
    diagonal two-pass rollout and the stop pass behind it, each with its
    algorithmic bytes over time against the MI355X HBM peak (8 TB/s).
    Algorithmic bytes of the stop pass: the g_cols payoff columns of every row,
    read once (4 g_cols bytes per row) -- an upper bound, a knocked path's scan
    ends at its hit row, and the rows rewritten behind it are not counted;
    beside them the fraction of paths knocked and their mean stopping row;
  * mc_value: one call at P = 51 points, mc = 65536, 50 steps of the knock-out
    problem at D = 100 beside kind DIAG's call on the same spec without the
    barrier; the median of 10 event-timed calls after 2 warm-ups;
  * exact: one call of the closed form at 1024 points.
    python tools/barrier_profile.py [out.json] [commit]   (default profiles/barrier_times.json)"""
import dataclasses
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "barrier_times.json")
COMMIT = sys.argv[2] if len(sys.argv) > 2 else None
M, N, K, WARM, STEPS, WINDOWS = 1024, 50, 100, 5, 20, 5
BARRIER = 0.99          # the mean of 100 assets from 1 moves by 0.02 sqrt(t) around a drift of 0.05 t: some 6 % of the paths are knocked
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


def stepper(make, prefetch):
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
    return m, step


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
    X = torch.empty(M * (N + 1) * D, device=dev)
    s.loss_grad(params, M, N, Xi, seed=100, loss=loss, X=X)
    torch.cuda.synchronize()
    X = X.cpu().numpy().reshape(M, N + 1, D)
    frozen = np.all(X[:, 1:] == X[:, :-1], axis=2)                      # row n + 1 repeats row n
    tau = np.where(frozen.any(1), frozen.argmax(1), N + 1)
    out["paths"] = dict(knocked_fraction=float(np.mean(tau <= N)), mean_stopping_row=float(tau[tau <= N].mean()) if np.any(tau <= N) else None)
    return out


def call_times(fn, warm=2, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = [timed(fn) for _ in range(reps)]
    return dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)))


LAYERS = 4 * [110] + [1]
res = {"commit": COMMIT,
       "shape": dict(D=K, M=M, N=N, barrier=BARRIER, hidden="4 x 110", mode="NAIS-Net", activation="Sine", optimizer="Adam",
                     warmups=WARM, steps_per_window=STEPS, windows=WINDOWS),
       "peaks": dict(hbm_bytes_per_s=HBM_BPS), "steps": {}, "rollout": {}, "mc_value": {}, "exact": {}}

diag = pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, g="call_mean", strike=1.0, q3=False)
barrier = dataclasses.replace(diag, barrier=BARRIER)
res["rollout"]["barrier_D100"] = launches(barrier, K, np.ones(K), ("rollout", "barrier_stop"))
res["rollout"]["diag_D100"] = launches(diag, K, np.ones(K), ("rollout",))
b = res["rollout"]["barrier_D100"]
b["stop_over_rollout"] = b["barrier_stop"]["us"] / b["rollout"]["us"]
for name, rows in res["rollout"].items():
    print(f"rollout {name}: " + ", ".join(f"{n} {v['us']:.1f} us ({100 * v['hbm_fraction']:.1f}% HBM)" for n, v in rows.items()
                                          if isinstance(v, dict) and "us" in v), rows.get("paths"), file=sys.stderr, flush=True)

args = (np.ones((1, K)), 1.0, M, N, K, None, [K + 1] + LAYERS, "NAIS-Net", "Sine")
makers = {"barrier": lambda: pkg.BarrierBasketCallOption(*args, device=dev, barrier=BARRIER),
          "basket": lambda: pkg.BasketCallOption(*args, device=dev)}
for pf in (True, False):
    # the two cases of one mode live side by side (a process has four hardware queues: more contexts would share them)
    cases = {f"{name}_{'prefetched' if pf else 'in_step'}": stepper(make, pf) for name, make in makers.items()}
    windows = {key: [] for key in cases}
    for w in range(WINDOWS):
        for key in (list(cases) if w % 2 == 0 else list(cases)[::-1]):
            step = cases[key][1]
            windows[key].append(float(np.median([timed(step) for _ in range(STEPS)])))
    for key, (m, _) in cases.items():
        m.solver.prefetch_drop()
        loss = float(m._gradbuf[-1])
        res["steps"][key] = dict(ms_median=float(np.median(windows[key])), ms_min=float(np.min(windows[key])),
                                 ms_max=float(np.max(windows[key])), window_medians=windows[key], last_loss=loss,
                                 finite=bool(np.isfinite(loss)))
        print(f"step {key}: {res['steps'][key]['ms_median']:.4f} ms {windows[key]}", file=sys.stderr, flush=True)
    del cases, m
    torch.cuda.synchronize()
for mode in ("prefetched", "in_step"):
    res["steps"][f"barrier_minus_basket_{mode}_ms"] = res["steps"][f"barrier_{mode}"]["ms_median"] - \
        res["steps"][f"basket_{mode}"]["ms_median"]

P, MC, STEPS_MC = 51, 65536, 50
rs = np.random.RandomState(0)
tm = torch.tensor(np.linspace(0.0, 0.9, P), dtype=torch.float32, device=dev)
Xd = torch.tensor(rs.uniform(0.99, 1.3, (P, K)), dtype=torch.float32, device=dev)
for name, sp in (("barrier_D100", barrier), ("diag_D100", diag)):
    res["mc_value"][name] = dict(P=P, mc=MC, n_steps=STEPS_MC, **call_times(
        lambda: pkg.mc_value(sp, tm, Xd, 1.0, STEPS_MC, mc=MC, seed=1)))
    print(f"mc_value {name}: {res['mc_value'][name]['ms_median']:.3f} ms", file=sys.stderr, flush=True)
res["mc_value"]["barrier_over_diag"] = res["mc_value"]["barrier_D100"]["ms_median"] / res["mc_value"]["diag_D100"]["ms_median"]

R = 1024
te = torch.tensor(np.linspace(0.0, 0.95, R), dtype=torch.float32, device=dev)
Xe = torch.tensor(rs.uniform(0.92, 1.5, (R, 1)), dtype=torch.float32, device=dev)
res["exact"]["barrier_call_1024"] = dict(R=R, D=1, **call_times(
    lambda: pkg.exact("barrier_call", te, Xe, 1.0, (0.05, 0.2, 1.0, 0.10, 0.9, 50.0))))
print(f"exact barrier_call: {res['exact']['barrier_call_1024']['ms_median']:.4f} ms", file=sys.stderr, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(res, open(OUT, "w"), indent=1)
print(json.dumps(res, indent=1))
