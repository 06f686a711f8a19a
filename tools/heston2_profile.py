"""Timings of the two-factor Heston problem (problem kind "heston2": two
Brownian motions per asset, rollout_heston2_kernel) beside the one-factor kind
of the reference ("heston", rollout_heston_kernel) in one session.  Needs a GPU.

  * step: 50 assets, Naisnet 4x110 Sine, M = 1024, N = 100, Adam, device mode;
    medians of 20 event-timed device steps after 5 warm-ups; arms kind 2 /
    kind 1 x prefetched / in-step;
  * rollout: forward-only device-mode calls under the library's profiler at
    k = 50: the rollout launch of each kind with its algorithmic bytes (the
    xin and sdw rows: 2 x 4 x 2k bytes per path step) over time against the
    MI355X HBM peak (8 TB/s), and its 4-byte row stores per second; the
    two-factor kernel at DBSDE_H2_THREADS = 64, 128 and 256 (the default),
    each in a process of its own (the variable is read once);
  * closed_form: one exact("heston") call at R = 1024 points of its stated
    domain, and mc_value: one call at k = 1, P = 8, mc = 65536, N = 100; each the
    median of 20 event-timed calls after 3 warm-ups.
    python tools/heston2_profile.py [out.json] [commit]   (default profiles/heston2_times.json)"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD = len(sys.argv) > 1 and sys.argv[1] == "--launches"
OUT = sys.argv[1] if len(sys.argv) > 1 and not CHILD else os.path.join(ROOT, "profiles", "heston2_times.json")
COMMIT = (sys.argv[2] if len(sys.argv) > 2 and not CHILD else None) or None
M, N, K, WARM, STEPS = 1024, 100, 50, 5, 20
HBM_BPS = 8.0e12
HESTON = dict(kappa=2.0, theta=0.2, sigma=0.3, rho=0.8)

pkg = importlib.import_module("deep-neural-network-solutions-for-partial-differential-equations_amd")
dev = torch.device("cuda:0")


def spec(kind, k):
    return pkg.ProblemSpec(kind=kind, mu_a=0.05, phi_r=0.05, g="call_mean", strike=1.0, g_alpha=10.0, g_cols=k,
                           u_clamp=True, q3=False, **HESTON)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def launches(k=K):
    """Per-launch time of each kind's rollout alone: forward-only calls."""
    out = {}
    for kind in ("heston2", "heston"):
        s = pkg.NativeSolver("Naisnet", [1 + 2 * k, 16, 16, 16, 16, 1], "Sine", spec(kind, k), 1.0, dev)
        params = torch.zeros(s.nparams, device=dev)
        Xi = torch.cat([torch.ones(k), torch.full((k,), 0.2)]).to(dev)
        loss = torch.empty(1, device=dev)
        for i in range(WARM):
            s.loss_grad(params, M, N, Xi, seed=i, loss=loss)
        s.profile(True)
        s.profile_reset()
        for i in range(10):
            s.loss_grad(params, M, N, Xi, seed=100 + i, loss=loss)
        torch.cuda.synchronize()
        v = s.profile_read()["rollout"]
        s.profile(False)
        us, mbyte = 1e3 * v["ms"] / v["launches"], v["bytes"] / v["launches"] / 1e6
        bw = mbyte * 1e6 / (us * 1e-6)
        out[kind] = dict(us=us, mbyte=mbyte, gbyte_per_s=bw / 1e9, hbm_fraction=bw / HBM_BPS,
                         row_stores_per_s=4.0 * M * (N + 1) * k / (us * 1e-6), brownian_dim=s.nb)
    return out


if CHILD:
    print(json.dumps(launches()))
    sys.exit(0)


def step_case(cls, prefetch, k=K):
    torch.manual_seed(0)
    np.random.seed(0)
    m = cls(np.ones((1, k)), 1.0, M, N, k, None, [k + 1] + 4 * [110] + [1], "Naisnet", "Sine", device=dev)
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
    return dict(kind=m.spec.kind, prefetched=prefetch, matrix_form=m.solver.matrix_form, ms_median=float(np.median(ms)),
                ms_min=float(np.min(ms)), ms_max=float(np.max(ms)), path_steps_per_s=M * N / (np.median(ms) * 1e-3),
                last_loss=loss, finite=bool(np.isfinite(loss)))


def call_times(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = [timed(fn) for _ in range(reps)]
    return dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)))


res = {"commit": COMMIT,
       "shape": dict(k=K, M=M, N=N, layers="[101, 110, 110, 110, 110, 1]", mode="Naisnet", activation="Sine",
                     optimizer="Adam", warmups=WARM, steps=STEPS),
       "peaks": dict(hbm_bytes_per_s=HBM_BPS), "steps": {}, "rollout": {}}
for ht in (64, 128, 256):               # the workgroup-size arms first, each a process of its own
    env = dict(os.environ, DBSDE_H2_THREADS=str(ht))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches"], env=env, capture_output=True,
                       text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(f"launch profile at DBSDE_H2_THREADS={ht} failed (exit {r.returncode})")
    res["rollout"][f"h2_threads_{ht}"] = json.loads(r.stdout.strip().split("\n")[-1])
    print(f"rollout h2_threads={ht}: " + ", ".join(f"{n} {v['us']:.1f} us ({100 * v['hbm_fraction']:.1f}% HBM)"
                                                    for n, v in res["rollout"][f"h2_threads_{ht}"].items()),
          file=sys.stderr, flush=True)
for cls in (pkg.HestonTwoFactorFBSNN, pkg.HestonFBSNN):
    for prefetch in (True, False):
        name = ("heston2" if cls is pkg.HestonTwoFactorFBSNN else "heston") + ("_prefetched" if prefetch else "_in_step")
        res["steps"][name] = step_case(cls, prefetch)
        print(f"step {name}: {res['steps'][name]['ms_median']:.3f} ms", file=sys.stderr, flush=True)

rs = np.random.RandomState(0)
R = 1024
X = torch.tensor(np.stack([rs.uniform(0.5, 2.0, R), rs.uniform(0.01, 1.0, R)], 1), dtype=torch.float32, device=dev)
t = torch.tensor(2.0 - rs.uniform(0.05, 2.0, R), dtype=torch.float32, device=dev)
res["closed_form"] = dict(R=R, T=2.0, **call_times(lambda: pkg.exact("heston", t, X, 2.0, (0.05, 1.0, 2.0, 0.2, 0.3, 0.8))))
P = 8
Xm = torch.tensor(np.stack([np.linspace(0.8, 1.2, P), np.full(P, 0.2)], 1), dtype=torch.float32, device=dev)
tm = torch.zeros(P, device=dev)
for kind in ("heston2", "heston"):
    res[f"mc_value_{kind}"] = dict(k=1, P=P, mc=65536, n_steps=N, **call_times(
        lambda: pkg.mc_value(spec(kind, 1), tm, Xm, 1.0, N, mc=65536, seed=1)))
print(f"closed_form R={R}: {res['closed_form']['ms_median']:.3f} ms; mc_value: "
      f"{res['mc_value_heston2']['ms_median']:.3f} ms (kind 1: {res['mc_value_heston']['ms_median']:.3f} ms)",
      file=sys.stderr, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(res, open(OUT, "w"), indent=1)
print(json.dumps(res, indent=1))
