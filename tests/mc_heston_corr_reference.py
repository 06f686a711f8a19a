"""NumPy restatement of dbsde_mc_value for the correlated k-asset Heston
(DBSDE_PROB_HESTON_CORR: kind "heston" with a Cholesky factor L [k, k] between
the assets' Brownian motions) -- test infrastructure only.

Terminal states: oracle.philox.increments(seed, offset, 0, mc, n_steps, k,
tau_p, L) -- the normals of the uncorrelated kind, dW = L (sqrt(dt) z) -- then
oracle.philox.heston_rollout, in float32 on the grid fp32(fp64 cumsum of
tau_p / n_steps).  Payoff, discount and standard error are
tests/mc_reference.py's.  L = None is mc_reference.mc_value's Heston branch.

product: how L . (sqrt(dt) z) is formed.  "fp64" (ph.increments: an fp64 product
rounded once) is the restatement; "fp32_chunks" sums fp32 products in 16-wide
chunks of the inner index, ascending, each chunk's partial sum added to the
running fp32 sum -- the coarsest fp32 order a 16-wide blocked product takes.
Twice the difference of the two bounds what any fp32 summation order of that
product may add to the value tolerance at large k."""
from __future__ import annotations

import numpy as np

import mc_reference as mr
from oracle import philox as ph

f32 = np.float32
HESTON = dict(mu_a=0.05, phi_r=0.05, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8)


def spec_for(pkg, k, payoff="call_mean"):
    return pkg.ProblemSpec(kind="heston", phi_c=0.0, g=payoff, strike=1.0, g_alpha=10.0, g_cols=k, u_clamp=True,
                           q3=False, **HESTON)


def equicorr_factor(k, rho):
    return np.linalg.cholesky((1 - rho) * np.eye(k) + rho * np.ones((k, k)))


def increments(seed, offset, mc, n_steps, k, tau, L, product="fp64"):
    L32 = None if L is None else np.asarray(L, f32)
    if L32 is None or product == "fp64":
        return ph.increments(seed, offset, 0, mc, n_steps, k, tau, L32)
    assert product == "fp32_chunks"
    dw = ph.increments(seed, offset, 0, mc, n_steps, k, tau)          # sqrt(dt) z, fp32
    Lt = np.tril(L32)
    out = np.zeros_like(dw)
    for c0 in range(0, k, 16):
        part = np.zeros_like(dw)
        for j in range(c0, min(c0 + 16, k)):
            part = (part + (Lt[None, None, :, j] * dw[:, :, j:j + 1]).astype(f32)).astype(f32)
        out = (out + part).astype(f32)
    return out


def terminal(spec, tau, x, n_steps, mc, seed, offset=0, L=None, product="fp64"):
    """X_T [mc, 2k] float32 of one point; tau a Python float holding the float32
    time to maturity."""
    x = np.asarray(x, f32).reshape(-1)
    k = x.size // 2
    dw = increments(seed, offset, mc, n_steps, k, tau, L, product)
    X, _ = ph.heston_rollout(x, dw, tau, mu_a=spec.mu_a, kappa=spec.kappa, theta=spec.theta, sigma=spec.sigma,
                             rho=spec.rho)
    return X[:, -1]


def mc_value(spec, t, X, T, n_steps, mc, seed=0, offset=0, L=None, product="fp64"):
    """dict(value [P], stderr [P]) as mc_reference.mc_value returns them."""
    assert spec.kind == "heston"
    t = np.asarray(t, f32).reshape(-1)
    X = np.asarray(X, f32).reshape(t.size, -1)
    out = dict(value=np.zeros(t.size), stderr=np.zeros(t.size))
    for p in range(t.size):
        tau = float(f32(T) - t[p])
        if tau <= 0:
            out["value"][p] = mr.payoff(spec, X[p:p + 1])[0][0]
            continue
        g, _, _ = mr.payoff(spec, terminal(spec, tau, X[p], n_steps, mc, seed, offset, L, product))
        disc = np.exp(-float(f32(spec.phi_r)) * tau)
        out["value"][p] = disc * np.mean(g)
        out["stderr"][p] = disc * np.std(g, ddof=1) / np.sqrt(mc) if mc > 1 else 0.0
    return out


# the case the correlation shows in: k = 8 assets, equicorrelation 0.9, S = 1,
# v = 0.2, T = 1, 10 steps, call on the mean at strike 1
GAP_K, GAP_RHO, GAP_STEPS, GAP_MC, GAP_SEED = 8, 0.9, 10, 2 ** 14, 1


def gap_point():
    return np.zeros(1, f32), np.concatenate([np.ones((1, GAP_K)), np.full((1, GAP_K), 0.2)], 1).astype(f32)


_GAP = {}


def gap_case(pkg, mc=GAP_MC):
    """(correlated, independent) restatement results of the gap case, computed
    once per process; treat them as read-only."""
    if mc not in _GAP:
        spec = spec_for(pkg, GAP_K)
        t, X = gap_point()
        L = equicorr_factor(GAP_K, GAP_RHO)
        _GAP[mc] = (mc_value(spec, t, X, 1.0, GAP_STEPS, mc, seed=GAP_SEED, L=L),
                    mc_value(spec, t, X, 1.0, GAP_STEPS, mc, seed=GAP_SEED))
    return _GAP[mc]
