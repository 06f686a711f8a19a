"""NumPy restatement of dbsde_mc_value (csrc/mc.hip, include/dbsde.h) -- test
infrastructure only.

The Feynman-Kac Monte-Carlo value of a linear problem on the device's own
draws: the increments of point p are oracle.philox.increments(seed, offset, 0,
mc, n_steps, nb, tau_p, L) (the same normals for every point), the paths come
from oracle.philox.rollout with mu_a = mu_eff = fp32(mu_a + phi_r phi_c) (or
heston_rollout) in float32 on the grid fp32(fp64 cumsum of tau_p / n_steps),
and g, dg/dX and the sums are float64 on those float32 paths:

  value[p]    = exp(-phi_r tau_p) mean_k g(X_T)
  stderr[p]   = exp(-phi_r tau_p) std_k(g, ddof = 1) / sqrt(mc)      (0 for mc = 1)
  delta[p, d] = exp(-phi_r tau_p) mean_k dg/dX_d(X_T) J_d            (diag only)

with J the tangent of the Euler step, J <- (J + (mu_eff J) dt) + (sig_a J) dW_d,
J_0 = 1, in float32.  tau_p <= 0 returns g(x_p), 0 and dg/dx_p.
"""
from __future__ import annotations

import numpy as np

from oracle import philox as ph

f32 = np.float32
AMBIGUOUS = 2e-5   # |a| below this: the call indicator may differ between the device's and the fp64 normals
                   # (ten times the 2e-6 normal error csrc/philox.hpp documents)


def mu_eff(spec):
    return f32(f32(spec.mu_a) + f32(f32(spec.phi_r) * f32(spec.phi_c)))


def g_cols(spec, D):
    return spec.g_cols if 0 < spec.g_cols < D else D


def payoff(spec, X):
    """g [M], dg/dX [M, D] and the kink variable a [M] (None for smooth g) in
    float64 at the rows of X; the call payoffs use 1/2 at a == 0."""
    X = np.asarray(X, np.float64)
    D = X.shape[1]
    c = g_cols(spec, D)
    Xc = X[:, :c]
    K, al = float(f32(spec.strike)), float(f32(spec.g_alpha))
    dg = np.zeros_like(X)
    a = None
    if spec.g == "sumsq":
        g = np.sum(Xc * Xc, 1)
        dg[:, :c] = 2.0 * Xc
    elif spec.g == "log":
        q = 0.5 + 0.5 * np.sum(Xc * Xc, 1)
        g = np.log(q)
        dg[:, :c] = Xc / q[:, None]
    elif spec.g == "smooth_call":
        a_ = np.mean(Xc, 1) - K
        s = 1.0 / (1.0 + np.exp(-al * a_))
        g = a_ * s
        dg[:, :c] = ((s + a_ * al * s * (1.0 - s)) / c)[:, None]
    elif spec.g in ("call_sum", "call_mean"):
        n = c if spec.g == "call_mean" else 1
        a = np.sum(Xc, 1) / n - K
        g = np.maximum(a, 0.0)
        dg[:, :c] = (np.where(a > 0, 1.0, np.where(a == 0, 0.5, 0.0)) / n)[:, None]
    else:
        raise ValueError(spec.g)
    return g, dg, a


def tangent(dw, tau, mu, sig_a):
    """J_T [M, D] float32 of the Euler step on the grid of ph.rollout."""
    M, N, D = dw.shape
    tg = ph.time_grid(N, tau)
    J = np.ones((M, D), f32)
    for n in range(N):
        dt = f32(tg[n + 1] - tg[n])
        J = (J + (f32(mu) * J) * dt) + (f32(sig_a) * J) * dw[:, n]
    return J


def terminal(spec, tau, x, n_steps, mc, seed, offset=0, L=None, want_J=False):
    """(X_T [mc, D] float32, J_T or None) of one point; tau a Python float holding
    the float32 time to maturity."""
    x = np.asarray(x, f32).reshape(-1)
    if spec.kind == "heston":
        k = x.size // 2
        dw = ph.increments(seed, offset, 0, mc, n_steps, k, tau)
        X, _ = ph.heston_rollout(x, dw, tau, mu_a=spec.mu_a, kappa=spec.kappa, theta=spec.theta, sigma=spec.sigma,
                                 rho=spec.rho)
        return X[:, -1], None
    dw = ph.increments(seed, offset, 0, mc, n_steps, x.size, tau, L)
    mu = mu_eff(spec)
    X = ph.rollout(x, dw, tau, mu_a=mu, sig_a=spec.sig_a, sig_b=spec.sig_b)
    return X[:, -1], (tangent(dw, tau, mu, spec.sig_a) if want_J else None)


def mc_value(spec, t, X, T, n_steps, mc, seed=0, offset=0, L=None, delta=False):
    """dict(value [P], stderr [P], delta [P, D] | None, delta_stderr [P, D] | None,
    ambiguous [P] = number of samples with |a| < AMBIGUOUS, delta_slack [P, D] =
    (sum over those samples of the kink's |dg J| magnitude) / mc)."""
    t = np.asarray(t, f32).reshape(-1)
    X = np.asarray(X, f32).reshape(t.size, -1)
    P, D = X.shape
    out = dict(value=np.zeros(P), stderr=np.zeros(P), ambiguous=np.zeros(P, int),
               delta=np.zeros((P, D)) if delta else None, delta_stderr=np.zeros((P, D)) if delta else None,
               delta_slack=np.zeros((P, D)) if delta else None)
    for p in range(P):
        tau = float(f32(T) - t[p])
        if tau <= 0:
            g, dg, _ = payoff(spec, X[p:p + 1])
            out["value"][p] = g[0]
            if delta:
                out["delta"][p] = dg[0]
            continue
        XT, J = terminal(spec, tau, X[p], n_steps, mc, seed, offset, L, want_J=delta)
        g, dg, a = payoff(spec, XT)
        disc = np.exp(-float(f32(spec.phi_r)) * tau)
        out["value"][p] = disc * np.mean(g)
        out["stderr"][p] = disc * np.std(g, ddof=1) / np.sqrt(mc) if mc > 1 else 0.0
        amb = np.abs(a) < AMBIGUOUS if a is not None else np.zeros(mc, bool)
        out["ambiguous"][p] = int(amb.sum())
        if delta:
            dj = dg * J.astype(np.float64)
            out["delta"][p] = disc * np.mean(dj, 0)
            out["delta_stderr"][p] = disc * np.std(dj, 0, ddof=1) / np.sqrt(mc) if mc > 1 else 0.0
            if a is not None:
                c = g_cols(spec, D)
                n = c if spec.g == "call_mean" else 1
                kink = np.zeros((mc, D))
                kink[:, :c] = np.abs(J[:, :c].astype(np.float64)) / n
                out["delta_slack"][p] = np.sum(kink[amb], 0) / mc
    return out


def euler_sumsq(spec, x, tau, n_steps):
    """Closed Euler expectation of the sumsq payoff for sigma = sig_a X:
    exp(-phi_r tau) |x|^2 ((1 + mu_eff dt)^2 + sig_a^2 dt)^N, and its gradient
    2 x_d times the same factor."""
    x = np.asarray(x, np.float64)
    dt = tau / n_steps
    f = np.exp(-float(f32(spec.phi_r)) * tau) * ((1.0 + float(mu_eff(spec)) * dt) ** 2
                                                  + float(f32(spec.sig_a)) ** 2 * dt) ** n_steps
    return f * np.sum(x * x), 2.0 * x * f
