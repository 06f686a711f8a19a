"""References for the geometric-average Asian problem (problem kind 8,
DBSDE_PROB_GEO_ASIAN; ProblemSpec(kind="diag", average="geometric")) -- test
infrastructure only.

The model: state [G, S_1..S_k], Brownian dimension k, G the running geometric
average exp((1/T) int mean_i log S_i dt), G_0 = 1.  The step of include/dbsde.h,
restated, every operation rounded to fp32 on its own unless cast:

    lg_i = fp32(log(fp64(S_i)))             the arithmetic problem's row sum and mean, on lg
    a'   = a + (m dt) / T                   a_0 = lg(G_0)
    row 0 stores G_0 as given; row n >= 1 stores fp32(exp(fp64(a_n)))

  * lg, rollout: that chain in float32 numpy (the S columns are
    oracle.philox.rollout's, the row sum tests/asian_reference.py's);
  * GeoAsianProblem, loss_and_grads: tests/asian_reference.py's loss_and_grads
    with the G column advanced by the scheme's own exponential step
    G' = G exp(mean log S dt / T) in float64 (an additive Euler step on G would
    differ from the device's X by O(dt^2) per step, far above the X bound);
  * pde_terms: tests/jet_reference.py's with the drift G mean log S / T;
  * mc_value: dbsde_mc_value's restatement -- G_T = G_p exp((sum_d I_d) / (k T)),
    I_d = sum_n fp64(fp32(lg(S_{d,n}) dt_n));
  * closed_form: the continuous-time value and deltas in float64.
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

import asian_reference as ar
import jet_reference as jr
import mc_reference as mr
import put_reference as pr
from oracle import fbsnn_ref as fr
from oracle import philox as ph

f32 = np.float32
T = ar.T
N = ar.N
KS = ar.KS
MS = ar.MS
COEF = dict(mu_a=0.05, sig_a=0.20, sig_b=0.0)
R_RATE = ar.R_RATE
equicorr_L = ar.equicorr_L


def xi_state(k, G0=1.0):
    """[G, S_1..S_k] = [G0, 1..] as one row."""
    return np.concatenate([[[G0]], np.ones((1, k))], 1)


# ---------------------------------------------------------------- the fp32 chain
def lg(S):
    return np.log(np.asarray(S, f32).astype(np.float64)).astype(f32)


def gexp(a):
    return np.exp(np.asarray(a, f32).astype(np.float64)).astype(f32)


def log_average(S, dts, G0, T):
    """a = log G [M, N+1] float32 from the asset paths S [M, N+1, k]."""
    M, N1, k = S.shape
    A = np.empty((M, N1), f32)
    a = lg(np.broadcast_to(np.asarray(G0, f32).reshape(-1), (M,)))
    for n in range(N1 - 1):
        A[:, n] = a
        m = ar.row_sum(lg(S[:, n])) / f32(k)
        a = a + (m * np.asarray(dts[n], f32).reshape(-1)) / f32(T)
        assert a.dtype == f32
    A[:, N1 - 1] = a
    return A


def rollout(Xi, dw, T, mu_a=0.05, sig_a=0.20, sig_b=0.0, tgrid=None, with_log=False):
    """X [M, N+1, 1 + k] and sdw [M, N, 1 + k] float32 from increments dw
    [M, N, k] (and a = log G [M, N+1] with with_log)."""
    assert sig_b == 0.0
    M, Nn, k = dw.shape
    dw = np.asarray(dw, f32)
    x = np.broadcast_to(np.asarray(Xi, f32).reshape(-1, 1 + k), (M, 1 + k))
    S = ph.rollout(x[:, 1:], dw, T, mu_a, sig_a, sig_b, tgrid)
    a = log_average(S, ph._dts(Nn, T, tgrid), x[:, 0], T)
    G = gexp(a)
    G[:, 0] = x[:, 0]
    X = np.concatenate([G[:, :, None], S], 2)
    sdw = np.zeros((M, Nn, 1 + k), f32)
    sdw[:, :, 1:] = (f32(sig_a) * S[:, :-1]) * dw
    return (X, sdw, a) if with_log else (X, sdw)


def g_column_bound(a, G, Nn):
    """The G column's documented distance from the chain on the device's own S:
    (4 N + 2) 2^-24 max(1, |a|) G per entry."""
    return (4 * Nn + 2) * 2.0 ** -24 * np.maximum(1.0, np.abs(a.astype(np.float64))) * G.astype(np.float64)


# ---------------------------------------------------------------- the problem (torch)
class GeoAsianProblem(ar.AsianProblem):
    """tests/asian_reference.py's AsianProblem with the G drift; step() is the
    scheme's own update of the state."""

    kind = "geo_asian"

    def __init__(self, k, payoff="call_mean", strike=1.0, alpha=10.0, T=T, mu_a=0.05, sig_a=0.20, phi_r=R_RATE):
        super().__init__(k, payoff, strike, alpha, T, mu_a, sig_a, 0.0, phi_r)

    def mu(self, t, X, Y=None, Z=None):
        S = X[:, 1:]
        return torch.cat([X[:, :1] * torch.mean(torch.log(S), dim=1, keepdim=True) / self.T, self.mu_a * S], dim=1)

    def step(self, X, dt, s):
        """X_{n+1}: the S columns by Euler, G' = G exp(mean log S dt / T)."""
        S = X[:, 1:]
        G1 = X[:, :1] * torch.exp(torch.mean(torch.log(S), dim=1, keepdim=True) * dt / self.T)
        return torch.cat([G1, S + self.mu_a * S * dt + s[:, 1:]], dim=1)


def spec(pkg, payoff="call_mean", strike=1.0, **coef):
    c = dict(COEF, **coef)
    return pkg.ProblemSpec(phi_r=R_RATE, phi_c=0.0, g=payoff, strike=strike, g_alpha=10.0, g_cols=1, q3=False,
                           average="geometric", **c)


# ---------------------------------------------------------------- loss and gradient (fp64)
LOSS_SEED = ar.LOSS_SEED
LOSS_STRIKE = 1.010        # G_T is about 1.01 +- 0.07 / sqrt(k): rows on both sides of the kink (test_geo_asian_cpu.py)
LOSS_CASES = ar.LOSS_CASES
loss_layers = ar.loss_layers
loss_model = ar.loss_model


def loss_and_grads(model, prob, tgrid, dw, Xi):
    """tests/asian_reference.py's loss_and_grads (oracle.fbsnn_ref.loss_function
    in float64) with X advanced by prob.step."""
    model = copy.deepcopy(model).double()
    model.zero_grad(set_to_none=True)
    D = prob.D
    dw = torch.as_tensor(np.asarray(dw, np.float64))
    tg = torch.as_tensor(np.asarray(tgrid, np.float64))
    M, Nn, _ = dw.shape
    X0 = torch.as_tensor(np.broadcast_to(np.asarray(Xi, np.float64).reshape(-1, D), (M, D)).copy())
    X0.requires_grad_(True)
    tcol = lambda n: tg[n].expand(M, 1)
    Y0, Z0 = fr.net_u(model, tcol(0), X0)
    Xs, Ys, Zs = [X0], [Y0], [Z0]
    loss = 0
    for n in range(Nn):
        dt = tg[n + 1] - tg[n]
        s = torch.squeeze(torch.matmul(prob.sigma(tcol(n), X0, Y0), dw[:, n].unsqueeze(-1)), dim=-1)
        X1 = prob.step(X0, dt, s)
        Y1t = Y0 + prob.phi(tcol(n), X0, Y0, Z0) * dt + torch.sum(Z0 * s, dim=1, keepdim=True)
        Y1, Z1 = fr.net_u(model, tcol(n + 1), X1)
        loss = loss + torch.sum(torch.pow(Y1 - Y1t, 2))
        X0, Y0, Z0 = X1, Y1, Z1
        Xs.append(X0)
        Ys.append(Y0)
        Zs.append(Z0)
    g = prob.g(X1)
    loss = loss + torch.sum(torch.pow(Y1 - g, 2))
    dg = torch.autograd.grad(outputs=[g], inputs=[X1], grad_outputs=torch.ones_like(g), allow_unused=True,
                             retain_graph=True, create_graph=True)[0]
    loss = loss + torch.sum(torch.pow(Z1[:, :1] - dg[:, :1], 2))
    loss.backward()
    grad, mask = fr.flat_grads(model)
    return dict(loss=float(loss.detach()), X=torch.stack(Xs, 1).detach().numpy(), Y=torch.stack(Ys, 1).detach().numpy(),
                Z=torch.stack(Zs, 1).detach().numpy(), grad=np.asarray(grad, np.float64), used=mask)


# ---------------------------------------------------------------- PDE terms (fp64)
def pde_setup(k, seed=7, R=12, act="Tanh"):
    """tests/asian_reference.py's pde_setup with G in [0.8, 1.2]."""
    model, flat, t, X = ar.pde_setup(k, seed, R, act)
    X[:, 0] = (0.8 + X[:, 0] / 3.0).astype(f32).astype(np.float64)
    return model, flat, t, X


def pde_terms(model, prob, t, X, L=None):
    return jr.pde_terms(model, prob, np.asarray(t, np.float64), np.asarray(X, np.float64),
                        None if L is None else np.asarray(L, np.float64))


# ---------------------------------------------------------------- Monte-Carlo value
payoff = ar.payoff


def mc_terminal(sp, tau, x, T_, n_steps, mc, seed, offset=0, L=None, want_J=False, path0=0):
    """(G_T [mc] float64, dG_T/dS [mc, k] float64 or None) of one point on the
    device's draws: sample s is global path path0 + s."""
    x = np.asarray(x, f32).reshape(-1)
    k = x.size - 1
    dw = ph.increments(seed, offset, path0, mc, n_steps, k, tau, L)
    mu = mr.mu_eff(sp)
    S = ph.rollout(x[1:], dw, tau, mu_a=mu, sig_a=sp.sig_a, sig_b=sp.sig_b)
    tg = ph.time_grid(n_steps, tau)
    dts = [f32(tg[n + 1] - tg[n]) for n in range(n_steps)]
    I = np.zeros((mc, k))
    for n in range(n_steps):
        I += (lg(S[:, n]) * dts[n]).astype(f32).astype(np.float64)
    kT = float(k) * float(f32(T_))
    GT = float(x[0]) * np.exp(I.sum(1) / kT)
    if not want_J:
        return GT, None
    J = np.ones((mc, k), f32)
    JI = np.zeros((mc, k))
    for n in range(n_steps):
        JI += ((J / S[:, n]) * dts[n]).astype(f32).astype(np.float64)
        J = (J + (f32(mu) * J) * dts[n]) + (f32(sp.sig_a) * J) * dw[:, n]
    return GT, GT[:, None] * JI / kT


def mc_value(sp, t, X, T_, n_steps, mc, seed=0, offset=0, L=None, delta=False, chunk=1 << 13):
    """tests/asian_reference.py's mc_value for this problem: dict(value [P],
    stderr [P], delta [P, 1 + k] | None, ambiguous [P], delta_slack [P, 1 + k] |
    None, mean_GT [P])."""
    t = np.asarray(t, f32).reshape(-1)
    X = np.asarray(X, f32).reshape(t.size, -1)
    P, D = X.shape
    out = dict(value=np.zeros(P), stderr=np.zeros(P), ambiguous=np.zeros(P, int), mean_GT=np.zeros(P),
               delta=np.zeros((P, D)) if delta else None, delta_slack=np.zeros((P, D)) if delta else None)
    for p in range(P):
        tau = float(f32(T_) - t[p])
        if tau <= 0:
            g, dg, _ = payoff(sp, X[p, :1])
            out["value"][p], out["mean_GT"][p] = g[0], X[p, 0]
            if delta:
                out["delta"][p, 0] = dg[0]
            continue
        gs, dgs, Gs, Js, amb_a = [], [], [], [], []
        for k0 in range(0, mc, chunk):
            GT, JI = mc_terminal(sp, tau, X[p], T_, n_steps, min(chunk, mc - k0), seed, offset, L, want_J=delta, path0=k0)
            g, dg, a = payoff(sp, GT)
            gs.append(g)
            dgs.append(dg)
            Gs.append(GT)
            Js.append(JI)
            amb_a.append(a)
        g, dg, GT = np.concatenate(gs), np.concatenate(dgs), np.concatenate(Gs)
        disc = np.exp(-float(f32(sp.phi_r)) * tau)
        out["value"][p] = disc * np.mean(g)
        out["stderr"][p] = disc * np.std(g, ddof=1) / np.sqrt(mc) if mc > 1 else 0.0
        out["mean_GT"][p] = np.mean(GT)
        amb = np.abs(np.concatenate(amb_a)) < mr.AMBIGUOUS if amb_a[0] is not None else np.zeros(mc, bool)
        out["ambiguous"][p] = int(amb.sum())
        if delta:
            dG = np.concatenate([(GT / float(X[p, 0]))[:, None], np.concatenate(Js)], 1)   # dG_T / d[G_p, S_1..S_k]
            out["delta"][p] = disc * np.mean(dg[:, None] * dG, 0)
            if amb_a[0] is not None:
                out["delta_slack"][p] = np.sum(np.abs(dG[amb]), 0) / mc
    return out


# the same-draws cases: tests/asian_reference.py's shapes, seed and evaluation times (t = T: a point with tau <= 0,
# whose G sits exactly at the strike 1: the tie)
MC_SEED = ar.MC_SEED
MC_T_POINTS = ar.MC_T_POINTS
MC_SHAPES = ar.MC_SHAPES
MC_PAYOFFS = ar.MC_PAYOFFS


def mc_points(k):
    """[G_p, S_1..S_k] at MC_T_POINTS: G_p about 1 (the geometric average so far of prices about 1)."""
    S = np.random.RandomState(11).uniform(0.8, 1.3, (5, k))
    return np.concatenate([np.array([[1.0], [0.99], [1.03], [1.0], [1.0]]), S], 1).astype(f32)


_MC = {}


def mc_case(pkg, payoff_, shape, corr=False):
    """The restatement of one same-draws case (with delta), computed once per process."""
    key = (payoff_, shape, corr)
    if key not in _MC:
        k, n_steps, mc = shape
        _MC[key] = mc_value(spec(pkg, payoff_), MC_T_POINTS, mc_points(k), T, n_steps, mc, seed=MC_SEED,
                            L=equicorr_L(k) if corr else None, delta=True)
    return _MC[key]


# ---------------------------------------------------------------- the closed form (fp64)
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def ncdf(x):
    return 0.5 * _erfc(-np.asarray(x, np.float64) / math.sqrt(2.0))


def factor_moments(L, k):
    """(cbar, vbar) = (mean_i (L L^T)_ii, 1^T L L^T 1 / k^2); (1, 1 / k) without a factor."""
    if L is None:
        return 1.0, 1.0 / k
    L = np.tril(np.asarray(L, np.float64))
    C = L @ L.T
    return float(np.trace(C)) / k, float(C.sum()) / (k * k)


def closed_form_terms(X, t, T_, mu, r, sigma, K, cbar, vbar):
    """(M, V, tau) [R] in float64."""
    X = np.asarray(X, np.float64)
    tau = T_ - np.asarray(t, np.float64).reshape(-1)
    ml = np.mean(np.log(X[:, 1:]), 1)
    M = np.log(X[:, 0]) + (tau * ml + (mu - 0.5 * sigma * sigma * cbar) * tau * tau * 0.5) / T_
    V = sigma * sigma * vbar * tau ** 3 / (3.0 * T_ * T_)
    return M, V, tau


def closed_form(X, t, T_, mu, r, sigma, K, cbar, vbar, put=False):
    """(price [R], delta [R, D]) of the call (put) on the geometric average at
    the points X [R, D] = [G, S_1..S_k] and times t [R], in float64; at tau <= 0
    the payoff and its one-sided derivative (1/2 at the tie) in G."""
    X = np.asarray(X, np.float64)
    R, D = X.shape
    k = D - 1
    M, V, tau = closed_form_terms(X, t, T_, mu, r, sigma, K, cbar, vbar)
    live = tau > 0
    price, fwd = np.zeros(R), np.zeros(R)
    with np.errstate(divide="ignore", invalid="ignore"):
        sv = np.sqrt(np.where(live, V, 1.0))
        d2 = (M - np.log(K)) / sv
        d1 = d2 + sv
        df, F = np.exp(-r * tau), np.exp(M + 0.5 * V)
        if put:
            pl, fl = df * (K * ncdf(-d2) - F * ncdf(-d1)), -df * F * ncdf(-d1)
        else:
            pl, fl = df * (F * ncdf(d1) - K * ncdf(d2)), df * F * ncdf(d1)
    s = (K - X[:, 0]) if put else (X[:, 0] - K)
    price = np.where(live, pl, np.maximum(s, 0.0))
    fwd = np.where(live, fl, (-1.0 if put else 1.0) * np.where(s > 0, 1.0, np.where(s == 0, 0.5, 0.0)) * X[:, 0])
    delta = np.zeros((R, D))
    delta[:, 0] = fwd / X[:, 0]
    delta[:, 1:] = np.where(live, fwd * tau / (k * T_), 0.0)[:, None] / X[:, 1:]
    return price, delta


# the arbiter's cases: strike 1, sigma = 0.4, mu = r = 0.05, mc = 2^16, n_steps up to 400
ARBITER = dict(mu_a=0.05, sig_a=0.4, strike=1.0, mc=1 << 16, seed=9, steps=(50, 100, 200, 400),
               points=((1, 0.0, 1.0), (1, 0.5, 0.97), (5, 0.0, 1.0), (5, 0.5, 0.97)))   # (k, t, G)


def arbiter_point(k, G):
    """[G, S_1..S_k]: k = 1: S = 1.05; k = 5: unequal prices."""
    S = [1.05] if k == 1 else np.linspace(0.9, 1.2, k)
    return np.concatenate([[G], S]).astype(f32)


def arbiter_L(k):
    """k = 5: equicorrelated rho = 0.3."""
    return None if k == 1 else equicorr_L(k, 0.3)


def arbiter_exact(k, t, G):
    c = ARBITER
    cbar, vbar = factor_moments(arbiter_L(k), k)
    x = arbiter_point(k, G).astype(np.float64)[None]
    return float(closed_form(x, [t], T, float(f32(c["mu_a"])), float(f32(R_RATE)), float(f32(c["sig_a"])), c["strike"],
                             cbar, vbar)[0][0])
