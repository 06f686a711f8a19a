"""References for the put payoffs (g kinds "put_sum", "put_mean", "smooth_put";
exact kinds "bs_put", "basket_avg_put", "basket_mean_put", "heston_put") -- test
infrastructure only.

  * PutProblem / PutHeston: the put payoffs as duck-typed problems of the
    unchanged oracle (oracle/fbsnn_ref.py loss_function / heston_loss_function),
    written with torch.maximum, whose 1/2 : 1/2 tie gradient the device has;
  * SITES and reference(): one network per place of the engine that evaluates
    the terminal condition, with the oracle's loss and gradients in fp32 and
    fp64 (tests/depth_cases.py's batch recipe and bounds);
  * tie_reference(): three paths with zero Brownian rows, X_N = Xi exactly:
    one in the money, one exactly at the kink, one out of the money;
  * heston2_loss_and_grads: tests/heston2_reference.py's loss on the two-factor
    step, with the payoff object passed in;
  * payoff / mc_value: the put payoff on the terminal states of
    tests/mc_reference.py, tests/heston2_reference.py and
    tests/mc_heston_corr_reference.py (the device's draws);
  * bs_put / exact_put / heston_put: numpy fp64 restatements of the kernels'
    closed forms, computed directly, never as the call minus parity (bs_put
    with logsf: the independent log-survival-function arithmetic).
"""
from __future__ import annotations

import copy
import dataclasses

import numpy as np
import torch

import depth_cases as dc
import heston2_reference as h2
import mc_heston_corr_reference as mhc
import mc_reference as mr
from oracle import fbsnn_ref as fr
from oracle import philox as ph

f32 = np.float32
PAYOFFS = ("put_sum", "put_mean", "smooth_put")
CALL_OF = {"put_sum": "call_sum", "put_mean": "call_mean", "smooth_put": "smooth_call"}
ALPHA = 10.0
T = 1.0


# ---------------------------------------------------------------- oracle problems
class PutProblem:
    """The dynamics and phi of oracle problem `base` ("call", "basket", "call1d",
    "bsb") with a put terminal condition over all D columns."""

    def __init__(self, base, D, payoff, strike, alpha=ALPHA):
        assert payoff in PAYOFFS
        self.base = fr.make_problem(base, D)
        self.kind, self.D, self.payoff, self.strike, self.alpha = base, D, payoff, float(strike), float(alpha)
        self.q3_compat = self.base.q3_compat

    def mu(self, t, X, Y, Z):
        return self.base.mu(t, X, Y, Z)

    def sigma(self, t, X, Y):
        return self.base.sigma(t, X, Y)

    def phi(self, t, X, Y, Z):
        return self.base.phi(t, X, Y, Z)

    def g(self, X):
        if self.payoff == "put_sum":
            return torch.maximum(self.strike - torch.sum(X, dim=1, keepdim=True), torch.tensor(0.0, dtype=X.dtype))
        a = self.strike - torch.mean(X, dim=1, keepdim=True)
        if self.payoff == "put_mean":
            return torch.maximum(a, torch.tensor(0.0, dtype=X.dtype))
        return a / (1 + torch.exp(-self.alpha * a))


@dataclasses.dataclass
class PutHeston(fr.Heston):
    """oracle.fbsnn_ref.Heston with the put on mean S: payoff "discontinuous"
    max(K - mean S, 0), "continuous" its sigmoid-smoothed form (alpha = 10)."""

    def g(self, S):
        a = self.strike - torch.mean(S, dim=1, keepdim=True) if self.k > 1 else self.strike - S
        if self.payoff == "discontinuous":
            return torch.maximum(a, torch.tensor(0.0, dtype=S.dtype))
        return a / (1 + torch.exp(-10.0 * a))


# the oracle problem each payoff rides on at D > 1, and its coefficients as a spec
BASE_OF = {"put_sum": "call", "put_mean": "basket", "smooth_put": "basket"}
COEF = {"call": dict(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=1.0),
        "basket": dict(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=0.0),
        "call1d": dict(mu_a=0.01, sig_a=0.25, phi_r=0.01, phi_c=0.0, q3=True),
        "bsb": dict(sig_a=0.4, phi_r=0.05, phi_c=1.0)}


def strike_of(payoff, D, level=1.0625):
    """K = level for the means, level * D for the sum.  From Xi = ones the mean
    of X_T drifts to about e^{0.05} = 1.051 with a spread of 0.2 / sqrt(D): at
    K = 1 every path of a D = 100 batch ends out of the money; 1.0625 (exact in
    fp32, as is 1.0625 D) puts rows on both sides of the kink at every D used
    (asserted in tests/test_put_cpu.py).  level = 1: the tie case."""
    return level * D if payoff == "put_sum" else level


def spec_for(pkg, base, payoff, D, level=1.0625):
    return pkg.ProblemSpec(g=payoff, strike=strike_of(payoff, D, level), g_alpha=ALPHA, **COEF[base])


# ---------------------------------------------------------------- cotangent sites
# One network per place that evaluates terminal_g / builds gA, gB.  env holds
# while the context is created (every other path switch unset).  M = 20, N = 3:
# 80 rows, ragged against the 16-, 32- and 64-row tiles; at M <= 128 the
# width-110 split-bf16 layout selects the column-split phase kernels by default.
_N110 = dict(mode="NAIS-Net", act="Sine", layers=[101] + 4 * [110] + [1])
_X3OFF = {"DBSDE_X3": "0", "DBSDE_TNW_X3": "0"}
SITES = {
    "fused110": dict(_N110, env={"DBSDE_CS": "0"}, fused=True),                 # phase.hpp row_cotan, split-bf16
    "fused110_fp32": dict(_N110, env=dict(_X3OFF, DBSDE_CS="0"), fused=True),   # the fp32-input form
    "colsplit110": dict(_N110, env={}, fused=True),                             # phasecs.hip
    "chain110": dict(_N110, env={"DBSDE_FUSED": "0"}, fused=False),             # EPI_COTAN epilogue
    "fused16": dict(mode="NAIS-Net", act="Sine", layers=[15] + 4 * [16] + [1], env={}, fused=True),   # phase2.hip
    "fc256_q3": dict(mode="FC", act="Sine", layers=[2] + 4 * [256] + [1], env={}, fused=True, base="call1d"),
    # (the fused width-256 kernels have the split-bf16 form only: without it, the fp32 chain's epilogue with q3)
    "fc256_q3_fp32": dict(mode="FC", act="Sine", layers=[2] + 4 * [256] + [1], env=_X3OFF, fused=False, base="call1d"),
    "wide130": dict(mode="FC", act="Tanh", layers=[131, 64, 32, 16, 1], env={}, fused=False),   # zrow_cotan_kernel
}
M, N = dc.M, dc.N
RUNS = [(s, p) for s in SITES for p in PAYOFFS]


def site_dim(site):
    return SITES[site]["layers"][0] - 1


def site_base(site, payoff):
    return SITES[site].get("base", BASE_OF[payoff])


def site_model(site):
    c = SITES[site]
    torch.manual_seed(site_dim(site) + len(c["layers"]))
    return fr.build_model(c["mode"], c["layers"], c["act"])


def _bundle(model, problem, t, W, Xi, M_):
    D = Xi.shape[1]
    ref32 = fr.loss_and_grads(model, problem, t, W, Xi, M_, D)
    ref64 = fr.loss_and_grads(copy.deepcopy(model).double(), problem, t.double(), W.double(), Xi.double(), M_, D)
    return dict(model=model, params=fr.flat_params(model), tensors=dc.tensors(model), M=M_, N=t.shape[1] - 1,
                t=t.squeeze(-1).numpy(), W=W.numpy(), Xi=Xi.numpy(), ref32=ref32, ref64=ref64)


_REFS = {}


def reference(site, payoff):
    """tests/depth_cases.py's bundle (model, params, tensors, t, W, Xi, ref32,
    ref64) of a site's network with the payoff; the sites that share a network
    share the bundle.  Computed once per process; treat it as read-only."""
    c = SITES[site]
    key = (c["mode"], tuple(c["layers"]), c["act"], site_base(site, payoff), payoff)
    if key not in _REFS:
        D = site_dim(site)
        t, W = fr.fetch_minibatch(M, N, D, T, rng=np.random.RandomState(7))
        prob = PutProblem(site_base(site, payoff), D, payoff, strike_of(payoff, D))
        _REFS[key] = _bundle(site_model(site), prob, t, W, torch.ones((1, D), dtype=torch.float32), M)
    return _REFS[key]


def moneyness(b, payoff, level=1.0625):
    """K - sum X_N (put_sum) or K - mean X_N of the bundle's terminal rows, fp64."""
    XN = b["ref64"]["X"][:, -1, :]
    D = XN.shape[1]
    return strike_of(payoff, D, level) - (XN.sum(1) if payoff == "put_sum" else XN.mean(1))


# ---------------------------------------------------------------- the tie case
TIE_SITES = ("fused110", "colsplit110", "chain110", "fused16", "wide130")
TIE_PAYOFFS = ("put_sum", "put_mean")
TIE_LEVELS = (1.0, 1.25, 0.75)      # at the kink, out of the money, in the money
# the terminal Z-term the device added, deduced as its loss minus every other
# term (from its own Y and Z, in fp64), against sum |Z_N - dg|^2 with the
# oracle's dg: within 1e-5 of the loss.  The loss is an fp32 sum of some ten
# fp32 terms per path, each rounded to 2^-24 relative: below 1e-6 of the loss.
TIE_ZTERM_RTOL = 1e-5


def tie_reference(site, payoff):
    """mu = 0 ("bsb" dynamics), per-path Xi = level * ones, W = 0: X_N = Xi
    exactly, and sum / mean of it are exact in fp32 and fp64 alike."""
    key = ("tie", site, payoff)
    if key not in _REFS:
        D = site_dim(site)
        Mt = len(TIE_LEVELS)
        t, W = fr.fetch_minibatch(Mt, N, D, T, rng=np.random.RandomState(7))
        W = torch.zeros_like(W)
        Xi = torch.tensor(TIE_LEVELS, dtype=torch.float32).reshape(Mt, 1).repeat(1, D)
        prob = PutProblem("bsb", D, payoff, strike_of(payoff, D, 1.0))
        _REFS[key] = _bundle(site_model(site), prob, t, W, Xi, Mt)
        _REFS[key]["problem"] = prob
    return _REFS[key]


# ---------------------------------------------------------------- Heston losses
def heston2_loss_and_grads(model, h, tgrid, dw, Xi):
    """tests/heston2_reference.py's loss_and_grads (the FBSNN loss of
    oracle.fbsnn_ref.heston_loss_function on the two-factor step, float64, on
    increments dw [M, N, 2k] and the grid tgrid) with the payoff object h."""
    k = h.k
    model = copy.deepcopy(model).double()
    model.zero_grad(set_to_none=True)
    dw = torch.as_tensor(np.asarray(dw, np.float64))
    tg = torch.as_tensor(np.asarray(tgrid, np.float64))
    M_, Nn, _ = dw.shape
    X0 = torch.as_tensor(np.broadcast_to(np.asarray(Xi, np.float64).reshape(-1, 2 * k), (M_, 2 * k)).copy())
    X0.requires_grad_(True)
    rb = float(np.sqrt(1.0 - h.rho * h.rho))
    tcol = lambda n: tg[n].expand(M_, 1)
    Y0, Z0 = fr.heston_net_u(model, tcol(0), X0)
    Xs, Ys, Zs = [X0], [Y0], [Z0]
    loss = 0
    for n in range(Nn):
        dt = tg[n + 1] - tg[n]
        S, v = X0[:, :k], X0[:, k:]
        mu = torch.cat([h2.R_RATE * S, h.kappa * (h.theta - v)], dim=1).clamp(-100, 100)
        sv = torch.sqrt(torch.clamp(v, min=1e-8))
        sigV = h.sigma * sv
        d00, d10, d11 = (sv * S).clamp(-100, 100), (h.rho * sigV).clamp(-100, 100), (rb * sigV).clamp(-100, 100)
        w1, w2 = dw[:, n, :k], dw[:, n, k:]
        a, b = d00 * w1, d10 * w1 + d11 * w2
        X1 = X0 + mu * dt + torch.cat([a, b], dim=1)
        Y1t = Y0 + h2.R_RATE * Y0 * dt + torch.sum(Z0[:, :k] * a + Z0[:, k:] * b, dim=1, keepdim=True)
        Y1, Z1 = fr.heston_net_u(model, tcol(n + 1), X1)
        loss = loss + torch.sum(torch.pow(Y1 - Y1t, 2))
        X0, Y0, Z0 = X1, Y1, Z1
        Xs.append(X0)
        Ys.append(Y0)
        Zs.append(Z0)
    S1 = X1[:, :k]
    g = h.g(S1)
    loss = loss + torch.sum(torch.pow(Y1 - g, 2))
    dg = torch.autograd.grad(outputs=[g], inputs=[S1], grad_outputs=torch.ones_like(g), allow_unused=True,
                             retain_graph=True, create_graph=True)[0]
    loss = loss + torch.sum(torch.pow(Z1[:, :k] - dg, 2))
    loss.backward()
    grad, mask = fr.flat_grads(model)
    return dict(loss=float(loss.detach()), X=torch.stack(Xs, 1).detach().numpy(), Y=torch.stack(Ys, 1).detach().numpy(),
                Z=torch.stack(Zs, 1).detach().numpy(), grad=np.asarray(grad, np.float64), used=mask)


HESTON_K, HESTON_M, HESTON_SEED = 3, 7, 4        # tests/heston2_reference.py's k3_m7 case


def heston_spec(pkg, kind, payoff_type, k=HESTON_K):
    return h2.spec(pkg, k, "put_mean" if payoff_type == "discontinuous" else "smooth_put", kind=kind)


# ---------------------------------------------------------------- Monte-Carlo
def payoff(spec, X):
    """tests/mc_reference.py's payoff for the put kinds: g [M], dg/dX [M, D]
    and the kink variable a [M] (None for the smooth put) in float64; -1/2 of
    the in-the-money gradient at a == 0."""
    X = np.asarray(X, np.float64)
    c = mr.g_cols(spec, X.shape[1])
    Xc = X[:, :c]
    K, al = float(f32(spec.strike)), float(f32(spec.g_alpha))
    dg = np.zeros_like(X)
    if spec.g == "smooth_put":
        a_ = K - np.mean(Xc, 1)
        s = 1.0 / (1.0 + np.exp(-al * a_))
        dg[:, :c] = (-(s + a_ * al * s * (1.0 - s)) / c)[:, None]
        return a_ * s, dg, None
    assert spec.g in ("put_sum", "put_mean"), spec.g
    n = c if spec.g == "put_mean" else 1
    a = K - np.sum(Xc, 1) / n
    dg[:, :c] = (-np.where(a > 0, 1.0, np.where(a == 0, 0.5, 0.0)) / n)[:, None]
    return np.maximum(a, 0.0), dg, a


def terminal(spec, tau, x, n_steps, mc, seed, offset=0, L=None, want_J=False):
    """(X_T [mc, D] float32, J_T or None) of one point on the device's draws,
    by the restatement of the spec's kind."""
    if spec.kind == "heston2":
        return h2.mc_terminal(spec, tau, x, n_steps, mc, seed, offset), None
    if spec.kind == "heston" and L is not None:
        return mhc.terminal(spec, tau, x, n_steps, mc, seed, offset, L), None
    return mr.terminal(spec, tau, x, n_steps, mc, seed, offset, L, want_J=want_J)


def mc_value(spec, t, X, T_, n_steps, mc, seed=0, offset=0, L=None, delta=False):
    """tests/mc_reference.py's mc_value with the put payoff, plus mean_XT [P]:
    mean over samples of the payoff columns' sum (put_sum) or mean."""
    t = np.asarray(t, f32).reshape(-1)
    X = np.asarray(X, f32).reshape(t.size, -1)
    P, D = X.shape
    out = dict(value=np.zeros(P), stderr=np.zeros(P), ambiguous=np.zeros(P, int), mean_XT=np.zeros(P),
               delta=np.zeros((P, D)) if delta else None, delta_slack=np.zeros((P, D)) if delta else None)
    c = mr.g_cols(spec, D)
    n = 1 if spec.g == "put_sum" else c
    for p in range(P):
        tau = float(f32(T_) - t[p])
        if tau <= 0:
            g, dg, _ = payoff(spec, X[p:p + 1])
            out["value"][p] = g[0]
            out["mean_XT"][p] = np.sum(X[p, :c].astype(np.float64)) / n
            if delta:
                out["delta"][p] = dg[0]
            continue
        XT, J = terminal(spec, tau, X[p], n_steps, mc, seed, offset, L, want_J=delta)
        g, dg, a = payoff(spec, XT)
        disc = np.exp(-float(f32(spec.phi_r)) * tau)
        out["value"][p] = disc * np.mean(g)
        out["stderr"][p] = disc * np.std(g, ddof=1) / np.sqrt(mc) if mc > 1 else 0.0
        out["mean_XT"][p] = np.mean(np.sum(XT[:, :c].astype(np.float64), 1) / n)
        amb = np.abs(a) < mr.AMBIGUOUS if a is not None else np.zeros(mc, bool)
        out["ambiguous"][p] = int(amb.sum())
        if delta:
            out["delta"][p] = disc * np.mean(dg * J.astype(np.float64), 0)
            if a is not None:
                kink = np.zeros((mc, D))
                kink[:, :c] = np.abs(J[:, :c].astype(np.float64)) / n
                out["delta_slack"][p] = np.sum(kink[amb], 0) / mc
    return out


# tests/test_gpu_mc.py's shapes, points, seed and evaluation times
MC_SHAPES = ((8, 6, 4096), (3, 1, 1000))
MC_SEED = 2
MC_T_POINTS = np.array([0.0, 0.25, 0.5, 1.0, 0.0], f32)       # t = T: a point with tau <= 0
MC_DIAG = ("put_mean", "put_mean_corr", "put_sum", "smooth_put")
MC_HESTON_K = 3
MC_HESTON = [(kind, g) for kind in ("heston", "heston2", "heston_corr") for g in ("put_mean", "smooth_put")]


def equicorr_L(D, rho=0.3):
    return np.linalg.cholesky((1 - rho) * np.eye(D) + rho * np.ones((D, D))).astype(f32)


def mc_diag_spec(pkg, name, D, call=False):
    """(spec, L) of a DIAG comparator case; call: its call twin."""
    g = name.replace("_corr", "")
    g = CALL_OF[g] if call else g
    coef = COEF["call"] if name == "put_sum" else dict(COEF["basket"])
    K = 1.0 * D if name == "put_sum" else 1.0
    return pkg.ProblemSpec(g=g, strike=K, g_alpha=ALPHA, **coef), (equicorr_L(D) if name.endswith("_corr") else None)


def mc_points(D):
    return np.random.RandomState(11).uniform(0.8, 1.3, (5, D)).astype(f32)


def mc_heston_spec(pkg, kind, g, k=MC_HESTON_K):
    """(spec, L): "heston_corr" is kind "heston" with an equicorrelated factor."""
    if kind == "heston2":
        return h2.spec(pkg, k, g), None
    return mhc.spec_for(pkg, k, g), (mhc.equicorr_factor(k, 0.5).astype(f32) if kind == "heston_corr" else None)


_MC = {}


def mc_diag_case(pkg, name, shape):
    if (name, shape) not in _MC:
        D, n_steps, mc = shape
        spec, L = mc_diag_spec(pkg, name, D)
        _MC[(name, shape)] = mc_value(spec, MC_T_POINTS, mc_points(D), T, n_steps, mc, seed=MC_SEED, L=L, delta=True)
    return _MC[(name, shape)]


def mc_heston_case(pkg, kind, g):
    if (kind, g) not in _MC:
        spec, L = mc_heston_spec(pkg, kind, g)
        _MC[(kind, g)] = mc_value(spec, MC_T_POINTS, h2.mc_points(MC_HESTON_K), T, h2.MC_STEPS, h2.MC_SAMPLES,
                                  seed=MC_SEED, L=L)
    return _MC[(kind, g)]


# ---------------------------------------------------------------- closed forms
def bs_put(S, K, tau, r, sig, logsf=False):
    """(price, delta) float64 of the Black-Scholes put, K e^{-r tau} N(-d2) -
    S N(-d1) and -N(-d1); the payoff and -1 / -1/2 / 0 at tau <= 0.  N(-d) is
    the kernel's 0.5 erfc(d / sqrt(2)) (csrc/evals.hip ncdf), or with logsf the
    independent exp(scipy.stats.norm.logsf(d)) in log arithmetic."""
    from scipy.special import erfc
    from scipy.stats import norm
    S, tau = np.broadcast_arrays(np.asarray(S, np.float64), np.asarray(tau, np.float64))
    run = tau > 0
    tt = np.where(run, tau, 1.0)
    st = sig * np.sqrt(tt)
    d1 = (np.log(S / K) + (r + 0.5 * sig * sig) * tt) / st
    d2 = d1 - st
    if logsf:
        price = np.exp(np.log(K) - r * tt + norm.logsf(d2)) - np.exp(np.log(S) + norm.logsf(d1))
        delta = -np.exp(norm.logsf(d1))
    else:
        ncdf = lambda x: 0.5 * erfc(-x * 0.70710678118654752440)
        price = K * np.exp(-r * tt) * ncdf(-d2) - S * ncdf(-d1)
        delta = -ncdf(-d1)
    return (np.where(run, price, np.maximum(K - S, 0.0)),
            np.where(run, delta, np.where(S < K, -1.0, np.where(S == K, -0.5, 0.0))))


def bs_call(S, K, tau, r, sig):
    """(price, delta) of the call by the same arithmetic (N(d) = sf(-d)), tau > 0."""
    from scipy.stats import norm
    S, tau = np.asarray(S, np.float64), np.asarray(tau, np.float64)
    st = sig * np.sqrt(tau)
    d1 = (np.log(S / K) + (r + 0.5 * sig * sig) * tau) / st
    return S * norm.sf(-d1) - K * np.exp(-r * tau) * norm.sf(-(d1 - st)), norm.sf(-d1)


def exact_put(kind, X, tau, r, sig, K):
    """(price, delta) [R, ncol] of "bs_put" (per coordinate), "basket_avg_put"
    (put on mean(x), sigma / sqrt(D)) and "basket_mean_put" (mean of the
    per-asset puts) at X [R, D], tau [R]."""
    X = np.asarray(X, np.float64)
    tau = np.asarray(tau, np.float64)
    D = X.shape[1]
    if kind == "bs_put":
        return bs_put(X, K, tau[:, None], r, sig)
    if kind == "basket_avg_put":
        p, d = bs_put(X.sum(1) / D, K, tau, r, sig / np.sqrt(D))
        return p[:, None], d[:, None]
    assert kind == "basket_mean_put"
    p, d = bs_put(X, K, tau[:, None], r, sig)
    return (p.sum(1) / D)[:, None], (d.sum(1) / D)[:, None]


def _heston_one(S, v, tau, r, K, kappa, theta, sigma, rho):
    """((call, P1), (put, -Q1)) of one point on the kernel's quadrature nodes
    (tests/heston2_reference.py _call_one), Q_j = 1/2 - I_j / pi."""
    if tau <= 0:
        return ((max(S - K, 0.0), 1.0 if S > K else (0.5 if S == K else 0.0)),
                (max(K - S, 0.0), -1.0 if S < K else (-0.5 if S == K else 0.0)))
    x = np.log(S / K)
    U = h2.upper_limit(tau, v, x, r, kappa, theta, sigma, rho)
    hw = U / h2.PANELS
    phi = ((np.arange(h2.PANELS) + 0.5) * hw)[:, None] + 0.5 * hw * h2.GL_X[None, :]
    I = []
    for j in (1, 2):
        E = h2.exponent(j, phi, tau, v, x, r, kappa, theta, sigma, rho)
        I.append(0.5 * hw * np.sum(h2.GL_W[None, :] * (np.exp(E.real) * np.sin(E.imag) / phi)) / np.pi)
    dK = K * np.exp(-r * tau)
    return ((S * (0.5 + I[0]) - dK * (0.5 + I[1]), 0.5 + I[0]), (dK * (0.5 - I[1]) - S * (0.5 - I[0]), -(0.5 - I[0])))


def heston_both(S, v, tau, r=h2.R_RATE, K=1.0, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8):
    """(call, call delta, put, put delta) float64 arrays at the points."""
    S, v, tau = np.broadcast_arrays(np.asarray(S, np.float64), np.asarray(v, np.float64), np.asarray(tau, np.float64))
    out = np.array([np.ravel(_heston_one(float(a), float(b), float(c), r, K, kappa, theta, sigma, rho))
                    for a, b, c in zip(S.ravel(), v.ravel(), tau.ravel())]).reshape(S.shape + (4,))
    return out[..., 0], out[..., 1], out[..., 2], out[..., 3]


def heston_put(S, v, tau, **kw):
    c, cd, p, pd = heston_both(S, v, tau, **kw)
    return p, pd


def closed_form_points():
    """tests/test_gpu_heston2.py's 64 points (S, v, tau): tau = 0 on both sides
    of and at the kink, the corners of the stated domain, random points of it."""
    rs = np.random.RandomState(21)
    S = np.concatenate([[1.5, 1.0, 0.5, 2.0, 0.5, 2.0, 0.5, 2.0, 0.5], rs.uniform(0.5, 2.0, 55)])
    v = np.concatenate([[0.2, 0.2, 0.2, 0.01, 0.01, 1.0, 1.0, 0.01, 1.0], rs.uniform(0.01, 1.0, 55)])
    tau = np.concatenate([[0.0, 0.0, 0.0, 0.05, 0.05, 2.0, 2.0, 2.0, 0.05], rs.uniform(0.05, 2.0, 55)])
    return S.astype(f32), v.astype(f32), tau.astype(f32)


# Black-Scholes parameters of the closed-form tests.  sigma = 0.4: at S / K = 2,
# tau = 0.05 the put is about 1e-15, a normal fp32 number (at sigma = 0.2 it is
# 1e-56 and fp32 cannot hold it), 15 orders of magnitude below the call.
BS = dict(r=0.05, sig=0.4, K=1.0)
DEEP_OTM = dict(S=2.0, tau=0.05)
