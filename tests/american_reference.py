"""References for the penalised American put (dbsde_problem.pen, ProblemSpec
penalty; exact kind "american_put") -- test infrastructure only.

  * AmericanProblem: tests/put_reference.py's PutProblem (dynamics, phi and put
    payoff of an oracle problem) with the driver phi - pen relu(g(X) - Y), as a
    duck-typed problem of the unchanged oracle (oracle/fbsnn_ref.py);
  * reference(): per cotangent site of tests/put_reference.py's SITES and
    payoff, the oracle's loss and gradients in fp32 and fp64 on
    tests/depth_cases.py's batch recipe (M = 20, N = 3, RandomState(7), Xi = ones);
  * margins(): per interior row (n < N) of the fp64 reference, the distance
    |g(X) - Y| / (1 + |Y|) from the exercise boundary and the indicator g > Y;
  * crr(): the Cox-Ross-Rubinstein recursion of include/dbsde.h
    (DBSDE_EXACT_AMERICAN_PUT) in numpy fp64;
  * hand_gradient(): the loss gradient from the cotangent formulas the kernels
    implement, written out (tests/test_american_cpu.py holds it to autograd).

Strikes and networks.  The indicator 1[g(X) > Y] must be decided the same way
in fp32 on the device and in fp64 in the oracle, and both branches must be
exercised, so every case needs rows well away from g = Y on both sides
(tests/test_american_cpu.py asserts: every interior row's margin >= 1e-3, each
branch >= 20 % of the interior rows).  Y is the untrained network's output,
which has no reason to sit near the payoff, so each network's output bias is
replaced by the case's bias, which moves every Y by the same amount and so
places the interior rows' Y among their payoffs.  The n = 0 rows (one third of
the interior rows) share X = Xi and t = 0, hence one branch; the rows of n = 1,
2 spread with the paths.  The values of NET_CASES below were chosen on the fp64
oracle alone: over the strike levels 1.0625, 1.125, 1.03125 and biases on a grid
of 1e-3, the pair with the largest smallest margin among those with 25 % to
75 % of the interior rows in exercise (smallest margins 6e-3 to 6e-2).
"""
from __future__ import annotations

import copy

import numpy as np
import torch

import depth_cases as dc
import put_reference as pr
from oracle import fbsnn_ref as fr

PEN = 100.0
PAYOFFS = ("put_sum", "put_mean")
SITES = tuple(pr.SITES)
RUNS = [(s, p) for s in SITES for p in PAYOFFS]
M, N, T = dc.M, dc.N, pr.T
MARGIN_MIN, BRANCH_MIN = 1e-3, 0.20


class AmericanProblem(pr.PutProblem):
    """PutProblem with the penalised driver: phi - pen relu(g(X) - Y)."""

    def __init__(self, base, D, payoff, strike, pen=PEN):
        super().__init__(base, D, payoff, strike)
        self.pen = float(pen)

    def phi(self, t, X, Y, Z):
        return self.base.phi(t, X, Y, Z) - self.pen * torch.relu(self.g(X) - Y)


# (site network, payoff) -> (strike level, output bias): K = level (x D for the
# sum); the network is tests/put_reference.py's site_model with its output bias
# replaced.  Sites that share a network (the four width-110 sites; the two
# width-256 ones) share the entry.
def _net_key(site):
    c = pr.SITES[site]
    return (c["mode"], tuple(c["layers"]), c["act"])


NET_CASES = {}


def _set(site, payoff, level, bias):
    NET_CASES[(_net_key(site), payoff)] = (float(level), float(bias))


# the values (see the module docstring); asserted by tests/test_american_cpu.py
_set("fused110", "put_sum", 1.03125, 3.324)
_set("fused110", "put_mean", 1.03125, 0.679)
_set("fused16", "put_sum", 1.03125, 1.385)
_set("fused16", "put_mean", 1.03125, 1.168)
_set("fc256_q3", "put_sum", 1.0625, -0.194)
_set("fc256_q3", "put_mean", 1.0625, -0.194)
_set("wide130", "put_sum", 1.03125, 0.802)
_set("wide130", "put_mean", 1.0625, -0.412)


def case_of(site, payoff):
    return NET_CASES[(_net_key(site), payoff)]


def strike_of(site, payoff):
    return pr.strike_of(payoff, pr.site_dim(site), case_of(site, payoff)[0])


def output_bias(model):
    """The bias of the network's output layer (the only one-element bias)."""
    found = [p for n, p in model.named_parameters() if n.endswith("bias") and p.numel() == 1]
    assert len(found) == 1, [n for n, _ in model.named_parameters()]
    return found[0]


def site_model(site, payoff):
    """tests/put_reference.py's network of the site with the output bias of the case."""
    model = pr.site_model(site)
    with torch.no_grad():
        output_bias(model).fill_(case_of(site, payoff)[1])
    return model


def spec_for(pkg, site, payoff, pen=PEN):
    base = pr.site_base(site, payoff)
    return pkg.ProblemSpec(g=payoff, strike=strike_of(site, payoff), g_alpha=pr.ALPHA, penalty=pen, **pr.COEF[base])


_REFS = {}


def bundle(model, problem, t, W, Xi, M_):
    D = Xi.shape[1]
    ref32 = fr.loss_and_grads(model, problem, t, W, Xi, M_, D)
    ref64 = fr.loss_and_grads(copy.deepcopy(model).double(), problem, t.double(), W.double(), Xi.double(), M_, D)
    return dict(model=model, params=fr.flat_params(model), tensors=dc.tensors(model), M=M_, N=t.shape[1] - 1,
                t=t.squeeze(-1).numpy(), W=W.numpy(), Xi=Xi.numpy(), ref32=ref32, ref64=ref64, problem=problem)


def reference(site, payoff, pen=PEN):
    """tests/depth_cases.py's bundle of the site's network with the penalised
    put; the sites that share a network share the bundle.  Computed once per
    process; treat it as read-only."""
    key = (_net_key(site), pr.site_base(site, payoff), payoff, float(pen))
    if key not in _REFS:
        D = pr.site_dim(site)
        t, W = fr.fetch_minibatch(M, N, D, T, rng=np.random.RandomState(7))
        prob = AmericanProblem(pr.site_base(site, payoff), D, payoff, strike_of(site, payoff), pen)
        _REFS[key] = bundle(site_model(site, payoff), prob, t, W, torch.ones((1, D), dtype=torch.float32), M)
    return _REFS[key]


def payoff_np(payoff, strike, X):
    """g over the last axis of X, fp64."""
    X = np.asarray(X, np.float64)
    a = strike - (X.sum(-1) if payoff == "put_sum" else X.mean(-1))
    return np.maximum(a, 0.0)


def margins(b):
    """(margin [M, N], indicator [M, N]) of the interior rows n < N of the
    bundle's fp64 reference: |g(X) - Y| / (1 + |Y|) and g(X) > Y."""
    prob = b["problem"]
    X, Y = b["ref64"]["X"][:, :-1, :], b["ref64"]["Y"][:, :-1, 0]
    g = payoff_np(prob.payoff, prob.strike, X)
    return np.abs(g - Y) / (1.0 + np.abs(Y)), g > Y


# ---------------------------------------------------------------- the tree
def crr(S, K, r, sigma, b, tau, n, pen):
    """(price, delta) of the put on the Cox-Ross-Rubinstein tree of n steps,
    fp64: u = e^{sigma sqrt(dt)}, d = 1 / u, p = (e^{b dt} - d) / (u - d),
    c = e^{-r dt} (p v_up + (1 - p) v_dn), g = max(K - s, 0); pen = inf: v =
    max(c, g); finite pen >= 0: v = g > c ? (c + pen dt g) / (1 + pen dt) : c.
    delta is the level-1 difference quotient; tau <= 0: the payoff and its
    0 / -1/2 / -1 delta; p outside [0, 1]: (nan, nan)."""
    S, K = float(S), float(K)
    if tau <= 0:
        return max(K - S, 0.0), (-1.0 if S < K else (-0.5 if S == K else 0.0))
    n = int(n)
    dt = tau / n
    u = np.exp(sigma * np.sqrt(dt))
    d = 1.0 / u
    p = (np.exp(b * dt) - d) / (u - d)
    disc = np.exp(-r * dt)
    if not 0.0 <= p <= 1.0:          # no risk-neutral probability: no tree value
        return float("nan"), float("nan")
    j = np.arange(n + 1, dtype=np.float64)
    v = np.maximum(K - S * u ** (2.0 * j - n), 0.0)         # node j: j up moves
    v1 = None
    for m in range(n - 1, -1, -1):
        s = S * u ** (2.0 * np.arange(m + 1, dtype=np.float64) - m)
        g = np.maximum(K - s, 0.0)
        c = disc * (p * v[1:m + 2] + (1.0 - p) * v[:m + 1])
        if np.isinf(pen):
            v = np.maximum(c, g)
        else:
            v = np.where(g > c, (c + pen * dt * g) / (1.0 + pen * dt), c)
        if m == 1:
            v1 = v.copy()
    return float(v[0]), float((v1[1] - v1[0]) / (S * u - S * d))


def bs_put_carry(S, K, r, sigma, b, tau):
    """The European put with cost of carry b, fp64 (b = r: Black-Scholes)."""
    from scipy.stats import norm
    st = sigma * np.sqrt(tau)
    d1 = (np.log(S / K) + (b + 0.5 * sigma * sigma) * tau) / st
    return K * np.exp(-r * tau) * norm.cdf(-(d1 - st)) - S * np.exp((b - r) * tau) * norm.cdf(-d1)


# ---------------------------------------------------------------- the cotangent formulas, written out
def hand_gradient(model, prob, coef, t, W, Xi, M_):
    """The gradient of the FBSNN loss of the penalised problem from the
    formulas the kernels implement, in the model's dtype:

      res_n  = Y_{n+1} - (Y_n + phi_n dt_n + Z_n . sdw_n),        n < N
      phi_n  = phi_r (Y_n - phi_c X_n . Z_n) - pen max(g(X_n) - Y_n, 0)
      ubar_n = -2 res_n (1 + (phi_r + pen 1[g(X_n) > Y_n]) dt_n) + [n >= 1] 2 res_{n-1}
      ubar_N = 2 (Y_N - g(X_N)) + 2 res_{N-1}
      zbar_n = -2 res_n (-phi_r phi_c X_n dt_n + sdw_n),          zbar_N = 2 (Z_N - Dg(X_N))

    contracted with d(Y, Z) / d(parameters) by one autograd call (X does not
    depend on the parameters).  coef: dict(mu_a, sig_a, phi_r, phi_c) of the
    base problem.  Returns (loss, flat gradient)."""
    Nn = t.shape[1] - 1
    D = Xi.shape[1]
    X0 = Xi.view(1, D).repeat(M_, 1).clone().requires_grad_(True)
    Xs, Ys, Zs, sdws = [], [], [], []
    for n in range(Nn + 1):
        Y, Z = fr.net_u(model, t[:, n, :], X0)
        Xs.append(X0), Ys.append(Y), Zs.append(Z)
        if n < Nn:
            dt = t[:, n + 1, :] - t[:, n, :]
            sdw = coef["sig_a"] * X0.detach() * (W[:, n + 1, :] - W[:, n, :])
            sdws.append(sdw)
            X0 = (X0.detach() + coef["mu_a"] * X0.detach() * dt + sdw).requires_grad_(True)
    pen, pr_, pc = prob.pen, coef["phi_r"], coef["phi_c"]
    res = []
    with torch.no_grad():
        ub = [None] * (Nn + 1)
        zb = [None] * (Nn + 1)
        for n in range(Nn):
            dt = t[:, n + 1, :] - t[:, n, :]
            X, Y, Z = Xs[n].detach(), Ys[n].detach(), Zs[n].detach()
            g = prob.g(X)
            ind = (g > Y).to(Y.dtype)
            phi = pr_ * (Y - pc * torch.sum(X * Z, 1, keepdim=True)) - pen * ind * (g - Y)
            r_n = Ys[n + 1].detach() - (Y + phi * dt + torch.sum(Z * sdws[n], 1, keepdim=True))
            res.append(r_n)
            ub[n] = -2.0 * r_n * (1.0 + (pr_ + pen * ind) * dt) + (2.0 * res[n - 1] if n >= 1 else 0.0)
            zb[n] = -2.0 * r_n * (-pr_ * pc * X * dt + sdws[n])
        XN, YN, ZN = Xs[Nn].detach(), Ys[Nn].detach(), Zs[Nn].detach()
    with torch.enable_grad():
        XNg = XN.clone().requires_grad_(True)
        gN = prob.g(XNg)
        dgN = torch.autograd.grad(gN, XNg, torch.ones_like(gN))[0]
    gN = gN.detach()
    ub[Nn] = 2.0 * (YN - gN) + 2.0 * res[Nn - 1]
    zb[Nn] = 2.0 * (ZN - dgN)
    loss = sum(float(torch.sum(r * r)) for r in res) + float(torch.sum((YN - gN) ** 2)) + float(torch.sum((ZN - dgN) ** 2))
    params = [p for p in model.parameters()]
    grads = torch.autograd.grad(Ys + Zs, params, ub + zb, allow_unused=True)
    flat = torch.cat([(g if g is not None else torch.zeros_like(p)).reshape(-1) for g, p in zip(grads, params)])
    return loss, flat.detach().numpy()


# ---------------------------------------------------------------- plugin against native
PLUGIN = dict(D=4, mode="Naisnet", act="Tanh", layers=[5, 16, 16, 16, 16, 1], strike=4.25, seed=11)


def plugin_reference():
    """The bundle of tests/test_gpu_american.py's plugin-against-native case:
    D = 4, put_sum at K = 4.25 on CallOption's coefficients, penalty 100, M = 20,
    N = 3; a seeded Naisnet whose output bias is the median gap g(X) - Y of the
    interior rows at bias 0, rounded to 1e-2 (rows on both sides of g = Y)."""
    if "plugin" not in _REFS:
        c = PLUGIN
        D = c["D"]
        torch.manual_seed(c["seed"])
        model = fr.build_model(c["mode"], c["layers"], c["act"])
        t, W = fr.fetch_minibatch(M, N, D, T, rng=np.random.RandomState(7))
        Xi = torch.ones((1, D), dtype=torch.float32)
        prob = AmericanProblem("call", D, "put_sum", c["strike"], PEN)
        bias = output_bias(model)
        with torch.no_grad():
            bias.fill_(0.0)
        r0 = fr.loss_and_grads(copy.deepcopy(model).double(), prob, t.double(), W.double(), Xi.double(), M, D)
        gap = payoff_np("put_sum", c["strike"], r0["X"][:, :-1, :]) - r0["Y"][:, :-1, 0]
        with torch.no_grad():
            bias.fill_(round(float(np.median(gap)), 2))
        _REFS["plugin"] = bundle(model, prob, t, W, Xi, M)
    return _REFS["plugin"]
