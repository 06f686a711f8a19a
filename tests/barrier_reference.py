"""References for the knock-out (barrier) problem (problem kind 11,
DBSDE_PROB_BARRIER; ProblemSpec(kind="diag", barrier=B)) -- test infrastructure
only, numpy and float64 torch, no GPU.

The model: the DIAG process, monitored at the grid times.  The statistic of a
row is the payoff's own over its g_cols columns, in float32, in the documented
row-sum order (tests/asian_reference.py row_sum); a call path is knocked at the
first row with stat <= B (row 0 counts), a put path at the first row with
stat >= B.  Training runs on the stopped process: rows n > tau hold X_tau, the
sigma dW rows n >= tau are 0, t keeps running.

  * stat / stop / rollout: the float32 chain (oracle.philox.rollout's rows, then
    the row rule);
  * BarrierProblem, loss_and_grads: the FBSNN loss of oracle.fbsnn_ref on the
    stopped process in float64 torch autograd on given increments, with THE
    STOPPING INDEX OF THE FLOAT32 CHAIN (a statistic within rounding of B cannot
    make the oracle stop elsewhere); cotangents: the same loss's derivatives in
    the network outputs, written by hand;
  * mc_value: dbsde_mc_value's restatement on the Philox draws, with every alive
    flag and each sample's margin to the barrier;
  * closed_form: the Reiner-Rubinstein price with the Broadie-Glasserman-Kou
    shift, restated;
  * arbiter: at k = 1 and N = 2 the scheme's expectation by quadrature.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

import asian_reference as ar
import mc_reference as mr
import put_reference as pr
from oracle import fbsnn_ref as fr
from oracle import philox as ph

f32 = np.float32
T = 1.0
COEF = dict(mu_a=0.05, sig_a=0.20, sig_b=0.0)
R_RATE = 0.05
PUTS = ("put_sum", "put_mean")
MEANS = ("call_mean", "put_mean")
# a statistic closer than this to B (times the number of columns of a sum) may sit on the other side on the device,
# whose normals differ from numpy's by up to 2e-6 (tests/mc_reference.py AMBIGUOUS)
MARGIN = mr.AMBIGUOUS


def sign_of(payoff):
    return -1.0 if payoff in PUTS else 1.0


# ---------------------------------------------------------------- the fp32 chain
def stat(Xc, payoff):
    """[M] float32: the monitored statistic of the payoff columns Xc [M, cols]."""
    Xc = np.asarray(Xc, f32)
    s = ar.row_sum(Xc)
    if payoff in MEANS:
        s = s / f32(Xc.shape[1])
    assert s.dtype == f32
    return s


def hit(s, B, payoff):
    return (s >= f32(B)) if payoff in PUTS else (s <= f32(B))


def stop(X, sdw, payoff, B, cols=0):
    """The row rule on unstopped rows X [M, N+1, D], sdw [M, N, D] (float32):
    (X stopped, sdw stopped, tau [M] with N + 1 for a path that never hits,
    stats [M, N+1] of the unstopped rows)."""
    X, sdw = np.array(X, f32), np.array(sdw, f32)
    M, N1, D = X.shape
    c = cols if 0 < cols < D else D
    stats = np.stack([stat(X[:, n, :c], payoff) for n in range(N1)], 1)
    h = hit(stats, B, payoff)
    tau = np.where(h.any(1), h.argmax(1), N1)
    for m in range(M):
        if tau[m] < N1:
            X[m, tau[m] + 1:] = X[m, tau[m]]
            sdw[m, tau[m]:] = 0
    return X, sdw, tau, stats


def rollout(Xi, dw, T, payoff, B, cols=0, tgrid=None, mu_a=0.05, sig_a=0.20, sig_b=0.0):
    """dict(X, sdw: the stopped rows; tau; stats; X0: the unstopped rows) from
    increments dw [M, N, D] on the reference grid or a caller's grid [M, N+1]."""
    dw = np.asarray(dw, f32)
    X0 = ph.rollout(Xi, dw, T, mu_a, sig_a, sig_b, tgrid)
    sdw0 = (f32(sig_a) * X0[:, :-1] + f32(sig_b)) * dw
    X, sdw, tau, stats = stop(X0, sdw0, payoff, B, cols)
    return dict(X=X, sdw=sdw, tau=tau, stats=stats, X0=X0)


def margin(stats, tau, B, cols, payoff):
    """[M]: the smallest |stat - B| over the rows that decide tau (0..tau), in
    units of MARGIN (times cols for a sum statistic)."""
    M, N1 = stats.shape
    unit = MARGIN * (1 if payoff in MEANS else cols)
    out = np.empty(M)
    for m in range(M):
        out[m] = np.abs(stats[m, :min(tau[m], N1 - 1) + 1].astype(np.float64) - float(f32(B))).min() / unit
    return out


# ---------------------------------------------------------------- the problem (torch)
class BarrierProblem:
    """mu, sigma, phi and g of the DIAG problem behind the barrier, in the dtype of X."""

    kind, q3_compat = "diag", False

    def __init__(self, D, payoff="call_mean", strike=1.0, cols=0, mu_a=0.05, sig_a=0.20, sig_b=0.0, phi_r=R_RATE,
                 phi_c=0.0):
        self.D, self.payoff, self.strike = D, payoff, float(strike)
        self.cols = cols if 0 < cols < D else D
        self.mu_a, self.sig_a, self.sig_b, self.phi_r, self.phi_c = mu_a, sig_a, sig_b, phi_r, phi_c

    def mu(self, t, X, Y=None, Z=None):
        return self.mu_a * X

    def sigma(self, t, X, Y=None):
        return torch.diag_embed(self.sig_a * X + self.sig_b)

    def phi(self, t, X, Y, Z):
        return self.phi_r * (Y - self.phi_c * torch.sum(X * Z, dim=1, keepdim=True))

    def g(self, X):
        S = X[:, :self.cols]
        a = (torch.mean(S, dim=1, keepdim=True) if self.payoff in MEANS else torch.sum(S, dim=1, keepdim=True)) - self.strike
        if self.payoff in PUTS:
            a = -a
        return torch.maximum(a, torch.tensor(0.0, dtype=X.dtype))


def spec(pkg, payoff="call_mean", strike=1.0, barrier=0.9, cols=0, phi_c=0.0, **coef):
    c = dict(COEF, **coef)
    return pkg.ProblemSpec(phi_r=R_RATE, phi_c=phi_c, g=payoff, strike=strike, g_cols=cols, q3=False, barrier=barrier, **c)


def loss_and_grads(model, prob, tgrid, dw, Xi, tau):
    """oracle.fbsnn_ref.loss_function on the stopped process, in float64 on
    increments dw [M, N, D] and the grid tgrid [N+1]; tau [M] is the stopping row
    of the float32 chain (N + 1: never; None: the unstopped DIAG problem).
    dict(loss, X, Y, Z, grad, used)."""
    model = copy.deepcopy(model).double()
    model.zero_grad(set_to_none=True)
    D = prob.D
    dw = torch.as_tensor(np.asarray(dw, np.float64))
    tg = torch.as_tensor(np.asarray(tgrid, np.float64))
    M, Nn, _ = dw.shape
    tau = np.full(M, Nn + 1) if tau is None else np.asarray(tau)
    X0 = torch.as_tensor(np.broadcast_to(np.asarray(Xi, np.float64).reshape(-1, D), (M, D)).copy())
    X0.requires_grad_(True)
    tcol = lambda n: tg[n].expand(M, 1)
    Y0, Z0 = fr.net_u(model, tcol(0), X0)
    Xs, Ys, Zs = [X0], [Y0], [Z0]
    loss = 0
    for n in range(Nn):
        dt = tg[n + 1] - tg[n]
        live = torch.as_tensor((tau > n).astype(np.float64)).reshape(M, 1)     # row n steps on: n < tau
        s = live * torch.squeeze(torch.matmul(prob.sigma(tcol(n), X0, Y0), dw[:, n].unsqueeze(-1)), dim=-1)
        X1 = X0 + live * (prob.mu(tcol(n), X0, Y0, Z0) * dt) + s
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
    c = prob.cols
    loss = loss + torch.sum(torch.pow(Z1[:, :c] - dg[:, :c], 2))
    loss.backward()
    grad, mask = fr.flat_grads(model)
    return dict(loss=float(loss.detach()), X=torch.stack(Xs, 1).detach().numpy(), Y=torch.stack(Ys, 1).detach().numpy(),
                Z=torch.stack(Zs, 1).detach().numpy(), grad=np.asarray(grad, np.float64), used=mask)


def row_loss(prob, tgrid, X, sdw, U, DU):
    """The loss as a function of the network outputs U [M, N+1, 1], DU [M, N+1, D]
    (torch float64) on given rows X [M, N+1, D], sdw [M, N, D]."""
    tg = torch.as_tensor(np.asarray(tgrid, np.float64))
    X, sdw = torch.as_tensor(np.asarray(X, np.float64)), torch.as_tensor(np.asarray(sdw, np.float64))
    N = X.shape[1] - 1
    loss = 0
    for n in range(N):
        dt = tg[n + 1] - tg[n]
        Y1t = U[:, n] + prob.phi(None, X[:, n], U[:, n], DU[:, n]) * dt + torch.sum(DU[:, n] * sdw[:, n], 1, keepdim=True)
        loss = loss + torch.sum((U[:, n + 1] - Y1t) ** 2)
    XN = X[:, N].clone().requires_grad_(True)
    g = prob.g(XN)
    dg = torch.autograd.grad(g.sum(), XN)[0]
    c = prob.cols
    return loss + torch.sum((U[:, N] - g.detach()) ** 2) + torch.sum((DU[:, N, :c] - dg[:, :c]) ** 2)


def cotangents(prob, tgrid, X, sdw, U, DU):
    """d loss / dU [M, N+1, 1] and d loss / dDU [M, N+1, D] of row_loss, by hand
    (numpy float64).  With r_n = U_{n+1} - U_n - phi_n dt_n - DU_n . sdw_n and
    phi = phi_r (U - phi_c X . DU):
        dL/dU_n  = 2 r_{n-1} - 2 r_n (1 + phi_r dt_n)                         (r_{-1} = 0)
        dL/dU_N  = 2 r_{N-1} + 2 (U_N - g(X_N))
        dL/dDU_n = -2 r_n (sdw_n - phi_r phi_c dt_n X_n)
        dL/dDU_N = 2 (DU_N - dg(X_N)) on the payoff columns, 0 elsewhere
    On a frozen row sdw_n = 0 and X_n = X_tau; on a knocked terminal row g = 0
    and dg = 0 (the regular barriers), so the same formulas teach u = 0, Du = 0."""
    tg = np.asarray(tgrid, np.float64)
    X, sdw, U, DU = (np.asarray(v, np.float64) for v in (X, sdw, U, DU))
    M, N1, D = X.shape
    N = N1 - 1
    dt = (tg[1:] - tg[:-1]).reshape(1, N, 1)
    phi = prob.phi_r * (U[:, :N] - prob.phi_c * np.sum(X[:, :N] * DU[:, :N], 2, keepdims=True))
    r = U[:, 1:] - U[:, :N] - phi * dt - np.sum(DU[:, :N] * sdw, 2, keepdims=True)
    ub, zb = np.zeros_like(U), np.zeros_like(DU)
    ub[:, 1:] += 2 * r
    ub[:, :N] -= 2 * r * (1 + prob.phi_r * dt)
    zb[:, :N] = -2 * r * (sdw - prob.phi_r * prob.phi_c * dt * X[:, :N])
    XN = torch.as_tensor(X[:, N]).requires_grad_(True)
    g = prob.g(XN)
    dg = torch.autograd.grad(g.sum(), XN)[0].numpy()
    c = prob.cols
    ub[:, N] += 2 * (U[:, N] - g.detach().numpy())
    zb[:, N, :c] += 2 * (DU[:, N, :c] - dg[:, :c])
    return ub, zb


# ---------------------------------------------------------------- the cases
def xi_rows(D, M, lo=0.8, hi=1.2):
    """Per-path initial states [M, D]: prices 1 scaled lo..hi over the paths, so
    the first paths start beyond a barrier below (the last ones beyond one above)."""
    return (np.ones((M, D)) * np.linspace(lo, hi, M)[:, None]).astype(f32)


def level(payoff, D, cols, x):
    """A strike or barrier at `x` per asset in the statistic's units."""
    c = cols if 0 < cols < D else D
    return x if payoff in MEANS else x * c


# rows: (k, M, N, payoff, cols, barrier per asset, xi range over the paths, seed, coefficients).  k = 17 crosses the
# 16-lane group, 130 is Dp > 128; N is ragged against the four-row blocks; both directions, sum and mean statistics; a
# payoff on fewer columns than D.  The mean of many assets barely moves (0.2 sqrt(t / k)), so the wide cases start
# close to the barrier, and the k = 130 call drifts down towards it (mu_a = -0.05).  Seeds: the first that shows
# tests/test_barrier_cpu.py's coverage with every deciding statistic more than MARGIN from the barrier.
_DOWN = dict(mu_a=-0.05, sig_a=0.20, sig_b=0.0)
ROW_CASES = {
    "k1_call_sum": (1, 70, 7, "call_sum", 0, 0.93, (0.8, 1.2), 1, COEF),
    "k3_put_mean": (3, 70, 5, "put_mean", 0, 1.06, (0.8, 1.2), 1, COEF),
    "k3_call_cols2": (3, 5, 1, "call_sum", 2, 0.95, (0.8, 1.2), 18, COEF),
    "k17_put_sum": (17, 70, 7, "put_sum", 0, 1.03, (0.8, 1.2), 1, COEF),
    "k17_call_mean": (17, 5, 5, "call_mean", 0, 0.97, (0.94, 1.02), 12, COEF),
    "k130_call_mean": (130, 70, 5, "call_mean", 0, 0.98, (0.96, 1.07), 1, _DOWN),
    "k130_put_mean": (130, 70, 5, "put_mean", 0, 1.02, (0.93, 1.04), 1, COEF),
    "k130_put_sum": (130, 5, 1, "put_sum", 0, 1.01, (0.8, 1.2), 1, COEF),
}


def row_case(name):
    k, M, N, payoff, cols, bar, (lo, hi), seed, coef = ROW_CASES[name]
    return dict(k=k, M=M, N=N, payoff=payoff, cols=cols, seed=seed, strike=level(payoff, k, cols, 1.0),
                barrier=level(payoff, k, cols, bar), xi=xi_rows(k, M, lo, hi), coef=dict(coef))


# loss cases: name -> (k, M, N, payoff, cols, barrier per asset, strike per asset, xi range, mode, activation, layers
# behind the input width, environment while the context is created, phi_c, seed)
LOSS_CASES = {
    "fused16_k3": (3, 24, 6, "call_mean", 0, 0.94, 1.0, (0.9, 1.1), "NAIS-Net", "Sine", 4 * [16] + [1], {}, 0.0, 3),
    "chain16_k3": (3, 24, 6, "put_sum", 0, 1.06, 1.0, (0.9, 1.1), "NAIS-Net", "Sine", 4 * [16] + [1],
                   {"DBSDE_FUSED": "0"}, 1.0, 5),
    "wide_k130": (130, 20, 6, "call_mean", 0, 0.985, 1.0, (0.975, 1.0), "FC", "Tanh", [64, 32, 16, 1], {}, 0.0, 5),
}


def loss_case(name):
    k, M, N, payoff, cols, bar, strike, (lo, hi), mode, act, tail, env, phi_c, seed = LOSS_CASES[name]
    return dict(k=k, M=M, N=N, payoff=payoff, cols=cols, barrier=level(payoff, k, cols, bar),
                strike=level(payoff, k, cols, strike), mode=mode, act=act, layers=[k + 1] + tail, env=env, phi_c=phi_c,
                seed=seed, xi=xi_rows(k, M, lo, hi), coef=dict(COEF))


_MODELS = {}


def loss_model(name):
    """(oracle model (float32), flat params); the cases of one network share it."""
    c = loss_case(name)
    key = (c["k"], c["mode"], c["act"], tuple(c["layers"]))
    if key not in _MODELS:
        torch.manual_seed(400 + c["k"] + len(c["layers"]))
        model = fr.build_model(c["mode"], c["layers"], c["act"])
        _MODELS[key] = (model, fr.flat_params(model))
    return _MODELS[key]


def loss_problem(name):
    c = loss_case(name)
    return BarrierProblem(c["k"], c["payoff"], c["strike"], c["cols"], phi_c=c["phi_c"], **COEF)


def coverage(tau, N):
    """What a case must show: the knocked fraction and paths with tau = 0, tau = N, never."""
    tau = np.asarray(tau)
    return dict(knocked=float(np.mean(tau <= N)), first=int(np.sum(tau == 0)), last=int(np.sum(tau == N)),
                never=int(np.sum(tau > N)))


# ---------------------------------------------------------------- Monte-Carlo value
def payoff(sp, X):
    fn = pr.payoff if sp.g in PUTS else mr.payoff
    return fn(sp, X)


def mc_paths(sp, tau, x, n_steps, mc, seed, offset=0, L=None):
    """(X [mc, n_steps + 1, D] float32 unstopped, stats [mc, n_steps + 1], alive [mc])
    of one point on the device's draws."""
    x = np.asarray(x, f32).reshape(-1)
    dw = ph.increments(seed, offset, 0, mc, n_steps, x.size, tau, L)
    X = ph.rollout(x, dw, tau, mu_a=mr.mu_eff(sp), sig_a=sp.sig_a, sig_b=sp.sig_b)
    c = mr.g_cols(sp, x.size)
    stats = np.stack([stat(X[:, n, :c], sp.g) for n in range(n_steps + 1)], 1)
    return X, stats, ~hit(stats, sp.barrier, sp.g).any(1)


def mc_value(sp, t, X, T_, n_steps, mc, seed=0, offset=0, L=None):
    """dict(value [P], stderr [P], alive [P, mc], margin [P] = the smallest margin
    of any sample of the point (in MARGIN units), ambiguous [P] = samples within
    MARGIN of the payoff's kink) -- exp(-phi_r tau) mean_k g(X_N) alive_k and the
    standard error of the same summand."""
    t = np.asarray(t, f32).reshape(-1)
    X = np.asarray(X, f32).reshape(t.size, -1)
    P, D = X.shape
    c = mr.g_cols(sp, D)
    out = dict(value=np.zeros(P), stderr=np.zeros(P), alive=np.zeros((P, mc), bool), margin=np.full(P, np.inf),
               ambiguous=np.zeros(P, int))
    for p in range(P):
        tau = float(f32(T_) - t[p])
        if tau <= 0:
            g, _, _ = payoff(sp, X[p:p + 1])
            live = not bool(hit(stat(X[p:p + 1, :c], sp.g), sp.barrier, sp.g)[0])
            out["value"][p] = g[0] if live else 0.0
            out["alive"][p] = live
            continue
        Xp, stats, alive = mc_paths(sp, tau, X[p], n_steps, mc, seed, offset, L)
        h = hit(stats, sp.barrier, sp.g)
        tau_k = np.where(h.any(1), h.argmax(1), n_steps + 1)
        out["margin"][p] = margin(stats, tau_k, sp.barrier, c, sp.g).min()
        g, _, a = payoff(sp, Xp[:, -1])
        out["ambiguous"][p] = int(np.sum((np.abs(a) < mr.AMBIGUOUS) & alive))
        g = g * alive
        disc = np.exp(-float(f32(sp.phi_r)) * tau)
        out["value"][p] = disc * np.mean(g)
        out["stderr"][p] = disc * np.std(g, ddof=1) / np.sqrt(mc) if mc > 1 else 0.0
        out["alive"][p] = alive
    return out


# same-draws cases: (k, n_steps, mc, payoff, barrier per asset, factor, seed); the points sit at t = 0, 0.25, 0.5 and T.
# Seeds: the first from 2 on at which no sample's deciding statistic lies within MARGIN of the barrier, no live
# sample within it of the kink, and between 10 % and 90 % of the samples of every running point stay alive
MC_T_POINTS = np.array([0.0, 0.25, 0.5, 1.0, 1.0], f32)
MC_CASES = {
    "k1_call": (1, 6, 512, "call_sum", 0.9, False, 2),
    "k3_put_mean": (3, 6, 512, "put_mean", 1.1, False, 2),
    "k3_put_mean-factor": (3, 6, 512, "put_mean", 1.1, True, 3),
    "k8_call_mean": (8, 5, 512, "call_mean", 0.97, False, 4),
    "k8_call_mean-factor": (8, 5, 512, "call_mean", 0.93, True, 2),
    "k100_put_sum": (100, 3, 256, "put_sum", 1.02, False, 19),
    "k100_call_sum-factor": (100, 3, 256, "call_sum", 0.975, True, 2),
}


def mc_points(k, payoff, bar):
    """Five points: three live ones, one at t = T live and in the money, one at t = T beyond the barrier."""
    rs = np.random.RandomState(11 + k)
    X = rs.uniform(0.97, 1.05, (5, k)) if payoff not in PUTS else rs.uniform(0.95, 1.03, (5, k))
    X[3] = 1.04 if payoff not in PUTS else 0.96
    X[4] = bar - 0.02 if payoff not in PUTS else bar + 0.02
    return X.astype(f32)


def mc_setup(pkg, name):
    k, n_steps, mc, pay, bar, corr, seed = MC_CASES[name]
    sp = spec(pkg, pay, strike=level(pay, k, 0, 1.0), barrier=level(pay, k, 0, bar))
    return dict(k=k, n_steps=n_steps, mc=mc, spec=sp, seed=seed, X=mc_points(k, pay, bar), t=MC_T_POINTS,
                L=ar.equicorr_L(k) if corr else None)


_MC = {}


def mc_case(pkg, name):
    if name not in _MC:
        c = mc_setup(pkg, name)
        _MC[name] = mc_value(c["spec"], c["t"], c["X"], T, c["n_steps"], c["mc"], seed=c["seed"], L=c["L"])
    return _MC[name]


# ---------------------------------------------------------------- closed form
BGK = 0.5826


def closed_form(S, tau, r, sig, K, b, B, n_mon, put):
    """(price, delta) float64 of the down-and-out call / up-and-out put without
    rebate (Reiner-Rubinstein) at S, tau (arrays), the barrier first shifted by
    exp(-+0.5826 sigma sqrt(tau / n_mon)) when n_mon > 0; 0 on the knocked side;
    tau <= 0: the payoff and its kink delta, 0 when knocked."""
    from scipy.special import erfc
    S, tau = np.broadcast_arrays(np.asarray(S, np.float64), np.asarray(tau, np.float64))
    N_ = lambda x: 0.5 * erfc(-x * 0.70710678118654752440)
    f = -1.0 if put else 1.0
    run = tau > 0
    tt = np.where(run, tau, 1.0)
    Bs = B * np.exp(-f * BGK * sig * np.sqrt(tt / n_mon)) if n_mon > 0 else np.full_like(tt, B)
    s = sig * np.sqrt(tt)
    lam = (b - 0.5 * sig * sig) / (sig * sig)
    x1 = np.log(S / K) / s + (1 + lam) * s
    y1 = np.log(Bs * Bs / (S * K)) / s + (1 + lam) * s
    cf, df = np.exp((b - r) * tt), np.exp(-r * tt)
    pw0 = (Bs / S) ** (2 * lam)
    pw1 = pw0 * (Bs / S) ** 2
    A = f * S * cf * N_(f * x1) - f * K * df * N_(f * x1 - f * s)
    C = f * S * cf * pw1 * N_(f * y1) - f * K * df * pw0 * N_(f * y1 - f * s)
    delta = f * cf * N_(f * x1) + f * cf * (2 * lam + 1) * pw1 * N_(f * y1) - 2 * lam * f * K * df * pw0 * N_(f * y1 - f * s) / S
    live = (S < Bs) if put else (S > Bs)
    price, delta = np.where(live, A - C, 0.0), np.where(live, delta, 0.0)
    a = f * (S - K)
    live0 = (S < B) if put else (S > B)
    pay = np.where(live0, np.maximum(a, 0.0), 0.0)
    dpay = np.where(live0, f * np.where(a > 0, 1.0, np.where(a == 0, 0.5, 0.0)), 0.0)
    return np.where(run, price, pay), np.where(run, delta, dpay)


def bs_carry(S, K, tau, r, sig, b, put):
    """The vanilla Black-Scholes price with cost of carry b (the B -> 0+ / B -> inf limit)."""
    from scipy.stats import norm
    S, tau = np.asarray(S, np.float64), np.asarray(tau, np.float64)
    st = sig * np.sqrt(tau)
    d1 = (np.log(S / K) + (b + 0.5 * sig * sig) * tau) / st
    d2 = d1 - st
    if put:
        return K * np.exp(-r * tau) * norm.cdf(-d2) - S * np.exp((b - r) * tau) * norm.cdf(-d1)
    return S * np.exp((b - r) * tau) * norm.cdf(d1) - K * np.exp(-r * tau) * norm.cdf(d2)


# ---------------------------------------------------------------- the two-step arbiter
ARBITER = dict(r=0.05, b=0.10, sig=0.2, K=1.0, x=1.0, T=1.0, n_steps=2, mc=1 << 18, seed=9,
               call=dict(B=0.95, value=0.131094), put=dict(B=1.05, value=0.034490))


def arbiter(put, B, r=0.05, b=0.10, sig=0.2, K=1.0, x=1.0, T_=1.0, nodes=400):
    """The expectation of the scheme at k = 1, N = 2, exactly: X_1 = x (1 + b dt)
    + sig x sqrt(dt) z is Gaussian; given X_1, X_2 is Gaussian with mean
    X_1 (1 + b dt) and standard deviation sig |X_1| sqrt(dt), so E[g(X_2) | X_1] is
    a Bachelier formula, and since g vanishes beyond the regular barrier the
    monitoring of row 2 changes nothing.  The value is exp(-r T) times its
    integral over the live half-line of X_1 (x itself is live), by Gauss-Legendre
    on [B, m + 12 s] (call) or [m - 12 s, B] (put) in panels, float64."""
    from scipy.stats import norm
    dt = T_ / 2
    m1, s1 = x * (1 + b * dt), sig * abs(x) * np.sqrt(dt)
    if (put and x >= B) or (not put and x <= B):
        return 0.0
    lo, hi = (m1 - 12 * s1, B) if put else (B, m1 + 12 * s1)
    z, w = np.polynomial.legendre.leggauss(nodes)
    total = 0.0
    panels = 8
    edges = np.linspace(lo, hi, panels + 1)
    for a_, b_ in zip(edges[:-1], edges[1:]):
        y = 0.5 * (b_ - a_) * z + 0.5 * (a_ + b_)
        m2, s2 = y * (1 + b * dt), sig * np.abs(y) * np.sqrt(dt)
        d = (m2 - K) / s2
        bach = (m2 - K) * norm.cdf(d) + s2 * norm.pdf(d)             # E max(X_2 - K, 0)
        if put:
            bach = bach - (m2 - K)                                   # E max(K - X_2, 0)
        total += 0.5 * (b_ - a_) * np.sum(w * bach * norm.pdf((y - m1) / s1) / s1)
    return float(np.exp(-r * T_) * total)


def arbiter_mc(put, B, n=1 << 22, seed=5, r=0.05, b=0.10, sig=0.2, K=1.0, x=1.0, T_=1.0):
    """(value, stderr) of the same two-step scheme by numpy Monte Carlo in float64."""
    rs = np.random.RandomState(seed)
    dt = T_ / 2
    z = rs.standard_normal((n, 2))
    x1 = x * (1 + b * dt) + sig * x * np.sqrt(dt) * z[:, 0]
    x2 = x1 * (1 + b * dt) + sig * x1 * np.sqrt(dt) * z[:, 1]
    if put:
        alive = (x < B) & (x1 < B) & (x2 < B)
        g = np.maximum(K - x2, 0.0) * alive
    else:
        alive = (x > B) & (x1 > B) & (x2 > B)
        g = np.maximum(x2 - K, 0.0) * alive
    d = np.exp(-r * T_)
    return d * g.mean(), d * g.std(ddof=1) / np.sqrt(n)
