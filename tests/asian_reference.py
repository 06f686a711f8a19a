"""References for the arithmetic-average (Asian) problem (problem kind 4,
DBSDE_PROB_ASIAN; ProblemSpec(kind="diag", average=True)) -- test
infrastructure only.

The model: state [A, S_1..S_k], Brownian dimension k (column i of the
increments drives S_i, A has no diffusion).  The step of include/dbsde.h,
restated, every operation rounded to fp32 on its own:

    s_i  = (sig_a S_i + sig_b) dW_i         S_i' = (S_i + (mu_a S_i) dt) + s_i
    p_l  = ((0 + S_l) + S_{l+16}) + ...     l = 0..15, ascending over the assets
    p_l <- p_l + p_{l xor o}                o = 1, 2, 4, 8 in turn;  sum = p_0
    m    = sum / fp32(k)                    A' = A + (m dt) / T

  * row_sum / rollout: that chain in float32 numpy (the S columns are
    oracle.philox.rollout's);
  * AsianProblem, loss_and_grads: the FBSNN loss of oracle.fbsnn_ref.loss_function
    on this process in float64 torch autograd on given increments, built on
    oracle.fbsnn_ref.net_u; the terminal Z term runs over the payoff column A
    alone (g_cols = 1), as the device's does;
  * pde_terms: tests/jet_reference.py's pde_terms with AsianProblem's mu and
    its [R, 1 + k, k] diffusion matrix;
  * mc_value: dbsde_mc_value's restatement -- A_T = A_p + (sum_d I_d) / (k T),
    I_d = sum_n fp64(fp32(S_{d,n} dt_n)) on oracle.philox.rollout's paths, with
    tests/mc_reference.py's and tests/put_reference.py's payoffs on one column;
  * euler_expectation: the exact expectation of the scheme for strike 0.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

import jet_reference as jr
import mc_reference as mr
import put_reference as pr
from oracle import fbsnn_ref as fr
from oracle import philox as ph

f32 = np.float32
T = 1.0
N = 6                              # the last 4-step Philox block is half used
KS = (1, 3, 17, 70, 130)           # fused 16; a ragged 16-block; the wide chain (Dp > 128)
MS = (24, 7)
COEF = dict(mu_a=0.05, sig_a=0.20, sig_b=0.0)
R_RATE = 0.05
LANES = 16


def xi_state(k, A0=0.0):
    """[A, S_1..S_k] = [A0, 1..] as one row."""
    return np.concatenate([[[A0]], np.ones((1, k))], 1)


def equicorr_L(k, rho=0.3):
    return np.linalg.cholesky((1 - rho) * np.eye(k) + rho * np.ones((k, k))).astype(f32)


# ---------------------------------------------------------------- the fp32 chain
def row_sum(S):
    """[M] float32: the sum over the k columns of S [M, k] in the documented order."""
    S = np.asarray(S, f32)
    M, k = S.shape
    p = np.zeros((M, LANES), f32)
    for l in range(LANES):
        for i in range(l, k, LANES):
            p[:, l] = p[:, l] + S[:, i]
    o = 1
    while o < LANES:
        p = p + p[:, np.arange(LANES) ^ o]
        o <<= 1
    assert p.dtype == f32
    return p[:, 0]


def average(S, dts, A0, T):
    """A [M, N+1] float32 from the asset paths S [M, N+1, k], the steps dts (N
    scalars or [M, 1] columns, oracle.philox._dts) and A_0 [M]."""
    M, N1, k = S.shape
    A = np.empty((M, N1), f32)
    a = np.broadcast_to(np.asarray(A0, f32).reshape(-1), (M,)).astype(f32)
    for n in range(N1 - 1):
        A[:, n] = a
        m = row_sum(S[:, n]) / f32(k)
        a = a + (m * np.asarray(dts[n], f32).reshape(-1)) / f32(T)
        assert a.dtype == f32
    A[:, N1 - 1] = a
    return A


def rollout(Xi, dw, T, mu_a=0.05, sig_a=0.20, sig_b=0.0, tgrid=None):
    """X [M, N+1, 1 + k] and sdw [M, N, 1 + k] float32 from increments dw
    [M, N, k] on the reference grid, or on a caller's grid tgrid [M, N+1]."""
    M, Nn, k = dw.shape
    dw = np.asarray(dw, f32)
    x = np.broadcast_to(np.asarray(Xi, f32).reshape(-1, 1 + k), (M, 1 + k))
    S = ph.rollout(x[:, 1:], dw, T, mu_a, sig_a, sig_b, tgrid)
    A = average(S, ph._dts(Nn, T, tgrid), x[:, 0], T)
    X = np.concatenate([A[:, :, None], S], 2)
    sdw = np.zeros((M, Nn, 1 + k), f32)
    sdw[:, :, 1:] = (f32(sig_a) * S[:, :-1] + f32(sig_b)) * dw
    return X, sdw


# ---------------------------------------------------------------- the problem (torch)
class AsianProblem:
    """mu, sigma, phi and g of the problem in the dtype of X, for
    tests/jet_reference.py and the loss below.  payoff: one of the six call /
    put kinds, all on the A column."""

    kind, q3_compat = "asian", False

    def __init__(self, k, payoff="call_mean", strike=1.0, alpha=10.0, T=T, mu_a=0.05, sig_a=0.20, sig_b=0.0,
                 phi_r=R_RATE):
        self.k, self.D, self.payoff, self.strike, self.alpha, self.T = k, k + 1, payoff, float(strike), float(alpha), T
        self.mu_a, self.sig_a, self.sig_b, self.phi_r = mu_a, sig_a, sig_b, phi_r

    def mu(self, t, X, Y=None, Z=None):
        S = X[:, 1:]
        return torch.cat([torch.mean(S, dim=1, keepdim=True) / self.T, self.mu_a * S], dim=1)

    def sigma(self, t, X, Y=None):
        A = torch.diag_embed(self.sig_a * X[:, 1:] + self.sig_b)
        return torch.cat([torch.zeros_like(A[:, :1, :]), A], dim=1)

    def phi(self, t, X, Y, Z):
        return self.phi_r * Y

    def g(self, X):
        a = X[:, :1] - self.strike
        if self.payoff in pr.PAYOFFS:
            a = -a
        if self.payoff in ("smooth_call", "smooth_put"):
            return a / (1 + torch.exp(-self.alpha * a))
        return torch.maximum(a, torch.tensor(0.0, dtype=X.dtype))


def spec(pkg, payoff="call_mean", strike=1.0, **coef):
    c = dict(COEF, **coef)
    return pkg.ProblemSpec(phi_r=R_RATE, phi_c=0.0, g=payoff, strike=strike, g_alpha=10.0, g_cols=1, q3=False,
                           average=True, **c)


# ---------------------------------------------------------------- loss and gradient (fp64)
# name -> (k, M, mode, activation, layers behind the input width, environment while the context is created)
LOSS_SEED = 4
LOSS_STRIKE = 1.02         # A_T is about 1.02 +- 0.12 / sqrt(k): rows on both sides of the kink (test_asian_cpu.py)
_X3 = {"DBSDE_X3": "1", "DBSDE_TNW_X3": "1"}
_FP32 = {"DBSDE_X3": "0", "DBSDE_TNW_X3": "0"}
LOSS_CASES = {
    "fused16_k3": (3, 24, "NAIS-Net", "Sine", 4 * [16] + [1], {}),
    "fused110_k99_x3": (99, 24, "NAIS-Net", "Sine", 4 * [110] + [1], _X3),
    "fused110_k99_fp32": (99, 24, "NAIS-Net", "Sine", 4 * [110] + [1], _FP32),
    "chain110_k99": (99, 24, "NAIS-Net", "Sine", 4 * [110] + [1], {"DBSDE_FUSED": "0"}),
    "wide_k130": (130, 7, "FC", "Tanh", [64, 32, 16, 1], {}),
}


def loss_layers(case):
    k = LOSS_CASES[case][0]
    return [k + 2] + LOSS_CASES[case][4]


_MODELS = {}


def loss_model(case):
    """(oracle model (float32), flat params); the cases of one network share it."""
    k, _, mode, act, tail, _ = LOSS_CASES[case]
    key = (k, mode, act, tuple(tail))
    if key not in _MODELS:
        torch.manual_seed(200 + k + len(tail))
        model = fr.build_model(mode, [k + 2] + tail, act)
        _MODELS[key] = (model, fr.flat_params(model))
    return _MODELS[key]


def loss_and_grads(model, prob, tgrid, dw, Xi):
    """oracle.fbsnn_ref.loss_function on the problem's process, in float64 on
    increments dw [M, N, k] and the grid tgrid [N+1]: dict(loss, X, Y, Z, grad,
    used).  The terminal Z term runs over the A column (g_cols = 1)."""
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
        X1 = X0 + prob.mu(tcol(n), X0, Y0, Z0) * dt + s
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
    """(oracle model in float64, flat float32 params, t [R, 1], X [R, 1 + k]
    float64 holding float32 values)."""
    torch.manual_seed(300 + k)
    model = fr.build_model("Naisnet", [k + 2, 16, 16, 16, 16, 1], act)
    flat = fr.flat_params(model).astype(f32)
    rs = np.random.RandomState(seed)
    t = rs.uniform(0.0, 0.9, (R, 1)).astype(f32).astype(np.float64)
    X = np.concatenate([rs.uniform(0.0, 1.2, (R, 1)), rs.uniform(0.7, 1.4, (R, k))], 1).astype(f32).astype(np.float64)
    return copy.deepcopy(model).double(), flat, t, X


def pde_terms(model, prob, t, X, L=None):
    """The seven terms [R, 1] (float64 numpy) by double autograd."""
    return jr.pde_terms(model, prob, np.asarray(t, np.float64), np.asarray(X, np.float64),
                        None if L is None else np.asarray(L, np.float64))


# ---------------------------------------------------------------- Monte-Carlo value
def payoff(sp, A):
    """g [M], dg/dA [M] and the kink variable a [M] (None for the smooth
    payoffs) in float64 at the averages A [M]."""
    fn = pr.payoff if sp.g in pr.PAYOFFS else mr.payoff
    g, dg, a = fn(sp, np.asarray(A, np.float64).reshape(-1, 1))
    return g, dg[:, 0], a


def mc_terminal(sp, tau, x, T_, n_steps, mc, seed, offset=0, L=None, want_J=False, path0=0):
    """(A_T [mc] float64, dA_T/dS [mc, k] float64 or None) of one point on the
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
        I += (S[:, n] * dts[n]).astype(f32).astype(np.float64)
    kT = float(k) * float(f32(T_))
    AT = float(x[0]) + I.sum(1) / kT
    if not want_J:
        return AT, None
    J = np.ones((mc, k), f32)
    JI = np.zeros((mc, k))
    for n in range(n_steps):
        JI += (J * dts[n]).astype(f32).astype(np.float64)
        J = (J + (f32(mu) * J) * dts[n]) + (f32(sp.sig_a) * J) * dw[:, n]
    return AT, JI / kT


def mc_value(sp, t, X, T_, n_steps, mc, seed=0, offset=0, L=None, delta=False, chunk=1 << 15):
    """dict(value [P], stderr [P], delta [P, 1 + k] | None, ambiguous [P],
    delta_slack [P, 1 + k] | None, mean_AT [P], dA_max [P, 1 + k] | None = the
    largest |dA_T / dx_d| over the samples) as tests/mc_reference.py's mc_value
    returns them; the samples run in chunks of `chunk` paths."""
    t = np.asarray(t, f32).reshape(-1)
    X = np.asarray(X, f32).reshape(t.size, -1)
    P, D = X.shape
    out = dict(value=np.zeros(P), stderr=np.zeros(P), ambiguous=np.zeros(P, int), mean_AT=np.zeros(P),
               delta=np.zeros((P, D)) if delta else None, delta_slack=np.zeros((P, D)) if delta else None,
               dA_max=np.zeros((P, D)) if delta else None)
    for p in range(P):
        tau = float(f32(T_) - t[p])
        if tau <= 0:
            g, dg, _ = payoff(sp, X[p, :1])
            out["value"][p], out["mean_AT"][p] = g[0], X[p, 0]
            if delta:
                out["delta"][p, 0] = dg[0]
            continue
        gs, dgs, As, Js, amb_a = [], [], [], [], []
        for k0 in range(0, mc, chunk):
            AT, JI = mc_terminal(sp, tau, X[p], T_, n_steps, min(chunk, mc - k0), seed, offset, L, want_J=delta, path0=k0)
            g, dg, a = payoff(sp, AT)
            gs.append(g)
            dgs.append(dg)
            As.append(AT)
            Js.append(JI)
            amb_a.append(a)
        g, dg, AT = np.concatenate(gs), np.concatenate(dgs), np.concatenate(As)
        disc = np.exp(-float(f32(sp.phi_r)) * tau)
        out["value"][p] = disc * np.mean(g)
        out["stderr"][p] = disc * np.std(g, ddof=1) / np.sqrt(mc) if mc > 1 else 0.0
        out["mean_AT"][p] = np.mean(AT)
        amb = np.abs(np.concatenate(amb_a)) < mr.AMBIGUOUS if amb_a[0] is not None else np.zeros(mc, bool)
        out["ambiguous"][p] = int(amb.sum())
        if delta:
            dA = np.concatenate([np.ones((mc, 1)), np.concatenate(Js)], 1)        # dA_T / d[A_p, S_1..S_k]
            out["delta"][p] = disc * np.mean(dg[:, None] * dA, 0)
            out["dA_max"][p] = np.abs(dA).max(0)
            if amb_a[0] is not None:
                out["delta_slack"][p] = np.sum(np.abs(dA[amb]), 0) / mc
    return out


# the same-draws cases: tests/test_gpu_mc.py's shapes, seed and evaluation times (t = T: a point with tau <= 0,
# whose A sits exactly at the strike 1: the tie)
MC_SEED = 2
MC_T_POINTS = np.array([0.0, 0.25, 0.5, 1.0, 0.0], f32)
MC_SHAPES = ((8, 6, 4096), (3, 1, 1000))          # (k, n_steps, mc)
MC_PAYOFFS = ("call_mean", "put_mean", "smooth_call", "smooth_put", "call_sum", "put_sum")


def mc_points(k):
    """[A_p, S_1..S_k] at MC_T_POINTS: A_p about t_p (the average so far of prices about 1)."""
    S = np.random.RandomState(11).uniform(0.8, 1.3, (5, k))
    return np.concatenate([np.array([[0.0], [0.24], [0.52], [1.0], [0.0]]), S], 1).astype(f32)


_MC = {}


def mc_case(pkg, payoff, shape, corr=False):
    """The restatement of one same-draws case (with delta), computed once per process."""
    key = (payoff, shape, corr)
    if key not in _MC:
        k, n_steps, mc = shape
        _MC[key] = mc_value(spec(pkg, payoff), MC_T_POINTS, mc_points(k), T, n_steps, mc, seed=MC_SEED,
                            L=equicorr_L(k) if corr else None, delta=True)
    return _MC[key]


def smooth_g3_max(alpha=10.0):
    """The largest |third derivative| of the smooth payoffs g(a) = a / (1 +
    exp(-alpha a)), by autograd on a grid of [-3, 3] (outside it decays like
    alpha^3 |a| exp(-alpha |a|))."""
    a = torch.linspace(-3.0, 3.0, 120001, dtype=torch.float64, requires_grad=True)
    g = a / (1 + torch.exp(-alpha * a))
    for _ in range(3):
        g = torch.autograd.grad(g.sum(), a, create_graph=True)[0]
    return float(g.detach().abs().max())


def central_difference_bound(dA_max, h, alpha=10.0):
    """A_T is affine in every column of the point (sig_b = 0: S_n is linear in
    S_0), so the central difference of the value over +-h in column d differs
    from the pathwise delta by at most max|g3| h^2 max|dA_T/dx_d|^3 / 6, g3 the
    third derivative of the payoff."""
    return smooth_g3_max(alpha) * h * h * np.asarray(dA_max, np.float64) ** 3 / 6.0


def euler_expectation(x, t, T_, n_steps, mu, phi_r):
    """exp(-phi_r tau) (A_p + (1 / (k T)) sum_i S_i sum_n (1 + mu dt)^n dt), dt =
    tau / n_steps: the expectation of the scheme's discounted A_T (the value of
    the call at strike 0 while S stays positive)."""
    x = np.asarray(x, np.float64).reshape(-1)
    k = x.size - 1
    tau = T_ - t
    dt = tau / n_steps
    geo = np.sum((1.0 + mu * dt) ** np.arange(n_steps)) * dt
    return np.exp(-phi_r * tau) * (x[0] + np.sum(x[1:]) * geo / (k * T_))


# the arbiter's cases: strike 0, mu = 0.05, sigma = 0.4, N = 50, mc = 2^18, 4 stderr
ARBITER = dict(mu_a=0.05, sig_a=0.4, n_steps=50, mc=1 << 18, seed=9, ks=(1, 5), ts=(0.0, 0.5))


def arbiter_point(k):
    """[A_p, S_1..S_k]: a running average already started, unequal prices."""
    return np.concatenate([[0.3], np.linspace(0.9, 1.2, k)]).astype(f32)
