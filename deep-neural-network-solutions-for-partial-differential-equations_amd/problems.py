"""Problem classes of the reference, as FBSNN subclasses with native
coefficients (problem_spec) plus the reference's torch expressions for
phi_tf / g_tf / mu_tf / sigma_tf.  The native step runs the spec; the methods
are compared with it on probe inputs at construction (fbsnn._select_problem),
so a subclass overriding one of them with other coefficients runs its own
methods (generic.py) instead of silently training the parent's problem.

  CallOption            nd_BSPDE_case.py:503-539        sum-payoff call, phi = r(Y - X.Z)
  PutOption             (no reference counterpart)      CallOption with the put payoff max(K - sum X, 0)
  CallOption1D          1d_BSPDE_case.py:510-560        1-D call, phi = 0.01 Y (Q3 broadcast)
  BasketCallOption      with_corr...py:546-596          mean-payoff basket, correlated dW
  BasketPutOption       (no reference counterpart)      BasketCallOption with max(K - mean X, 0)
  BSPDETestCase         with_corr...py:599-616          sum X^2 payoff, mu = 0.05 X
  HamiltonJacobiBellman hjb_implement.py:590-604        phi = |Z|^2, g = log(1/2 + |X|^2/2)
  HestonFBSNN           heston_dnnpde.py:519-699        k-asset stochastic volatility
  HestonTwoFactorFBSNN  (no reference counterpart)      the two-factor Heston model on that surface
  AsianCallOption / AsianPutOption, AsianBasketCallOption / AsianBasketPutOption
                        (no reference counterpart)      arithmetic-average options: the running
                                                        average as one more state coordinate
  GeometricAsianCallOption / GeometricAsianPutOption, GeometricAsianBasketCallOption /
  GeometricAsianBasketPutOption
                        (no reference counterpart)      geometric-average options, with a closed form
  AmericanPutOption / AmericanBasketPutOption
                        (no reference counterpart)      PutOption / BasketPutOption with early exercise,
                                                        by penalisation: phi -= penalty (g(X) - Y)^+
  BarrierCallOption / BarrierPutOption, BarrierBasketCallOption / BarrierBasketPutOption
                        (no reference counterpart)      CallOption / PutOption / BasketCallOption /
                                                        BasketPutOption knocked out at a barrier
                                                        (down-and-out calls, up-and-out puts)
  BlackScholesBarenblatt: see deepbsde.py (DeepBSDE.py:326-341 surface)
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from . import networks
from .fbsnn import FBSNN
from .solver import ProblemSpec
from .solver import exact as _exact


class CallOption(FBSNN):
    """nd_BSPDE_case.py:503-539."""

    def problem_spec(self):
        return ProblemSpec(mu_a=0.05, sig_a=0.20, phi_r=0.05, phi_c=1.0, g="call_sum", strike=self.strike)

    def phi_tf(self, t, X, Y, Z):
        return 0.05 * (Y - torch.sum(X * Z, dim=1, keepdim=True))

    def g_tf(self, X):
        return torch.maximum(torch.sum(X, dim=1, keepdim=True) - self.strike, torch.tensor(0.0, device=X.device))

    def mu_tf(self, t, X, Y, Z):
        return 0.05 * X

    def sigma_tf(self, t, X, Y):
        return 0.20 * torch.diag_embed(X)


class PutOption(CallOption):
    """CallOption's problem with the put payoff max(K - sum X, 0): the same
    dynamics, phi, strike default and train surface."""

    def problem_spec(self):
        return dataclasses.replace(super().problem_spec(), g="put_sum")

    def g_tf(self, X):
        return torch.maximum(self.strike - torch.sum(X, dim=1, keepdim=True), torch.tensor(0.0, device=X.device))


class CallOption1D(FBSNN):
    """1d_BSPDE_case.py:510-560 (strike = D; the D == 1 squeeze broadcast of
    1d_BSPDE_case.py:271-273 is reproduced)."""

    def problem_spec(self):
        return ProblemSpec(mu_a=0.01, sig_a=0.25, phi_r=0.01, phi_c=0.0, g="call_sum", strike=self.strike, q3=True)

    def phi_tf(self, t, X, Y, Z):
        return 0.01 * Y

    def g_tf(self, X):
        return torch.maximum(torch.sum(X, dim=1, keepdim=True) - self.strike, torch.tensor(0.0, device=X.device))

    def mu_tf(self, t, X, Y, Z):
        return 0.01 * X

    def sigma_tf(self, t, X, Y):
        return 0.25 * torch.diag_embed(X)


class _WithCorrTrain:
    """The train() surface of with_corr_high_dimension_pde.py:355-453: log and
    record every 500 iterations (no print), return (graph, min_loss,
    min_loss_state, time_logs)."""

    schedule = "corr"
    log_every = 500
    log_print = False
    train_returns_time_logs = True


class BasketCallOption(_WithCorrTrain, FBSNN):
    """with_corr_high_dimension_pde.py:546-596 (its FBSNN sets strike = 1.0 and
    applies the N**(1/5) schedule of with_corr...:406-409)."""

    def _default_strike(self):
        return 1.0

    def problem_spec(self):
        return ProblemSpec(mu_a=0.05, sig_a=0.20, phi_r=0.05, phi_c=0.0, g="call_mean", strike=self.strike)

    def phi_tf(self, t, X, Y, Z):
        return 0.05 * (Y)

    def g_tf(self, X):
        return torch.maximum(torch.mean(X, dim=1, keepdim=True) - self.strike, torch.tensor(0.0, device=X.device))

    def mu_tf(self, t, X, Y, Z):
        return 0.05 * X

    def sigma_tf(self, t, X, Y):
        return 0.20 * torch.diag_embed(X)


class BasketPutOption(BasketCallOption):
    """BasketCallOption's problem with the put payoff max(K - mean X, 0): the
    same dynamics, phi, strike default (1.0), schedule and train surface."""

    def problem_spec(self):
        return dataclasses.replace(super().problem_spec(), g="put_mean")

    def g_tf(self, X):
        return torch.maximum(self.strike - torch.mean(X, dim=1, keepdim=True), torch.tensor(0.0, device=X.device))


class BSPDETestCase(_WithCorrTrain, FBSNN):
    """with_corr_high_dimension_pde.py:599-616."""

    def _default_strike(self):
        return 1.0

    def problem_spec(self):
        return ProblemSpec(mu_a=0.05, sig_a=0.20, phi_r=0.05, phi_c=1.0, g="sumsq")

    def phi_tf(self, t, X, Y, Z):
        return 0.05 * (Y - torch.sum(X * Z, dim=1, keepdim=True))

    def g_tf(self, X):
        return torch.sum(X ** 2, dim=1, keepdim=True)

    def mu_tf(self, t, X, Y, Z):
        return 0.05 * X

    def sigma_tf(self, t, X, Y):
        return 0.20 * torch.diag_embed(X)


class HamiltonJacobiBellman(FBSNN):
    """hjb_implement.py:590-604.  The reference passes Mm=None and therefore
    cannot train (np.ceil(None)); here Mm=None means a fixed N.
    Its train() (hjb_implement.py:394-450) logs and prints every 500
    iterations and returns (graph, min_loss, min_loss_state, time_logs)."""

    log_every = 500
    train_returns_time_logs = True

    def __init__(self, Xi, T, M, N, D, layers, mode, activation, **kw):
        super().__init__(Xi, T, M, N, D, None, layers, mode, activation, **kw)

    def _default_strike(self):
        return 1.0

    def problem_spec(self):
        return ProblemSpec(sig_b=math.sqrt(2.0), phi_zz=1.0, g="log")

    def phi_tf(self, t, X, Y, Z):
        return torch.sum(Z ** 2, dim=1, keepdim=True)

    def g_tf(self, X):
        return torch.log(0.5 + 0.5 * torch.sum(X ** 2, dim=1, keepdim=True))

    def sigma_tf(self, t, X, Y):
        return math.sqrt(2.0) * super().sigma_tf(t, X, Y)


class HestonFBSNN(FBSNN):
    """heston_dnnpde.py:519-699, generalised from one asset to k = D assets.

    State [S_1..S_k, v_1..v_k] (k = 1 is the reference's [S, v]); one Brownian
    motion per asset drives both S_i and v_i (the reference's FBSNN dimension is
    1 and its einsum broadcasts dW, :522, :638); mu and the 2x2 diffusion block
    of each asset are clamped to [-100, 100] (:591, :605); u = max(net, 0)
    (:568); phi = 0.05 Y; the terminal payoff is the call on mean S (the
    reference's max(S - 1, 0) at k = 1, or its sigmoid-smoothed "continuous"
    variant, :546-558), or with option_type="put" the put on mean S in the
    same two variants (no reference counterpart), and the terminal Z term uses dU/dS only (:654).  The
    network takes (t, S, v) -- 1 + 2k inputs -- and is initialised as the
    reference re-initialises it (xavier gain 0.5, zero biases, :580-585).
    An iteration whose loss is NaN is skipped (:409-411).  k > 1 has no
    reference golden; k = 1 is pinned by tests/golden/g1_heston_*."""

    skip_nonfinite = True
    log_print = False             # its progress print is commented out (heston_dnnpde.py:432-434)
    option_type = "call"          # "put": the put on mean S (set by the constructor)

    def __init__(self, Xi, T, M, N, D, Mm, layers, mode, activation, correlation_type="no_correlation",
                 kappa=2.0, theta=0.2, sigma=0.3, rho=0.8, v0=0.2, payoff_type='discontinuous', device=None, option_type="call"):
        if payoff_type not in ("discontinuous", "continuous"):
            raise ValueError("Invalid payoff type. Choose 'discontinuous' or 'continuous'.")
        if option_type not in ("call", "put"):
            raise ValueError("Invalid option type. Choose 'call' or 'put'.")
        self.option_type = option_type
        self.kappa, self.theta, self.sigma, self.rho, self.v0 = kappa, theta, sigma, rho, v0
        self.payoff_type = payoff_type
        self.n_assets = D
        self.Y0_values = []
        self.y0_values = []
        super().__init__(Xi, T, M, N, D, Mm, layers, mode, activation, correlation_type, device=device)

    def _default_strike(self):
        return 1.0

    def _native_layers(self, layers):
        return [1 + 2 * self.n_assets] + layers[1:]

    def _make_model(self, layers):
        return networks.make_heston_model(self.mode, layers, self.activation, 1 + 2 * self.n_assets)

    def _full_state(self, Xi):
        """[S_1..S_k, ...] -> [S_1..S_k, v0..v0]: the reference always starts the
        variance at self.v0 and reads only the S column(s) of Xi
        (heston_dnnpde.py:619-623; predict may append v0, :668-670, which
        loss_function then ignores)."""
        k = self.n_assets
        x = torch.as_tensor(np.asarray(Xi) if not isinstance(Xi, torch.Tensor) else Xi,
                            dtype=torch.float32).to(self.device)
        x = x.reshape(-1, x.shape[-1]) if x.dim() > 1 else x.reshape(1, -1)
        if x.shape[1] < k:
            raise ValueError(f"Xi has {x.shape[1]} columns; the {k} asset prices come first")
        S = x[:, :k]
        return torch.cat([S, torch.full_like(S, self.v0)], 1).contiguous()

    def _initial_state(self, Xi):
        return self._full_state(Xi)

    def problem_spec(self):
        smooth = self.payoff_type == "continuous"
        if self.option_type == "put":
            g = "smooth_put" if smooth else "put_mean"
        else:
            g = "smooth_call" if smooth else "call_mean"
        return ProblemSpec(kind="heston", mu_a=0.05, phi_r=0.05, phi_c=0.0, g=g,
                           strike=self.strike, g_alpha=10.0, g_cols=self.n_assets, u_clamp=True, q3=False,
                           kappa=self.kappa, theta=self.theta, sigma=self.sigma, rho=self.rho)

    def g_tf(self, X):
        S = X[:, :self.n_assets] if X.dim() > 1 else X
        a = torch.mean(S, dim=1, keepdim=True) - self.strike if S.dim() > 1 else S - self.strike
        if self.option_type == "put":
            a = -a
        if self.payoff_type == "discontinuous":
            return torch.maximum(a, torch.tensor(0.0, device=X.device))
        return a / (1 + torch.exp(-10.0 * a))

    def phi_tf(self, t, X, Y, Z):
        return 0.05 * Y

    def mu_tf(self, t, X, Y=None, Z=None):
        k = self.n_assets
        S, v = X[:, :k], X[:, k:]
        return torch.cat([0.05 * S, self.kappa * (self.theta - v)], dim=1).clamp(-100, 100)

    def _record_y0(self, out):
        y0 = float(out["Y"][0, 0, 0])
        self.Y0_values.append(y0)

    def _train_graph(self):
        return np.column_stack((self.iteration, self.training_loss, self.Y0_values))

    def train(self, N_Iter, learning_rate, optimizer_type='Adam'):
        """heston_dnnpde.py:345-450 -> graph [iteration, training_loss, Y0]."""
        graph, _, _ = super().train(N_Iter, learning_rate, optimizer_type)
        return graph

    def predict(self, Xi_star, t_star, W_star):
        """heston_dnnpde.py:661-683 -> (S, v, Y)."""
        X, Y = super().predict(self._full_state(Xi_star), t_star, W_star)
        k = self.n_assets
        return X[:, :, :k], X[:, :, k:], Y

    def calculate_greeks(self, S, v, t):
        """heston_dnnpde.py:685-699 -> numpy (Y [R, 1], delta [R, k], gamma).

        S and v hold the R evaluation points ([R] at k = 1, as the reference
        passes them, or [R, k]); t the R times.  delta = dU/dS is net_u's Du
        over the S columns, and gamma = autograd.grad(delta, S, ones_like(delta))
        in the reference's expression order, so gamma has S's shape.  At k = 1
        that is d2U/dS2.  For k > 1 the all-ones cotangent sums the Hessian
        block over assets: gamma[r, i] = sum_j d2U / dS_i dS_j at point r (the
        row sums of the S-S Hessian block, not its diagonal).  Through the
        u clamp: Y, delta and gamma are 0 where the network output is negative.
        The Hessian-vector product is one native dbsde_net_u_xvjp."""
        k = self.n_assets
        S = torch.tensor(np.asarray(S), dtype=torch.float32, device=self.device, requires_grad=True)
        v = torch.tensor(np.asarray(v), dtype=torch.float32, device=self.device, requires_grad=True)
        t = torch.tensor(np.asarray(t), dtype=torch.float32, device=self.device)
        with torch.enable_grad():
            X = torch.cat([S.reshape(-1, k), v.reshape(-1, k)], dim=1)
            Y, Du = self.net_u(t.reshape(-1), X)
            delta = Du[:, :k]
            gamma = torch.autograd.grad(delta, S, grad_outputs=torch.ones_like(delta))[0]
        return Y.detach().cpu().numpy(), delta.detach().cpu().numpy(), gamma.detach().cpu().numpy()

    def _mc_state(self, X):
        """mc_value's points: [S_1..S_k] rows get v0 appended, as predict
        starts the variance; [S.., v..] rows (2k columns) are taken as given."""
        k = self.n_assets
        x = torch.as_tensor(np.asarray(X) if not isinstance(X, torch.Tensor) else X,
                            dtype=torch.float32).to(self.device)
        if x.dim() == 2 and x.shape[1] == 2 * k:
            return x.contiguous()
        return self._full_state(x.reshape(-1, k))

    def mc_greeks(self, S, v, t, mc=2 ** 16, n_steps=None, seed=0, h=0.01):
        """Monte-Carlo (price, delta, gamma) at the points of calculate_greeks,
        with its shapes: numpy ([R, 1], [R, k], [R, k]).  Delta and gamma are the
        central differences in S of mc_value at S - h, S, S + h, all three
        evaluated in ONE call and therefore on the same draws, so the differences
        are deterministic -- the bump-and-reprice of the reference's
        delta_surface / gamma_surface (numerics/heston_closed_form_ii.py:46-83)
        on this problem's own process.  For k > 1 all S columns are bumped
        together, matching calculate_greeks' all-ones cotangent: delta is the
        directional derivative along (1, .., 1) and gamma its second difference,
        each repeated over the k columns.  No u clamp is applied (the expectation
        of a non-negative payoff needs none).  As mc_value, a correlated object
        bumps and reprices on its correlated process."""
        k = self.n_assets
        S = torch.as_tensor(np.asarray(S), dtype=torch.float32).to(self.device).reshape(-1, k)
        v = torch.as_tensor(np.asarray(v), dtype=torch.float32).to(self.device).reshape(-1, k)
        t = torch.as_tensor(np.asarray(t), dtype=torch.float32).to(self.device).reshape(-1)
        R = S.shape[0]
        X = torch.cat([torch.cat([S + b, v], dim=1) for b in (-float(h), 0.0, float(h))], dim=0)
        val, _, _ = self.mc_value(t.repeat(3), X, mc=mc, n_steps=n_steps, seed=seed)
        dn, mid, up = (val[i * R:(i + 1) * R].double() for i in range(3))
        delta = ((up - dn) / (2.0 * h)).float().repeat(1, k)
        gamma = ((up - 2.0 * mid + dn) / (h * h)).float().repeat(1, k)
        return mid.float().cpu().numpy(), delta.cpu().numpy(), gamma.cpu().numpy()


class HestonTwoFactorFBSNN(HestonFBSNN):
    """The two-factor (textbook) Heston model on HestonFBSNN's surface.

    HestonFBSNN follows the reference, whose FBSNN dimension is 1: one scalar
    Brownian motion per asset drives both S_i and v_i, a degenerate one-factor
    diffusion.  Here each asset has two Brownian motions W^S_i and W^v_i with
    correlation rho between them (problem kind "heston2", include/dbsde.h
    DBSDE_PROB_HESTON2), so the network solves

      u_t + r S u_S + kappa (theta - v) u_v + 1/2 v S^2 u_SS + rho sigma v S u_Sv
          + 1/2 sigma^2 v u_vv - r u = 0,   u(T, .) = g,   r = 0.05,

    per asset.  State, network, payoffs, u clamp, NaN skip, predict,
    calculate_greeks, mc_value and mc_greeks are HestonFBSNN's; the Brownian
    dimension is 2k: column i of W is W^S_i, column k + i is W^v_i, all
    independent (fetch_minibatch draws 2k columns).  Limits: no correlation
    between assets (any correlation_type but "no_correlation" raises
    ValueError), no pathwise Monte-Carlo delta (mc_greeks bumps and reprices),
    and closed_form -- the characteristic-function price of the call or, with
    option_type="put", the put -- for one asset and the 'discontinuous' payoff
    only."""

    def __init__(self, Xi, T, M, N, D, Mm, layers, mode, activation, correlation_type="no_correlation", **kw):
        if correlation_type != "no_correlation":
            raise ValueError("HestonTwoFactorFBSNN has no correlation between assets: correlation_type must be "
                             "'no_correlation' (rho correlates each asset's own two Brownian motions)")
        if not abs(kw.get("rho", 0.8)) <= 1.0:
            raise ValueError("rho must lie in [-1, 1]")
        super().__init__(Xi, T, M, N, D, Mm, layers, mode, activation, correlation_type, **kw)

    def problem_spec(self):
        return dataclasses.replace(super().problem_spec(), kind="heston2")

    def sigma_tf(self, t, X, Y=None):
        """The diffusion matrix [R, 2k, 2k] of the kind-2 step: column i (dW^S_i)
        holds (S_i: sv S, v_i: rho sigma sv), column k + i (dW^v_i) holds
        (v_i: sqrt(1 - rho^2) sigma sv), sv = sqrt(max(v, 1e-8)), every entry
        clamped to [-100, 100]."""
        k = self.n_assets
        S, v = X[:, :k], X[:, k:]
        sv = torch.sqrt(torch.clamp(v, min=1e-8))
        sigV = self.sigma * sv
        A = torch.zeros((X.shape[0], 2 * k, 2 * k), dtype=X.dtype, device=X.device)
        i = torch.arange(k, device=X.device)
        A[:, i, i] = (sv * S).clamp(-100, 100)
        A[:, k + i, i] = (self.rho * sigV).clamp(-100, 100)
        A[:, k + i, k + i] = (math.sqrt(1.0 - self.rho ** 2) * sigV).clamp(-100, 100)
        return A

    def closed_form(self, S, v, t):
        """The Heston characteristic-function price of this object's problem at
        the points (S [R], v [R], t [R]): (price [R, 1], delta [R, 1] = dprice/dS)
        as float32 tensors on the device, through exact("heston", ...)
        (DBSDE_EXACT_HESTON) -- exact("heston_put", ...) for option_type "put"
        -- with r = 0.05 and this object's strike, kappa, theta, sigma and rho.
        One asset and the unsmoothed payoff ('discontinuous') only: anything
        else raises ValueError."""
        if self.n_assets != 1:
            raise ValueError("closed_form exists for one asset only (k = 1)")
        if self.payoff_type != "discontinuous":
            raise ValueError("closed_form prices the call payoff ('discontinuous') only")
        S = torch.as_tensor(np.asarray(S), dtype=torch.float32).to(self.device).reshape(-1)
        v = torch.as_tensor(np.asarray(v), dtype=torch.float32).to(self.device).reshape(-1)
        t = torch.as_tensor(np.asarray(t), dtype=torch.float32).to(self.device).reshape(-1)
        if not (S.numel() == v.numel() == t.numel()):
            raise ValueError("S, v and t must hold the same number of points")
        kind = "heston_put" if self.option_type == "put" else "heston"
        return _exact(kind, t, torch.stack([S, v], dim=1).contiguous(), self.T,
                      (0.05, self.strike, self.kappa, self.theta, self.sigma, self.rho))


class _AsianState:
    """The arithmetic-average (Asian) option on D assets (no reference
    counterpart; problem kind DBSDE_PROB_ASIAN, ProblemSpec(average=True)).

    The running average is carried as one more state coordinate: the state is
    [A, S_1..S_D] (state_dim = D + 1), every S_i follows the basket dynamics
    dS = 0.05 S dt + 0.20 S dW_i, A' = A + mean_i S_i dt / T (the left-point
    rule, A_0 = 0), and u(t, A, S) solves

      u_t + (mean S / T) u_A + sum_i 0.05 S_i u_{S_i} + 1/2 tr(sigma sigma^T D^2_S u) - 0.05 u = 0,
      u(T, .) = g(A),

    g the call max(A - K, 0) or put max(K - A, 0) on the average, or with
    payoff_type='continuous' their sigmoid-smoothed forms (alpha = 10).  The
    Brownian dimension is D (fetch_minibatch draws D columns; correlation_type
    correlates the D assets), the network takes (t, A, S) -- D + 2 inputs:
    `layers[0]` is replaced by D + 2 -- and Xi holds the D asset prices (A = 0
    is prepended; rows of D + 1 columns are taken as [A, S] as given).  predict
    returns X [M, N+1, D + 1] with A in column 0; net_u, theta, pde_residual and
    mc_value take points [A, S_1..S_D] (mc_value also [S_1..S_D] with A = 0).
    Limits: the average is arithmetic with a fixed strike (no floating-strike
    average; the geometric average is the Geometric* classes), it has no closed
    form (the geometric price is its lower bound), the assets are diagonal
    processes (no average over Heston states), and a subclass overriding a
    coefficient method with other coefficients is refused (NotImplementedError)
    instead of running on the generic path."""

    option_type = "call"

    def __init__(self, Xi, T, M, N, D, Mm, layers, mode, activation, correlation_type="no_correlation",
                 payoff_type='discontinuous', device=None):
        if payoff_type not in ("discontinuous", "continuous"):
            raise ValueError("Invalid payoff type. Choose 'discontinuous' or 'continuous'.")
        self.payoff_type = payoff_type
        self.n_assets = D
        super().__init__(Xi, T, M, N, D, Mm, layers, mode, activation, correlation_type, device=device)

    def _default_strike(self):
        return 1.0

    def _native_layers(self, layers):
        return [2 + self.n_assets] + layers[1:]

    def _make_model(self, layers):
        return networks.make_model(self.mode, [2 + self.n_assets] + list(layers[1:]), self.activation)

    def _full_state(self, Xi):
        """[S_1..S_D] -> [0, S_1..S_D]; rows of D + 1 columns are [A, S] already."""
        k = self.n_assets
        x = torch.as_tensor(np.asarray(Xi) if not isinstance(Xi, torch.Tensor) else Xi,
                            dtype=torch.float32).to(self.device)
        x = x.reshape(-1, x.shape[-1]) if x.dim() > 1 else x.reshape(1, -1)
        if x.shape[1] == k + 1:
            return x.contiguous()
        if x.shape[1] != k:
            raise ValueError(f"Xi has {x.shape[1]} columns; expected the {k} asset prices (or [A, S]: {k + 1})")
        return torch.cat([torch.zeros_like(x[:, :1]), x], 1).contiguous()

    def _initial_state(self, Xi):
        return self._full_state(Xi)

    def _mc_state(self, X):
        return self._full_state(X)

    def problem_spec(self):
        smooth = self.payoff_type == "continuous"
        if self.option_type == "put":
            g = "smooth_put" if smooth else "put_mean"
        else:
            g = "smooth_call" if smooth else "call_mean"
        return ProblemSpec(mu_a=0.05, sig_a=0.20, phi_r=0.05, phi_c=0.0, g=g, strike=self.strike, g_alpha=10.0,
                           g_cols=1, q3=False, average=True)

    def phi_tf(self, t, X, Y, Z):
        return 0.05 * (Y)

    def g_tf(self, X):
        a = X[:, :1] - self.strike
        if self.option_type == "put":
            a = -a
        if self.payoff_type == "discontinuous":
            return torch.maximum(a, torch.tensor(0.0, device=X.device))
        return a / (1 + torch.exp(-10.0 * a))

    def mu_tf(self, t, X, Y=None, Z=None):
        S = X[:, 1:]
        return torch.cat([torch.mean(S, dim=1, keepdim=True) / self.T, 0.05 * S], dim=1)

    def sigma_tf(self, t, X, Y=None):
        """[R, D + 1, D]: a zero A row over 0.20 diag(S)."""
        A = 0.20 * torch.diag_embed(X[:, 1:])
        return torch.cat([torch.zeros_like(A[:, :1, :]), A], dim=1)

    def predict(self, Xi_star, t_star, W_star):
        """-> (X [M, N+1, D + 1] with A in column 0, Y)."""
        return super().predict(self._full_state(Xi_star), t_star, W_star)


class AsianCallOption(_AsianState, FBSNN):
    """The arithmetic-average call max(A_T - K, 0), K = 1 by default, on
    CallOption's surface (its train(), schedule and gradient clipping)."""


class AsianPutOption(AsianCallOption):
    """AsianCallOption's problem with the put payoff max(K - A_T, 0)."""

    option_type = "put"


class AsianBasketCallOption(_AsianState, _WithCorrTrain, FBSNN):
    """The arithmetic-average call on a basket, on BasketCallOption's surface:
    its train() (the N**(1/5) schedule, time_logs) and correlated increments."""


class AsianBasketPutOption(AsianBasketCallOption):
    """AsianBasketCallOption's problem with the put payoff max(K - A_T, 0)."""

    option_type = "put"


class _GeoAsianState(_AsianState):
    """The geometric-average Asian option on D assets (no reference counterpart;
    problem kind DBSDE_PROB_GEO_ASIAN, ProblemSpec(average="geometric")).

    _AsianState's surface with the state [G, S_1..S_D], G the running geometric
    average exp((1/T) int_0^t mean_i log S_i ds): G_0 = 1 (prepended to Xi; rows
    of D + 1 columns are [G, S] as given), dG = G (mean_i log S_i / T) dt, every
    S_i the GBM dS = 0.05 S dt + 0.20 S dW_i, and u(t, G, S) solves

      u_t + G (mean log S / T) u_G + sum_i 0.05 S_i u_{S_i} + 1/2 tr(sigma sigma^T D^2_S u) - 0.05 u = 0,
      u(T, .) = g(G).

    G_T is log-normal, so the unsmoothed option has a closed form at any D and
    with a Cholesky factor between the assets: closed_form().  It is the
    continuous-time value; the training grid's scheme (the left-point rule on
    log S) differs from it by O(dt).  Limits: fixed strike, sig_b = 0 (GBM
    assets), no Heston states; mc_value with a factor keeps D <= 128."""

    def _full_state(self, Xi):
        """[S_1..S_D] -> [1, S_1..S_D]; rows of D + 1 columns are [G, S] already.
        Values held on the host are checked: G and every S must be positive."""
        k = self.n_assets
        host = not (isinstance(Xi, torch.Tensor) and Xi.device.type != "cpu")
        x = torch.as_tensor(np.asarray(Xi) if not isinstance(Xi, torch.Tensor) else Xi, dtype=torch.float32)
        x = x.reshape(-1, x.shape[-1]) if x.dim() > 1 else x.reshape(1, -1)
        if host and not bool((x > 0).all()):
            raise ValueError("the geometric average needs G > 0 and every S_i > 0")
        x = x.to(self.device)
        if x.shape[1] == k + 1:
            return x.contiguous()
        if x.shape[1] != k:
            raise ValueError(f"Xi has {x.shape[1]} columns; expected the {k} asset prices (or [G, S]: {k + 1})")
        return torch.cat([torch.ones_like(x[:, :1]), x], 1).contiguous()

    def problem_spec(self):
        return dataclasses.replace(super().problem_spec(), average="geometric")

    def mu_tf(self, t, X, Y=None, Z=None):
        S = X[:, 1:]
        return torch.cat([X[:, :1] * torch.mean(torch.log(S), dim=1, keepdim=True) / self.T, 0.05 * S], dim=1)

    def closed_form(self, G, S, t):
        """The continuous-time price of this object's option at the points
        (G [R], S [R, D], t [R]): (price [R, 1], delta [R, D + 1] = [d/dG,
        d/dS_1..d/dS_D]) as float32 tensors on the device, through
        exact("geo_asian", ...) -- "geo_asian_put" for option_type "put" -- with
        mu = r = 0.05, sigma = 0.20, this object's strike and T, and cbar, vbar
        of this object's own Cholesky factor.  The unsmoothed payoff
        ('discontinuous') only."""
        if self.payoff_type != "discontinuous":
            raise ValueError("closed_form prices the unsmoothed payoff ('discontinuous') only")
        k = self.n_assets
        G = torch.as_tensor(np.asarray(G) if not isinstance(G, torch.Tensor) else G, dtype=torch.float32).reshape(-1, 1)
        S = torch.as_tensor(np.asarray(S) if not isinstance(S, torch.Tensor) else S, dtype=torch.float32).reshape(-1, k)
        t = torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t, dtype=torch.float32).reshape(-1)
        if not (G.shape[0] == S.shape[0] == t.numel()):
            raise ValueError("G, S and t must hold the same number of points")
        X = self._full_state(torch.cat([G.to(S.device), S], dim=1))
        L = np.eye(k) if self._L is None else np.tril(np.asarray(self._L, dtype=np.float64))
        C = L @ L.T
        cbar, vbar = float(np.trace(C)) / k, float(C.sum()) / (k * k)
        kind = "geo_asian_put" if self.option_type == "put" else "geo_asian"
        return _exact(kind, t.to(self.device), X, self.T, (0.05, 0.05, 0.20, self.strike, cbar, vbar))


class GeometricAsianCallOption(_GeoAsianState, FBSNN):
    """The geometric-average call max(G_T - K, 0), K = 1 by default, on
    CallOption's surface (its train(), schedule and gradient clipping)."""


class GeometricAsianPutOption(GeometricAsianCallOption):
    """GeometricAsianCallOption's problem with the put payoff max(K - G_T, 0)."""

    option_type = "put"


class GeometricAsianBasketCallOption(_GeoAsianState, _WithCorrTrain, FBSNN):
    """The geometric-average call on a basket, on BasketCallOption's surface:
    its train() (the N**(1/5) schedule, time_logs) and correlated increments."""


class GeometricAsianBasketPutOption(GeometricAsianBasketCallOption):
    """GeometricAsianBasketCallOption's problem with the put payoff max(K - G_T, 0)."""

    option_type = "put"


class _AmericanPut:
    """Early exercise by penalisation (dbsde_problem.pen): the
    parent's put with the driver

      phi = phi_parent - penalty max(g(X) - Y, 0),

    g the parent's payoff on the row's own X, i.e. the semilinear PDE
    u_t + L u - phi_lin + penalty (g - u)^+ = 0, u(T, .) = g, whose solution
    rises to the American value as penalty grows (at penalty = 100, the
    default, about 2 % of the early-exercise premium is missing at the money,
    K = 1, r = 0.05, sigma = 0.2, T = 1).  problem_spec() carries the penalty,
    so the problem runs in the kernels; a subclass that changes phi_tf runs its
    own methods (generic.py) like any other.  Not linear: mc_value raises;
    the arbiter is tree_value (one asset).  european() is the same problem
    without the penalty, whose mc_value and closed_form bound it from below."""

    def __init__(self, *args, penalty=100.0, **kw):
        penalty = float(penalty)
        if not (penalty >= 0.0 and math.isfinite(penalty)):
            raise ValueError("penalty must be finite and >= 0")
        self.penalty = penalty
        self._ctor = (args, dict(kw))
        super().__init__(*args, **kw)

    def problem_spec(self):
        return dataclasses.replace(super().problem_spec(), penalty=self.penalty)

    def phi_tf(self, t, X, Y, Z):
        return super().phi_tf(t, X, Y, Z) - self.penalty * torch.relu(self.g_tf(X) - Y)

    def european(self):
        """The same problem with penalty = 0: a new object built from this one's
        constructor arguments, with its own (freshly initialised) network and
        this object's correlation -- correlation_matrix, the Cholesky factor _L
        and the native context's copy are taken from self, not drawn again, so
        its mc_value prices the same correlated basket.  The caller's numpy and
        torch (CPU) random streams are left where they were."""
        args, kw = self._ctor
        np_state, torch_state = np.random.get_state(), torch.get_rng_state()
        try:
            twin = type(self)(*args, penalty=0.0, **kw)
        finally:
            np.random.set_state(np_state)
            torch.set_rng_state(torch_state)
        twin.correlation_matrix = np.array(self.correlation_matrix, copy=True)
        twin._L = None if self._L is None else np.array(self._L, copy=True)
        if twin._L is not None:
            twin.solver.set_corr(twin._L)
        return twin

    def _one_asset(self, what):
        if self.D != 1:
            raise ValueError(f"{what} prices one asset (D = 1); this object has D = {self.D}")
        spec = self.problem_spec()
        # r, sigma, K and the risk-neutral drift b of the simulated asset
        return spec.phi_r, spec.sig_a, float(self.strike), spec.mu_a + spec.phi_r * spec.phi_c

    def _tx(self, t, X):
        X = torch.as_tensor(np.asarray(X) if not isinstance(X, torch.Tensor) else X,
                            dtype=torch.float32).to(self.device).reshape(-1, 1).contiguous()
        t = torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t,
                            dtype=torch.float32).to(self.device).reshape(-1).contiguous()
        if t.numel() != X.shape[0]:
            raise ValueError("t and X must hold the same number of points")
        return t, X

    def tree_value(self, t, X, n_tree=2000, penalised=False):
        """(price [R, 1], delta [R, 1]) of this object's put with early exercise
        at the points (t [R], X [R, 1]) on a binomial tree of n_tree steps
        (exact("american_put"), DBSDE_EXACT_AMERICAN_PUT) with the object's r,
        sigma, strike and drift b = mu_a + phi_r phi_c.  penalised=False: the
        American value; True: the value of the penalised problem the network
        trains on (this object's penalty).  One asset only."""
        r, sigma, K, b = self._one_asset("tree_value")
        t, X = self._tx(t, X)
        return _exact("american_put", t, X, self.T, r, sigma, K, b=b, n_tree=n_tree,
                      penalty=self.penalty if penalised else math.inf)

    def closed_form(self, t, X):
        """The European put's Black-Scholes value with cost of carry b at the
        points: (price [R, 1], delta [R, 1]), evaluated in float64 and returned
        as float32 tensors on the device.  It is the solution of the penalty = 0
        problem only: an object with penalty > 0 raises ValueError (its problem
        has no closed form; european().closed_form is its lower bound and
        tree_value its arbiter).  One asset only."""
        if self.penalty != 0.0:
            raise ValueError(f"{type(self).__name__} with penalty > 0 has no closed form: european().closed_form "
                             "is the European lower bound, tree_value the American value")
        r, sigma, K, b = self._one_asset("closed_form")
        t, X = self._tx(t, X)
        S, tau = X[:, 0].double(), self.T - t.double()
        live = tau > 0
        tl = torch.where(live, tau, torch.ones_like(tau))
        st = sigma * torch.sqrt(tl)
        d1 = (torch.log(S / K) + (b + 0.5 * sigma * sigma) * tl) / st
        N = lambda v: 0.5 * torch.erfc(-v / math.sqrt(2.0))
        carry = torch.exp((b - r) * tl)
        price = K * torch.exp(-r * tl) * N(-(d1 - st)) - S * carry * N(-d1)
        delta = -carry * N(-d1)
        pay = torch.clamp(K - S, min=0.0)
        dpay = torch.where(S < K, -torch.ones_like(S), torch.where(S == K, -0.5 * torch.ones_like(S), torch.zeros_like(S)))
        price, delta = torch.where(live, price, pay), torch.where(live, delta, dpay)
        return price.float().reshape(-1, 1), delta.float().reshape(-1, 1)


class AmericanPutOption(_AmericanPut, PutOption):
    """PutOption (payoff max(K - sum X, 0), phi = r (Y - X.Z)) with early exercise
    by penalisation, on PutOption's surface; keyword penalty=100.0."""


class AmericanBasketPutOption(_AmericanPut, BasketPutOption):
    """BasketPutOption (payoff max(K - mean X, 0), correlated increments, its
    schedule and train surface) with early exercise by penalisation; keyword
    penalty=100.0.  No multi-asset arbiter: tree_value needs D = 1."""


class _KnockOut:
    """A knock-out barrier on the parent's option (problem kind
    DBSDE_PROB_BARRIER, ProblemSpec(barrier=B)): keyword barrier=B > 0.  The
    calls are down-and-out (B <= strike), the puts up-and-out (B >= strike);
    the monitored statistic is the payoff's own (the sum of the assets for
    CallOption / PutOption, their mean for the baskets), checked at the grid
    times t_0..t_N, no rebate.  Training runs on the stopped paths X_{t ^ tau}
    (rows behind the knock-out row hold its state, their sigma dW is 0), on
    which the BSDE loss itself teaches u = 0 beyond the barrier; predict and
    loss_function return the stopped X.  fetch_minibatch still returns the
    unstopped Brownian path: the stop pass follows every rollout.

    european() is the twin without the barrier (an upper bound), closed_form
    the Reiner-Rubinstein price for one asset, mc_value the knocked-out
    Monte-Carlo value on the training scheme (D <= 128; delta=True raises: bump
    and reprice on the same draws).  Limits: no knock-in, rebate, reverse or
    double barrier, no bridge correction between grid times, no barrier on
    Heston, Asian or American problems; pde_residual is meaningful on the live
    side only; a subclass overriding a coefficient method with other
    coefficients is refused (NotImplementedError): the generic rollout does not
    stop paths.  barrier=0 builds the parent's problem (european() does)."""

    def __init__(self, *args, barrier, **kw):
        barrier = float(barrier)
        if not (barrier >= 0.0 and math.isfinite(barrier)):
            raise ValueError("barrier must be finite and > 0 (0: no barrier)")
        self.barrier = barrier
        self._ctor = (args, dict(kw))
        super().__init__(*args, **kw)

    def problem_spec(self):
        spec = super().problem_spec()
        return dataclasses.replace(spec, barrier=self.barrier, q3=False) if self.barrier else spec

    def european(self):
        """The same option without the barrier: a new object built from this
        one's constructor arguments with barrier=0, its own (freshly initialised)
        network and this object's correlation, as _AmericanPut.european builds
        its twin.  Its value bounds the knock-out value from above, path by path
        on the same draws.  The caller's numpy and torch (CPU) random streams are
        left where they were."""
        args, kw = self._ctor
        np_state, torch_state = np.random.get_state(), torch.get_rng_state()
        try:
            twin = type(self)(*args, barrier=0.0, **kw)
        finally:
            np.random.set_state(np_state)
            torch.set_rng_state(torch_state)
        twin.correlation_matrix = np.array(self.correlation_matrix, copy=True)
        twin._L = None if self._L is None else np.array(self._L, copy=True)
        if twin._L is not None:
            twin.solver.set_corr(twin._L)
        return twin

    def closed_form(self, t, X, monitoring="discrete"):
        """(price [R, 1], delta [R, 1]) of this object's knock-out option at the
        points (t [R], X [R, 1]): the Reiner-Rubinstein formula
        (exact("barrier_call" / "barrier_put"), DBSDE_EXACT_BARRIER_*) with the
        object's r, sigma, strike, cost of carry b = mu_a + phi_r phi_c and
        barrier.  monitoring="discrete": the barrier is first shifted by the
        Broadie-Glasserman-Kou factor for this object's grid -- n_mon = N (T - t)
        / T dates over the remaining time, i.e. a spacing of T / N at every point;
        "continuous": no shift.  One asset only."""
        if monitoring not in ("discrete", "continuous"):
            raise ValueError("monitoring must be 'discrete' or 'continuous'")
        if self.D != 1:
            raise ValueError(f"closed_form prices one asset (D = 1); this object has D = {self.D}")
        if not self.barrier:
            raise ValueError("closed_form is the knock-out price: this object has no barrier")
        spec = self.problem_spec()
        r, sigma, K, b = spec.phi_r, spec.sig_a, float(self.strike), spec.mu_a + spec.phi_r * spec.phi_c
        X = torch.as_tensor(np.asarray(X) if not isinstance(X, torch.Tensor) else X,
                            dtype=torch.float32).to(self.device).reshape(-1, 1).contiguous()
        t = torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t,
                            dtype=torch.float32).to(self.device).reshape(-1).contiguous()
        if t.numel() != X.shape[0]:
            raise ValueError("t and X must hold the same number of points")
        kind = "barrier_put" if spec.g.startswith("put") else "barrier_call"
        price, delta = torch.empty_like(X), torch.empty_like(X)
        for tv in torch.unique(t).tolist():   # n_mon is one parameter of a call: one call per time
            sel = t == tv
            tau = float(self.T) - tv
            n_mon = self.N * tau / float(self.T) if (monitoring == "discrete" and tau > 0) else 0.0
            pr, dl = _exact(kind, t[sel], X[sel], self.T, (r, sigma, K, b, self.barrier, n_mon))
            price[sel], delta[sel] = pr, dl
        return price, delta


class BarrierCallOption(_KnockOut, CallOption):
    """CallOption (payoff max(sum X - K, 0), phi = r (Y - X.Z)) knocked out when
    sum X <= barrier at a grid time; keyword barrier= (<= strike)."""


class BarrierPutOption(_KnockOut, PutOption):
    """PutOption (payoff max(K - sum X, 0)) knocked out when sum X >= barrier at a
    grid time; keyword barrier= (>= strike)."""


class BarrierBasketCallOption(_KnockOut, BasketCallOption):
    """BasketCallOption (payoff max(mean X - K, 0), correlated increments, its
    schedule and train surface) knocked out when mean X <= barrier at a grid time;
    keyword barrier= (<= strike)."""


class BarrierBasketPutOption(_KnockOut, BasketPutOption):
    """BasketPutOption (payoff max(K - mean X, 0)) knocked out when mean X >=
    barrier at a grid time; keyword barrier= (>= strike)."""


__all__ = ["CallOption", "PutOption", "CallOption1D", "BasketCallOption", "BasketPutOption", "BSPDETestCase", "HamiltonJacobiBellman",
           "HestonFBSNN", "HestonTwoFactorFBSNN", "AsianCallOption", "AsianPutOption", "AsianBasketCallOption",
           "AsianBasketPutOption", "GeometricAsianCallOption", "GeometricAsianPutOption",
           "GeometricAsianBasketCallOption", "GeometricAsianBasketPutOption", "AmericanPutOption",
           "AmericanBasketPutOption", "BarrierCallOption", "BarrierPutOption", "BarrierBasketCallOption",
           "BarrierBasketPutOption"]
