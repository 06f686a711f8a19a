"""The two-factor Heston problem without a GPU: the restatements the GPU tests
compare against (tests/heston2_reference.py) are held to fp64 references of
their own, and the Python class selects the native coefficients.

  * the closed form on the kernel's quadrature nodes against the converged
    integral over the domain include/dbsde.h states (2e-7, a tenth of the
    fp32 ATOL of tests/test_gpu_mc.py);
  * its sigma -> 0 limit (Black-Scholes at volatility sqrt(theta)) and the PDE
    it solves, so the formula itself is pinned, not only its quadrature;
  * the fp32 chain against the fp64 loss oracle's paths, and the chosen
    Monte-Carlo seed against the ambiguity cap of the GPU comparison;
  * HestonTwoFactorFBSNN: native coefficients, consistent sigma_tf / mu_tf, the
    refusal of a correlation type."""
import numpy as np
import pytest
import torch

import heston2_reference as h2
from conftest import load_pkg
from oracle import philox as ph


# ------------------------------------------------------------------ closed form
def test_kernel_nodes_agree_with_the_converged_integral():
    worst = 0.0
    for rho, tau, v, m in h2.domain_grid():
        p, d = h2.closed_form(m, v, tau, rho=rho)
        q, dq = h2.closed_form_quad(m, v, tau, rho=rho)
        worst = max(worst, abs(float(p) - q), abs(float(d) - dq))
        assert abs(float(p) - q) <= 2e-7 and abs(float(d) - dq) <= 2e-7, (rho, tau, v, m, float(p), q)
    print(f"max |kernel nodes - converged| over {len(h2.domain_grid())} points: {worst:.3e} (bound 2e-7)")


def test_eight_times_the_panels_changes_nothing():
    """The same rule with 8 x the panels (the stand-in for a converged
    integration where scipy is missing) agrees to the same 2e-7."""
    for rho, tau, v, m in h2.domain_grid()[::7]:
        p, d = h2.closed_form(m, v, tau, rho=rho)
        q, dq = h2.closed_form(m, v, tau, rho=rho, panels=8 * h2.PANELS)
        assert abs(float(p - q)) <= 2e-7 and abs(float(d - dq)) <= 2e-7


def test_maturity_and_bounds():
    p, d = h2.closed_form([1.5, 1.0, 0.5], 0.2, [0.0, 0.0, -0.1])
    np.testing.assert_array_equal(p, [0.5, 0.0, 0.0])
    np.testing.assert_array_equal(d, [1.0, 0.5, 0.0])
    for S in (0.5, 1.0, 2.0):                       # no-arbitrage bounds and a delta in (0, 1)
        p, d = h2.closed_form(S, 0.2, 1.0)
        assert max(S - np.exp(-0.05), 0.0) < float(p) < S and 0.0 < float(d) < 1.0


def test_small_vol_of_vol_limit_is_black_scholes():
    """v = theta keeps the variance at theta when sigma = 0, so the price tends
    to Black-Scholes at volatility sqrt(theta).  The expansion in the vol of
    vol (Lewis 2000, ch. 3) starts at first order, price = BS + sigma rho c1 +
    O(sigma^2) with c1 a vega-type term of order tau theta, so halving sigma
    must at least cut the difference by 1.5 (2 in the limit), and a tenth of
    sigma by 5 (10 in the limit)."""
    theta, tau, S = 0.2, 1.0, 1.1
    bs, bd = h2.bs_call(S, 1.0, tau, 0.05, np.sqrt(theta))
    errs = []
    for sigma in (0.04, 0.02, 0.01, 1e-3):
        p, d = h2.closed_form(S, theta, tau, sigma=sigma, theta=theta, rho=-0.7)
        errs.append((abs(float(p) - bs), abs(float(d) - bd)))
    print("sigma -> 0:", errs)
    for (e0, f0), (e1, f1) in zip(errs[:2], errs[1:3]):
        assert e1 < e0 / 1.5 and f1 < f0 / 1.5
    assert errs[3][0] < errs[2][0] / 5 and errs[3][1] < errs[2][1] / 5      # sigma / 10


def test_closed_form_solves_the_pde():
    """u_t + r S u_S + kappa (theta - v) u_v + 1/2 v S^2 u_SS + rho sigma v S u_Sv
    + 1/2 sigma^2 v u_vv - r u = 0 by central differences of the restatement in
    fp64, on one fixed node set per point (U of the centre: the quadrature error
    is then smooth and differences out).  Steps h = 1e-3 (S, v, t): the
    truncation error of each second difference is h^2 / 12 times a fourth
    derivative (below 50 at these points: 5e-6), the rounding error 4 eps |u| /
    h^2 = 1e-9; the residual stays below 2e-5 where its largest term is above
    1e-2."""
    r, h = 0.05, 1e-3
    for rho in (0.8, -0.7):
        c = dict(h2.HESTON, rho=rho)
        for S, v, tau in ((1.0, 0.2, 1.0), (0.9, 0.1, 0.5), (1.2, 0.4, 1.5)):
            U = h2.upper_limit(tau, v, np.log(S), r, c["kappa"], c["theta"], c["sigma"], rho)
            u = lambda s, w, ta: float(h2.closed_form(s, w, ta, U=U, **c)[0])
            u0 = u(S, v, tau)
            u_t = -(u(S, v, tau + h) - u(S, v, tau - h)) / (2 * h)             # t = T - tau
            u_S = (u(S + h, v, tau) - u(S - h, v, tau)) / (2 * h)
            u_v = (u(S, v + h, tau) - u(S, v - h, tau)) / (2 * h)
            u_SS = (u(S + h, v, tau) - 2 * u0 + u(S - h, v, tau)) / h ** 2
            u_vv = (u(S, v + h, tau) - 2 * u0 + u(S, v - h, tau)) / h ** 2
            u_Sv = (u(S + h, v + h, tau) - u(S + h, v - h, tau) - u(S - h, v + h, tau) + u(S - h, v - h, tau)) / (4 * h * h)
            terms = [u_t, r * S * u_S, c["kappa"] * (c["theta"] - v) * u_v, 0.5 * v * S * S * u_SS,
                     rho * c["sigma"] * v * S * u_Sv, 0.5 * c["sigma"] ** 2 * v * u_vv, -r * u0]
            res = sum(terms)
            print(f"rho={rho} (S, v, tau)=({S}, {v}, {tau}): residual {res:.3e}, largest term {max(map(abs, terms)):.3e}")
            assert max(map(abs, terms)) > 1e-2 and abs(res) < 2e-5
            # and delta is the S derivative of the price
            assert abs(float(h2.closed_form(S, v, tau, U=U, **c)[1]) - u_S) < 1e-5


# ------------------------------------------------------------------ the chain and the oracles
def test_chain_matches_the_fp64_oracle_paths():
    """The float32 chain and the float64 loss oracle step the same increments:
    their paths agree to float32 rounding (the bound the GPU test holds the
    device to), and rho couples v to dW^S."""
    k, M = 3, 7
    dw = ph.increments(5, 0, 0, M, h2.N, 2 * k, h2.T)
    X, sdw = h2.rollout(h2.xi_state(k), dw, h2.T, **h2.HESTON)
    _, model, _ = h2.loss_model(k)
    ref = h2.loss_and_grads(model, k, ph.time_grid(h2.N, h2.T), dw, h2.xi_state(k), **h2.HESTON)
    np.testing.assert_allclose(X, ref["X"], rtol=1e-5, atol=1e-6)
    assert np.isfinite(ref["loss"]) and np.abs(ref["grad"][ref["used"]]).max() > 0
    # first step by hand: S1 = S + 0.05 S dt + sqrt(v) S w1, v1 = v + kappa (theta - v) dt + sigma sqrt(v) (rho w1 + rhob w2)
    dt, sv = 1.0 / h2.N, np.sqrt(0.2)
    np.testing.assert_allclose(X[:, 1, :k], 1.0 + 0.05 * dt + sv * dw[:, 0, :k], rtol=1e-6)
    np.testing.assert_allclose(X[:, 1, k:], 0.2 + 0.3 * sv * (0.8 * dw[:, 0, :k] + 0.6 * dw[:, 0, k:]), rtol=1e-5, atol=1e-7)
    np.testing.assert_array_equal(sdw[:, 0, :k], (np.float32(sv) * np.float32(1.0)) * dw[:, 0, :k])


@pytest.mark.parametrize("case", list(h2.LOSS_CASES))
def test_loss_cases_are_well_conditioned(case):
    """The shapes and seeds of the GPU loss test, on the oracle's own draws: the
    float32 chain and the float64 oracle agree within a tenth of the X
    tolerance (no path sits on the sqrt(max(v, 1e-8)) kink), the variance does
    get close to the kink or below it somewhere at the larger k, and the network
    is not clamped away (Y and the gradient are not zero)."""
    k, M, width = h2.LOSS_CASES[case]
    dw = ph.increments(h2.LOSS_SEED + k, 0, 0, M, h2.N, 2 * k, h2.T)
    X, _ = h2.rollout(h2.xi_state(k), dw, h2.T, **h2.HESTON)
    _, model, _ = h2.loss_model(k, width)
    ref = h2.loss_and_grads(model, k, ph.time_grid(h2.N, h2.T), dw, h2.xi_state(k), **h2.HESTON)
    worst = float((np.abs(X - ref["X"]) / (1e-6 + 1e-5 * np.abs(ref["X"]))).max())
    print(f"{case}: X err / tol = {worst:.3f}, min v = {X[:, :, k:].min():.4f}, loss = {ref['loss']:.4f}, "
          f"max|Y| = {np.abs(ref['Y']).max():.3f}, max|grad| = {np.abs(ref['grad']).max():.3f}")
    assert worst < 0.1
    assert np.abs(ref["Y"]).max() > 0.01 and np.abs(ref["grad"][ref["used"]]).max() > 0.01
    assert (ref["Y"] > 0).mean() > 0.5


def test_pde_terms_are_the_textbook_operator():
    """The restated diffusion term equals 1/2 v S^2 u_SS + rho sigma v S u_Sv +
    1/2 sigma^2 v u_vv of the network by a direct Hessian (k = 1)."""
    import heston_corr_reference as hc
    oracle, _, t, X, clamped = hc.pde_setup(k=1, seed=7, R=12)
    terms = h2.pde_terms(oracle, t, X, 1, **h2.HESTON)
    model = __import__("copy").deepcopy(oracle).double()
    for r in np.flatnonzero(~clamped)[:4]:
        z = torch.tensor(np.concatenate([t[r], X[r]]).astype(np.float64))
        H = torch.autograd.functional.hessian(lambda q: model(q[None, :])[0, 0], z).numpy()[1:, 1:]
        S, v = float(X[r, 0]), float(X[r, 1])
        want = 0.5 * v * S * S * H[0, 0] + 0.8 * 0.3 * v * S * H[0, 1] + 0.5 * 0.09 * v * H[1, 1]
        np.testing.assert_allclose(terms["diffusion"][r, 0], want, rtol=1e-9, atol=1e-12)
    assert np.all(terms["u"][clamped] == 0) and np.all(terms["diffusion"][clamped] == 0)


@pytest.mark.parametrize("k", [1, 2])
def test_the_mc_seed_keeps_the_ambiguity_cap(k):
    """At most 4 samples per point of the call payoff lie within 2e-5 of the
    kink in the restatement (the GPU comparison asserts the same)."""
    pkg = load_pkg()
    ref = h2.mc_case(pkg, k, "call_mean")
    print("ambiguous", ref["ambiguous"], "value", ref["value"])
    assert ref["ambiguous"].max() <= 4
    assert np.all(np.isfinite(ref["value"])) and np.all(ref["stderr"][[0, 1, 2, 4]] > 0)


# ------------------------------------------------------------------ the class
def _bare(pkg, k, cls=None):
    m = object.__new__(cls or pkg.HestonTwoFactorFBSNN)      # no device here: _select_problem needs none
    m.kappa, m.theta, m.sigma, m.rho, m.v0 = 2.0, 0.2, 0.3, 0.8, 0.2
    m.payoff_type, m.n_assets, m.strike, m.T = "discontinuous", k, 1.0, 1.0
    m.layers = [1 + 2 * k, 16, 16, 16, 16, 1]
    m.device = torch.device("cpu")
    m.Xi = torch.tensor(h2.xi_state(k), dtype=torch.float32)
    return m


@pytest.mark.parametrize("k", [1, 3])
def test_class_runs_native_coefficients(k):
    pkg = load_pkg()
    m = _bare(pkg, k)
    spec = m._select_problem()
    assert m.native_coefficients and m.generic_reason is None
    assert spec.kind == "heston2" and spec.to_c().kind == 2 and spec.g_cols == k and spec.u_clamp
    assert _bare(pkg, k, pkg.HestonFBSNN)._select_problem().kind == "heston"       # the parent is unchanged
    X = torch.tensor(np.random.RandomState(1).uniform(0.05, 1.5, (5, 2 * k)))
    mu, A = h2.coefficients(X, k, **h2.HESTON)
    np.testing.assert_allclose(m.sigma_tf(None, X).numpy(), A.numpy(), rtol=1e-12)
    np.testing.assert_allclose(m.mu_tf(None, X).numpy(), mu.numpy(), rtol=1e-12)
    a = (A @ A.transpose(1, 2)).numpy()             # the covariance of the textbook model
    S, v = X[:, 0].numpy(), X[:, k].numpy()
    np.testing.assert_allclose(a[:, 0, 0], v * S * S, rtol=1e-12)
    np.testing.assert_allclose(a[:, 0, k], 0.8 * 0.3 * v * S, rtol=1e-12)
    np.testing.assert_allclose(a[:, k, k], 0.09 * v, rtol=1e-12)


def test_class_refuses_a_correlation_type_and_a_wide_closed_form():
    pkg = load_pkg()
    with pytest.raises(ValueError, match="no_correlation"):
        pkg.HestonTwoFactorFBSNN(np.ones((1, 2)), 1.0, 4, 4, 2, None, [3, 16, 16, 16, 16, 1], "Naisnet", "Sine",
                                 correlation_type="random_correlation")
    with pytest.raises(ValueError, match="one asset"):
        _bare(pkg, 2).closed_form([1.0], [0.2], [0.0])
    m = _bare(pkg, 1)
    m.payoff_type = "continuous"
    with pytest.raises(ValueError, match="call payoff"):
        m.closed_form([1.0], [0.2], [0.0])
