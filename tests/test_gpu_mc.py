"""dbsde_mc_value on the device against its numpy restatement
(tests/mc_reference.py) on the same Philox draws, its independence of the call's
shape, the closed Euler expectation on the device's own draws, and the Python
surface (FBSNN.mc_value, HestonFBSNN.mc_greeks).  Needs an MI355X.

Tolerance: rtol 2e-5 / atol 2e-6, the tolerance
test_hjb_mc_matches_oracle_on_the_same_draws uses for the same kind of sum (the
device normals are within 2e-6 of the restatement's fp64 ones)."""
import numpy as np
import pytest
import torch

import mc_reference as mr
from conftest import load_pkg

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-6
T_POINTS = np.array([0.0, 0.25, 0.5, 1.0, 0.0], np.float32)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def _equicorr_L(D, rho=0.3):
    return np.linalg.cholesky((1 - rho) * np.eye(D) + rho * np.ones((D, D))).astype(np.float32)


def _specs(pkg, D):
    S = pkg.ProblemSpec
    return {
        "basket": (S(mu_a=0.05, sig_a=0.20, phi_r=0.05, phi_c=0.0, g="call_mean", strike=1.0), None),
        "basket_corr": (S(mu_a=0.05, sig_a=0.20, phi_r=0.05, phi_c=0.0, g="call_mean", strike=1.0), _equicorr_L(D)),
        "call": (S(mu_a=0.05, sig_a=0.20, phi_r=0.05, phi_c=1.0, g="call_sum", strike=1.0 * D), None),
        "bsb": (S(sig_a=0.4, phi_r=0.05, phi_c=1.0, g="sumsq"), None),
        "smooth_call": (S(mu_a=0.05, sig_a=0.20, phi_r=0.05, g="smooth_call", strike=1.0, g_alpha=10.0), None),
        # additive noise, a drift fold with phi_c != 1, and payoff columns that stop before D
        "log_gcols": (S(mu_a=0.03, sig_a=0.10, sig_b=0.2, phi_r=0.02, phi_c=0.5, g="log", g_cols=2), None),
    }


def _device(pkg, dev, spec, t, X, T, n_steps, mc, seed, L=None, delta=False, offset=0):
    v, e, d = pkg.mc_value(spec, torch.from_numpy(np.asarray(t, np.float32)).to(dev),
                           torch.from_numpy(np.asarray(X, np.float32)).to(dev), T, n_steps, mc=mc, seed=seed,
                           offset=offset, L=L, delta=delta)
    torch.cuda.synchronize()
    return v.cpu().numpy()[:, 0], e.cpu().numpy()[:, 0], None if d is None else d.cpu().numpy()


def _check_against(ref, v, e, d, kinked):
    print("value", v, ref["value"], "stderr", e, ref["stderr"], "ambiguous", ref["ambiguous"])
    np.testing.assert_allclose(v, ref["value"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(e, ref["stderr"], rtol=RTOL, atol=ATOL)
    if d is None:
        return
    print("delta", d, ref["delta"])
    slack = ref["delta_slack"] if kinked else 0.0
    tol = ATOL + RTOL * np.abs(ref["delta"]) + slack
    assert np.all(np.abs(d - ref["delta"]) <= tol), (np.abs(d - ref["delta"]).max(), tol.min())


@pytest.mark.parametrize("name", ["basket", "basket_corr", "call", "bsb", "smooth_call", "log_gcols"])
@pytest.mark.parametrize("D,n_steps,mc", [(8, 6, 4096), (3, 1, 1000)])
def test_same_draws_diag(pkg, dev, name, D, n_steps, mc):
    """Value, standard error and pathwise delta == the restatement on the same
    draws.  For the call payoffs a sample whose |a| < 2e-5 in the restatement
    may sit on the other side of the kink on the device; the device delta lies
    within the restatement's +- (sum over those samples of the kink's |dg J|) / mc.
    At most 4 samples per point are ambiguous (asserted)."""
    spec, L = _specs(pkg, D)[name]
    X = np.random.RandomState(11).uniform(0.8, 1.3, (5, D)).astype(np.float32)
    ref = mr.mc_value(spec, T_POINTS, X, 1.0, n_steps, mc, seed=2, L=L, delta=True)
    assert ref["ambiguous"].max() <= 4
    v, e, d = _device(pkg, dev, spec, T_POINTS, X, 1.0, n_steps, mc, 2, L=L, delta=True)
    _check_against(ref, v, e, d, kinked=spec.g in ("call_sum", "call_mean"))
    v2, e2, none = _device(pkg, dev, spec, T_POINTS, X, 1.0, n_steps, mc, 2, L=L, delta=False)
    assert none is None                      # the kernel without the tangent computes the same value
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(e2, e)


def test_same_draws_long_state(pkg, dev):
    """D > 256: a thread runs several coordinates in turn (and a second time
    for the delta); D = 300 is the smallest shape class that takes this path."""
    D, n_steps, mc = 300, 5, 96
    spec = pkg.ProblemSpec(mu_a=0.05, sig_a=0.20, phi_r=0.05, g="smooth_call", strike=1.0, g_alpha=10.0, g_cols=290)
    X = np.random.RandomState(12).uniform(0.8, 1.3, (3, D)).astype(np.float32)
    t = np.array([0.0, 0.5, 1.0], np.float32)
    ref = mr.mc_value(spec, t, X, 1.0, n_steps, mc, seed=4, offset=3, delta=True)
    v, e, d = _device(pkg, dev, spec, t, X, 1.0, n_steps, mc, 4, delta=True, offset=3)
    _check_against(ref, v, e, d, kinked=False)
    assert np.all(d[:, 290:] == 0)


@pytest.mark.parametrize("D", [40, 100])
def test_same_draws_correlated_tiles(pkg, dev, D):
    """The correlated product over more than one 16-row block of L: D = 40 (three
    row blocks, six samples side by side = two 16-column blocks, the second one
    partly empty) and D = 100 (a ragged last row block, two samples = half a
    column block), with a random (not equicorrelated) factor."""
    n_steps, mc = 5, 96
    A = np.random.RandomState(5).normal(size=(D, D))
    C = A @ A.T + D * np.eye(D)
    C /= np.sqrt(np.outer(np.diag(C), np.diag(C)))
    L = np.linalg.cholesky(C).astype(np.float32)
    spec = pkg.ProblemSpec(mu_a=0.05, sig_a=0.20, phi_r=0.05, g="smooth_call", strike=1.0, g_alpha=10.0)
    X = np.random.RandomState(12).uniform(0.8, 1.3, (3, D)).astype(np.float32)
    t = np.array([0.0, 0.5, 0.25], np.float32)
    ref = mr.mc_value(spec, t, X, 1.0, n_steps, mc, seed=4, L=L, delta=True)
    v, e, d = _device(pkg, dev, spec, t, X, 1.0, n_steps, mc, 4, L=L, delta=True)
    _check_against(ref, v, e, d, kinked=False)


@pytest.mark.parametrize("payoff", ["call_mean", "smooth_call"])
@pytest.mark.parametrize("k", [1, 2])
def test_same_draws_heston(pkg, dev, k, payoff):
    """The problem's own Heston process (one Brownian motion per asset drives S
    and v, clamps) against heston_rollout on the same draws; no pathwise delta."""
    spec = pkg.ProblemSpec(kind="heston", mu_a=0.05, phi_r=0.05, phi_c=0.0, g=payoff, strike=1.0, g_alpha=10.0,
                           g_cols=k, u_clamp=True, q3=False, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8)
    rs = np.random.RandomState(11)
    X = np.concatenate([rs.uniform(0.8, 1.3, (5, k)), rs.uniform(0.1, 0.3, (5, k))], 1).astype(np.float32)
    ref = mr.mc_value(spec, T_POINTS, X, 1.0, 6, 4096, seed=2)
    v, e, _ = _device(pkg, dev, spec, T_POINTS, X, 1.0, 6, 4096, 2)
    _check_against(ref, v, e, None, kinked=False)
    with pytest.raises(ValueError, match="Heston"):
        _device(pkg, dev, spec, T_POINTS, X, 1.0, 6, 4096, 2, delta=True)


@pytest.mark.parametrize("name", ["basket_corr", "bsb"])
def test_a_point_does_not_depend_on_the_call(pkg, dev, name):
    """Common random numbers: identical points of one call agree bitwise, a
    point's value / standard error / delta are bitwise the same alone (P = 1), as
    row 3 of a P = 5 call and in the second tile of a P = 11 call, and a call
    repeats bitwise."""
    D = 8
    spec, L = _specs(pkg, D)[name]
    X = np.random.RandomState(11).uniform(0.8, 1.3, (5, D)).astype(np.float32)
    X[4] = X[0]                                # T_POINTS[4] == T_POINTS[0]
    a = _device(pkg, dev, spec, T_POINTS, X, 1.0, 6, 4096, 2, L=L, delta=True)
    b = _device(pkg, dev, spec, T_POINTS, X, 1.0, 6, 4096, 2, L=L, delta=True)
    for u, w in zip(a, b):
        np.testing.assert_array_equal(u, w)
    for u in a:
        np.testing.assert_array_equal(u[0], u[4])
    one = _device(pkg, dev, spec, T_POINTS[2:3], X[2:3], 1.0, 6, 4096, 2, L=L, delta=True)   # t = 0.5
    X11 = np.concatenate([X, X, X[2:3]])[[0, 1, 3, 2, 4, 5, 6, 7, 8, 10, 9]]                # row 3 and row 9 <- X[2]
    t11 = np.concatenate([T_POINTS, T_POINTS, T_POINTS[2:3]])[[0, 1, 3, 2, 4, 5, 6, 7, 8, 10, 9]]
    big = _device(pkg, dev, spec, t11, X11, 1.0, 6, 4096, 2, L=L, delta=True)
    five = _device(pkg, dev, spec, t11[:5], X11[:5], 1.0, 6, 4096, 2, L=L, delta=True)
    for u, w5, w11 in zip(one, five, big):
        np.testing.assert_array_equal(u[0], w5[3])
        np.testing.assert_array_equal(u[0], w11[3])
        np.testing.assert_array_equal(u[0], w11[9])
    assert one[0][0] != a[0][0]                # and it is that point's value, not a constant


def test_known_value_on_the_devices_own_draws(pkg, dev):
    """BSB sumsq, D = 4, 32 steps, 65536 samples: the Euler expectation is
    exp(-r tau) |x|^2 ((1 + mu_eff dt)^2 + sigma^2 dt)^N in closed form (delta:
    2 x_d times the factor).  The device value is within 4 reported standard
    errors of it -- the discount, the drift fold and the standard error at once --
    each delta component within 4 of the restatement's standard errors, and
    exact("bsb") is no further away than that plus the scheme's own bias."""
    D, N, mc = 4, 32, 65536
    spec = pkg.ProblemSpec(sig_a=0.4, phi_r=0.05, phi_c=1.0, g="sumsq")
    X = np.array([[1.0, 0.5, 1.2, 0.8]], np.float32)
    t = np.zeros(1, np.float32)
    v, e, d = _device(pkg, dev, spec, t, X, 1.0, N, mc, 1, delta=True)
    cv, cd = mr.euler_sumsq(spec, X[0], 1.0, N)
    ref = mr.mc_value(spec, t, X, 1.0, N, mc, seed=1, delta=True)
    print("value", v, "stderr", e, "closed", cv, "delta", d, "closed", cd, "delta stderr", ref["delta_stderr"])
    assert e[0] > 0 and abs(v[0] - cv) <= 4 * e[0]
    np.testing.assert_allclose(e, ref["stderr"], rtol=RTOL, atol=ATOL)
    assert np.all(np.abs(d[0] - cd) <= 4 * ref["delta_stderr"][0])
    ex, _ = pkg.exact("bsb", torch.from_numpy(t).to(dev), torch.from_numpy(X).to(dev), 1.0, [0.05, 0.4])
    ex = float(ex.cpu()[0, 0])
    assert abs(v[0] - ex) <= 4 * e[0] + abs(cv - ex)


def test_heston_mc_greeks_are_central_differences_on_the_same_draws(pkg, dev):
    """HestonFBSNN.mc_greeks (k = 1, continuous payoff, h = 0.05) == the
    restatement's central differences on the same draws.  With the value
    tolerance tol = ATOL + RTOL |value|: delta atol = 2 tol / (2 h), gamma atol =
    4 tol / h^2."""
    h, mc = 0.05, 4096
    m = pkg.HestonFBSNN(np.ones((1, 1)), 1.0, 8, 6, 1, None, [2] + 4 * [16] + [1], "Naisnet", "Tanh",
                        payoff_type="continuous", device=dev)
    S = np.array([0.9, 1.0, 1.15], np.float32)
    v = np.array([0.2, 0.15, 0.25], np.float32)
    t = np.array([0.0, 0.5, 0.25], np.float32)
    price, delta, gamma = m.mc_greeks(S, v, t, mc=mc, seed=2, h=h)
    assert price.shape == (3, 1) and delta.shape == (3, 1) and gamma.shape == (3, 1)
    spec = m.problem_spec()
    vals = [mr.mc_value(spec, t, np.stack([S + np.float32(b), v], 1), 1.0, m.N, mc, seed=2)["value"]
            for b in (-h, 0.0, h)]
    tol = ATOL + RTOL * np.abs(vals[1])
    print("price", price[:, 0], vals[1], "delta", delta[:, 0], "gamma", gamma[:, 0])
    assert np.all(np.abs(price[:, 0] - vals[1]) <= tol)
    assert np.all(np.abs(delta[:, 0] - (vals[2] - vals[0]) / (2 * h)) <= 2 * tol / (2 * h))
    assert np.all(np.abs(gamma[:, 0] - (vals[2] - 2 * vals[1] + vals[0]) / h ** 2) <= 4 * tol / h ** 2)
    # [S] rows get v0 appended, as predict starts the variance
    a = m.mc_value(t, S[:, None], mc=256, seed=2)[0]
    b = m.mc_value(t, np.stack([S, np.full(3, m.v0, np.float32)], 1), mc=256, seed=2)[0]
    assert torch.equal(a, b)


def test_fbsnn_mc_value_uses_the_objects_problem_and_cholesky_factor(pkg, dev):
    """BasketCallOption with a correlation: FBSNN.mc_value == solver.mc_value with
    the factor the object handed to set_corr (and differs from the independent one)."""
    D = 8
    np.random.seed(3)
    m = pkg.BasketCallOption(np.ones((1, D)), 1.0, 8, 6, D, 1.0, [D + 1] + 4 * [16] + [1], "Naisnet", "Tanh",
                             "random_correlation", device=dev)
    X = torch.from_numpy(np.random.RandomState(11).uniform(0.8, 1.3, (5, D)).astype(np.float32)).to(dev)
    t = torch.from_numpy(T_POINTS).to(dev)
    got = m.mc_value(t, X, mc=4096, seed=2, delta=True)
    want = pkg.mc_value(m.problem_spec(), t, X, 1.0, 6, mc=4096, seed=2, L=m._L, delta=True)
    indep = pkg.mc_value(m.problem_spec(), t, X, 1.0, 6, mc=4096, seed=2)
    for u, w in zip(got, want):
        assert torch.equal(u, w)
    assert not torch.equal(got[0], indep[0])
    assert got[0].shape == (5, 1) and got[1].shape == (5, 1) and got[2].shape == (5, D)
