"""dbsde_mc_value for the correlated k-asset Heston (DBSDE_PROB_HESTON_CORR) on
the device: against its numpy restatement (tests/mc_heston_corr_reference.py)
on the same draws, bitwise against the uncorrelated kind with L = I, bitwise
across workspace groupings and call shapes, the correlation in the value, and
the Python surface (FBSNN.mc_value, HestonFBSNN.mc_greeks of a correlated
object).  Needs an MI355X.

Tolerance: tests/test_gpu_mc.py's rtol 2e-5 / atol 2e-6."""
import os

import numpy as np
import pytest
import torch

import heston_corr_reference as hc
import mc_heston_corr_reference as hr
import mc_reference as mr
from conftest import load_pkg

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-6
T_POINTS = np.array([0.0, 0.25, 0.5, 1.0, 0.0], np.float32)     # tau = 0 and a repeated time
N_STEPS = 6                                                     # one whole Philox block and a ragged one


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


@pytest.fixture
def ws_env():
    """Restores DBSDE_MC_WS_MB (read by the library at every call)."""
    old = os.environ.get("DBSDE_MC_WS_MB")
    yield
    if old is None:
        os.environ.pop("DBSDE_MC_WS_MB", None)
    else:
        os.environ["DBSDE_MC_WS_MB"] = old


def _points(k, P=5, seed=11):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.uniform(0.8, 1.3, (P, k)), rs.uniform(0.1, 0.3, (P, k))], 1).astype(np.float32)


def _device(pkg, dev, spec, t, X, n_steps, mc, seed, L=None, offset=0):
    v, e, d = pkg.mc_value(spec, torch.from_numpy(np.asarray(t, np.float32)).to(dev),
                           torch.from_numpy(np.asarray(X, np.float32)).to(dev), 1.0, n_steps, mc=mc, seed=seed,
                           offset=offset, L=L)
    torch.cuda.synchronize()
    assert d is None
    return v.cpu().numpy()[:, 0], e.cpu().numpy()[:, 0]


def _close(got, ref):
    print("value", got[0], ref["value"], "stderr", got[1], ref["stderr"],
          "deviation / bound", np.max(np.abs(got[0] - ref["value"]) / (ATOL + RTOL * np.abs(ref["value"]))),
          np.max(np.abs(got[1] - ref["stderr"]) / (ATOL + RTOL * np.abs(ref["stderr"]))))
    np.testing.assert_allclose(got[0], ref["value"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got[1], ref["stderr"], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("payoff", ["call_mean", "smooth_call"])
@pytest.mark.parametrize("k", [1, 3, 17, 130, 300])
def test_same_draws_against_the_restatement(pkg, dev, k, payoff):
    """Value and standard error == the restatement on the same draws.  k = 1: one
    output block of the increment product with seven idle waves; 3: a ragged
    block; 17: the second block; 130: a factor beyond 128; 300: a thread runs two
    assets in turn.  mc = 1000 (k <= 17) leaves a partial 16-sample group.
    Measured on an MI355X: the largest deviation of any case is 0.003 of the
    bound (k = 1, smooth_call), at k = 300 it is 0.001 (call_mean) and 0.002
    (smooth_call) of the bound -- the summation order of the increment product
    needs no allowance of its own."""
    mc = 1000 if k <= 17 else 96
    spec = hr.spec_for(pkg, k, payoff)
    L = hc.random_factor(k)
    X = _points(k)
    ref = hr.mc_value(spec, T_POINTS, X, 1.0, N_STEPS, mc, seed=2, offset=3, L=L)
    got = _device(pkg, dev, spec, T_POINTS, X, N_STEPS, mc, 2, L=L, offset=3)
    _close(got, ref)
    assert got[1][3] == 0                       # tau = 0: the payoff, no standard error


@pytest.mark.parametrize("k", [3, 50])
def test_identity_factor_is_the_uncorrelated_kind_bitwise(pkg, dev, k):
    """L = I: products with 1 and sums with 0 are exact, so the increments are the
    uncorrelated kind's normals and value and standard error are kind 1's bits."""
    spec = hr.spec_for(pkg, k)
    X = _points(k)
    want = _device(pkg, dev, spec, T_POINTS, X, N_STEPS, 1000, 2)
    got = _device(pkg, dev, spec, T_POINTS, X, N_STEPS, 1000, 2, L=np.eye(k))
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert want[1][0] > 0


def test_grouping_does_not_change_bits(pkg, dev, ws_env):
    """k = 17, mc = 4096, 6 steps: 137 chunks of 30 samples, 12240 bytes of
    increments each.  A workspace bound of 1/4 MB holds 21 chunks: 7 groups,
    against one group at the default; the results are bitwise equal, and the
    profile of the context-free calls counts the increment launches."""
    k, mc = 17, 4096
    spec = hr.spec_for(pkg, k)
    L = hc.random_factor(k)
    X = _points(k)

    def run(mb):
        if mb is None:
            os.environ.pop("DBSDE_MC_WS_MB", None)
        else:
            os.environ["DBSDE_MC_WS_MB"] = mb
        pkg.free_call_profile(enable=True, reset=True)
        out = _device(pkg, dev, spec, T_POINTS, X, N_STEPS, mc, 2, L=L)
        prof = pkg.free_call_profile(enable=False)
        return out, prof["corr_increments"]["launches"], prof["mc_heston_corr_paths"]["launches"]

    whole, n1, p1 = run(None)
    split, n7, p7 = run("0.25")
    chunk, n137, p137 = run("0.001")                 # below one chunk: every chunk a group of its own
    print("increment launches", n1, n7, n137)
    assert (n1, p1) == (1, 1) and (n7, p7) == (7, 7) and (n137, p137) == (137, 137)
    for other in (split, chunk):
        np.testing.assert_array_equal(other[0], whole[0])
        np.testing.assert_array_equal(other[1], whole[1])
    # not recorded while the store is off
    pkg.free_call_profile(reset=True)
    _device(pkg, dev, spec, T_POINTS, X, N_STEPS, 64, 2, L=L)
    assert pkg.free_call_profile()["corr_increments"]["launches"] == 0


def test_a_point_does_not_depend_on_the_call(pkg, dev):
    """Common random numbers: duplicated points of one call agree bitwise, a point
    alone (P = 1) has the bits it has as row 3 and as row 8 (the second tile) of a
    P = 9 call, and a call repeats bitwise."""
    k, mc = 17, 1000
    spec = hr.spec_for(pkg, k, "smooth_call")
    L = hc.random_factor(k)
    X = _points(k)
    X[4] = X[0]                                   # T_POINTS[4] == T_POINTS[0]
    a = _device(pkg, dev, spec, T_POINTS, X, N_STEPS, mc, 2, L=L)
    b = _device(pkg, dev, spec, T_POINTS, X, N_STEPS, mc, 2, L=L)
    for u, w in zip(a, b):
        np.testing.assert_array_equal(u, w)
        np.testing.assert_array_equal(u[0], u[4])
    one = _device(pkg, dev, spec, T_POINTS[2:3], X[2:3], N_STEPS, mc, 2, L=L)
    idx = [0, 1, 3, 2, 4, 0, 1, 3, 2]
    nine = _device(pkg, dev, spec, T_POINTS[idx], X[idx], N_STEPS, mc, 2, L=L)
    for u, w in zip(one, nine):
        np.testing.assert_array_equal(u[0], w[3])
        np.testing.assert_array_equal(u[0], w[8])
    assert one[0][0] != a[0][0]                   # and it is that point's value, not a constant


def test_the_correlation_is_in_the_value(pkg, dev):
    """k = 8, equicorrelation 0.9, S = 1, v = 0.2, T = 1, 10 steps, call on the
    mean at strike 1, 2^14 samples: the device's correlated and uncorrelated
    values differ by more than 6 x the sum of the device's standard errors, and
    each is its restatement's."""
    ref_c, ref_i = hr.gap_case(pkg)
    spec = hr.spec_for(pkg, hr.GAP_K)
    t, X = hr.gap_point()
    corr = _device(pkg, dev, spec, t, X, hr.GAP_STEPS, hr.GAP_MC, hr.GAP_SEED, L=hr.equicorr_factor(hr.GAP_K, hr.GAP_RHO))
    ind = _device(pkg, dev, spec, t, X, hr.GAP_STEPS, hr.GAP_MC, hr.GAP_SEED)
    _close(corr, ref_c)
    _close(ind, ref_i)
    assert abs(corr[0][0] - ind[0][0]) > 6 * (corr[1][0] + ind[1][0])


def _heston_object(pkg, dev, correlation_type, **kw):
    """HestonFBSNN(k = 3) as tests/test_gpu_heston_corr.py's heston_object builds
    it: the factor drawn right after np.random.seed(hc.PDE_SEED)."""
    k = hc.PDE_K
    np.random.seed(hc.PDE_SEED)
    m = pkg.HestonFBSNN(np.ones((1, k)), hc.T, 24, hc.N, k, None, [2] + 4 * [16] + [1], "Naisnet", "Tanh",
                        correlation_type=correlation_type, device=dev, **kw)
    assert m.native_coefficients
    return m


def test_python_surface_of_a_correlated_object(pkg, dev):
    """FBSNN.mc_value of a correlated Heston object == solver.mc_value with the
    factor the object handed to set_corr, and differs from the independent
    call; mc_greeks (h = 0.05) == the restatement's central differences on the
    same correlated draws, with the bounds of
    test_heston_mc_greeks_are_central_differences_on_the_same_draws: value
    tolerance tol = ATOL + RTOL |value|, delta 2 tol / (2 h), gamma 4 tol / h^2."""
    k, mc, h = hc.PDE_K, 4096, 0.05
    m = _heston_object(pkg, dev, "random_correlation", payoff_type="continuous")
    np.testing.assert_array_equal(m._L, hc.object_factor(pkg))
    assert np.abs(np.tril(m._L, -1)).max() > 0
    X = torch.from_numpy(_points(k)).to(dev)
    t = torch.from_numpy(T_POINTS).to(dev)
    spec = m.problem_spec()
    got = m.mc_value(t, X, mc=mc, seed=2)
    want = pkg.mc_value(spec, t, X, hc.T, hc.N, mc=mc, seed=2, L=m._L)
    indep = pkg.mc_value(spec, t, X, hc.T, hc.N, mc=mc, seed=2)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] is None
    assert not torch.equal(got[0], indep[0])
    assert got[0].shape == (5, 1) and got[1].shape == (5, 1)

    S = np.array([[0.9, 1.0, 1.1], [1.0, 1.05, 0.95], [1.15, 0.9, 1.0]], np.float32)
    v = np.array([[0.2, 0.15, 0.25], [0.15, 0.2, 0.2], [0.25, 0.2, 0.1]], np.float32)
    tg = np.array([0.0, 0.5, 0.25], np.float32)
    price, delta, gamma = m.mc_greeks(S, v, tg, mc=mc, seed=2, h=h)
    assert price.shape == (3, 1) and delta.shape == (3, k) and gamma.shape == (3, k)
    vals = [hr.mc_value(spec, tg, np.concatenate([S + np.float32(b), v], 1), hc.T, m.N, mc, seed=2, L=m._L)["value"]
            for b in (-h, 0.0, h)]
    tol = ATOL + RTOL * np.abs(vals[1])
    print("price", price[:, 0], vals[1], "delta", delta[:, 0], "gamma", gamma[:, 0])
    assert np.all(np.abs(price[:, 0] - vals[1]) <= tol)
    assert np.all(np.abs(delta[:, 0] - (vals[2] - vals[0]) / (2 * h)) <= 2 * tol / (2 * h))
    assert np.all(np.abs(gamma[:, 0] - (vals[2] - 2 * vals[1] + vals[0]) / h ** 2) <= 4 * tol / h ** 2)
    ind = mr.mc_value(spec, tg, np.concatenate([S, v], 1), hc.T, m.N, mc, seed=2)["value"]
    assert np.all(np.abs(price[:, 0] - ind) > 10 * tol)          # and not the independent assets' price


def test_python_surface_of_an_uncorrelated_object(pkg, dev):
    """An uncorrelated Heston object's mc_value is bitwise solver.mc_value without
    a factor (kind 1, as before)."""
    k = hc.PDE_K
    m = _heston_object(pkg, dev, "no_correlation")
    assert m._L is None
    X = torch.from_numpy(_points(k)).to(dev)
    t = torch.from_numpy(T_POINTS).to(dev)
    got = m.mc_value(t, X, mc=1000, seed=2)
    want = pkg.mc_value(m.problem_spec(), t, X, hc.T, hc.N, mc=1000, seed=2)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
