"""dbsde_mc_value (the Feynman-Kac Monte-Carlo comparator) without a GPU: the
symbol is exported and bound, every bad argument is DBSDE_EINVAL before any
HIP call, the Python surface rejects the HJB problem, and the numpy
restatement the GPU tests compare against (tests/mc_reference.py) is itself
right: closed Euler expectation, maturity."""
import ctypes
import importlib
import subprocess

import numpy as np
import pytest

import mc_reference as mr
from conftest import load_pkg


@pytest.fixture(scope="module")
def lib():
    pkg = load_pkg()
    importlib.import_module(pkg.__name__ + ".build_lib").build(verbose=False)
    return pkg._lib.load()


def test_symbol_is_exported_and_bound(lib):
    pkg = load_pkg()
    assert "dbsde_mc_value" in pkg._lib.EXPORTED
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert " T dbsde_mc_value" in out
    assert lib.dbsde_mc_value.argtypes is not None and len(lib.dbsde_mc_value.argtypes) == 15
    assert callable(pkg.mc_value) and hasattr(pkg.FBSNN, "mc_value") and hasattr(pkg.HestonFBSNN, "mc_greeks")


def _call(lib, prob, D=4, T=1.0, L=None, t=1, x=1, P=1, n_steps=4, mc=16, value=1, err=None, delta=None):
    """Pointers are never dereferenced on these paths: 1 stands for 'not NULL'
    (every call here must be rejected before any HIP call; there is no device)."""
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    return lib.dbsde_mc_value(ctypes.byref(prob) if prob is not None else None, D, T, vp(L), vp(t), vp(x), P, n_steps,
                              mc, 0, 0, vp(value), vp(err), vp(delta), None)


def test_every_bad_argument_is_einval_before_any_hip_call(lib):
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    diag = pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, g="call_mean", strike=1.0).to_c()
    hes = pkg.ProblemSpec(kind="heston", mu_a=0.05, phi_r=0.05, g="call_mean", strike=1.0, g_cols=2, kappa=2.0,
                          theta=0.2, sigma=0.3, rho=0.8).to_c()
    assert _call(lib, None) == E
    assert _call(lib, diag, t=None) == E
    assert _call(lib, diag, x=None) == E
    assert _call(lib, diag, value=None) == E
    for kw in (dict(P=0), dict(D=0), dict(n_steps=0), dict(mc=0), dict(mc=2 ** 32 + 1), dict(D=4097)):
        assert _call(lib, diag, **kw) == E, kw
    assert _call(lib, hes, D=5) == E
    assert b"even" in lib.dbsde_last_error(None)
    assert _call(lib, hes, D=4, L=1) == E
    assert _call(lib, hes, D=4, delta=1) == E
    assert b"Heston" in lib.dbsde_last_error(None)
    assert _call(lib, diag, D=129, L=1) == E
    bad = pkg.ProblemSpec().to_c()
    bad.g_kind = 9
    assert _call(lib, bad) == E
    bad = pkg.ProblemSpec().to_c()
    bad.kind = 7
    assert _call(lib, bad) == E
    hjb = pkg.ProblemSpec(sig_b=2.0 ** 0.5, phi_zz=1.0, g="log").to_c()
    assert _call(lib, hjb) == E
    assert b"dbsde_hjb_mc" in lib.dbsde_last_error(None)
    with pytest.raises(ValueError, match="hjb_mc"):
        pkg._lib.check(E)


def test_python_surface_rejects_hjb_and_generic_problems():
    """FBSNN.mc_value refuses before it touches a device: an HJB spec names
    hjb_mc, a problem on the generic (plugin) path has no spec to simulate."""
    pkg = load_pkg()
    m = object.__new__(pkg.HamiltonJacobiBellman)     # no device here: the check needs none
    m.native_coefficients, m.generic_reason = True, None
    with pytest.raises(ValueError, match="hjb_mc"):
        m.mc_value(np.zeros(1), np.zeros((1, 4)))
    with pytest.raises(ValueError, match="hjb_mc"):
        pkg.mc_value(m.problem_spec(), None, None, 1.0, 4)
    m = object.__new__(pkg.CallOption)
    m.native_coefficients, m.generic_reason = False, "no problem_spec()"
    with pytest.raises(ValueError, match="coefficient methods"):
        m.mc_value(np.zeros(1), np.zeros((1, 4)))


def test_restatement_matches_the_closed_euler_expectation():
    """D = 1, sumsq: E[X_N^2] = x^2 ((1 + mu_eff dt)^2 + sig_a^2 dt)^N exactly for
    the Euler scheme; the restatement is within 4 of its own standard errors
    (value and delta), with the drift fold mu_eff = 0 + 0.05 * 1."""
    pkg = load_pkg()
    spec = pkg.ProblemSpec(sig_a=0.4, phi_r=0.05, phi_c=1.0, g="sumsq")
    assert mr.mu_eff(spec) == np.float32(0.05)
    x, N, mc = np.array([[1.1]], np.float32), 8, 16384
    r = mr.mc_value(spec, [0.25], x, 1.0, N, mc, seed=3, delta=True)
    v, dv = mr.euler_sumsq(spec, x[0], 0.75, N)
    assert r["stderr"][0] > 0 and abs(r["value"][0] - v) <= 4 * r["stderr"][0]
    assert abs(r["delta"][0, 0] - dv[0]) <= 4 * r["delta_stderr"][0, 0]
    # and the continuous limit is DBSDE_EXACT_BSB's exp((r + s^2) tau) |x|^2, an O(dt) away
    assert abs(v - np.exp((0.05 + 0.16) * 0.75) * 1.1 ** 2) < 0.02


@pytest.mark.parametrize("g", ["sumsq", "call_sum", "call_mean", "log", "smooth_call"])
def test_restatement_at_maturity_returns_payoff_and_gradient(g):
    pkg = load_pkg()
    spec = pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, g=g, strike=1.0, g_alpha=10.0, g_cols=2)
    X = np.array([[1.5, 0.9, 7.0], [0.5, 1.5, 7.0], [0.2, 0.3, 7.0]], np.float32)   # a > 0, a == 0 (mean), a < 0
    r = mr.mc_value(spec, [1.0, 1.0, 2.0], X, 1.0, 4, 8, delta=True)
    gx, dgx, _ = mr.payoff(spec, X)
    np.testing.assert_array_equal(r["value"], gx)
    np.testing.assert_array_equal(r["delta"], dgx)
    np.testing.assert_array_equal(r["stderr"], 0.0)
    assert np.all(r["delta"][:, 2] == 0)          # past g_cols
    eps = 1e-6                                    # dg is the gradient of g (away from the kink)
    for d in range(2):
        Xp, Xm = X.astype(np.float64).copy(), X.astype(np.float64).copy()
        Xp[:, d] += eps
        Xm[:, d] -= eps
        fd = (mr.payoff(spec, Xp)[0] - mr.payoff(spec, Xm)[0]) / (2 * eps)
        ok = np.ones(3, bool) if g in ("sumsq", "log", "smooth_call") else np.array([True, False, True])
        np.testing.assert_allclose(dgx[ok, d], fd[ok], rtol=1e-6, atol=1e-8)
    if g == "call_mean":
        assert dgx[1, 0] == 0.25                  # 1/2 at the kink, / cols
