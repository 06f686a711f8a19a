"""The two-factor Heston problem (problem kind 2) and its closed form (exact
kind 4) at the C boundary, without a GPU: the new values ride on the existing
entry points (no new symbol, ABI version 3), and every bad argument is
DBSDE_EINVAL before any HIP call."""
import ctypes
import importlib

import pytest

from conftest import load_pkg


@pytest.fixture(scope="module")
def lib():
    pkg = load_pkg()
    importlib.import_module(pkg.__name__ + ".build_lib").build(verbose=False)
    return pkg._lib.load()


def test_kinds_are_bound_to_the_header_values():
    pkg = load_pkg()
    assert pkg._lib.PROBLEM_KINDS["heston2"] == 2
    assert "heston" in pkg._lib.EXACT_KINDS and pkg._lib.EXACT_KINDS["heston"] == 4
    assert pkg.ProblemSpec(kind="heston2").to_c().kind == 2
    assert pkg._lib.ABI_VERSION == 3
    assert hasattr(pkg, "HestonTwoFactorFBSNN") and issubclass(pkg.HestonTwoFactorFBSNN, pkg.HestonFBSNN)


def _create(pkg, lib, layers, **prob):
    cfg = pkg._lib.Config()
    cfg.mode, cfg.activation, cfg.n_layers = pkg._lib.MODES["Naisnet"], 0, len(layers)
    for k, v in enumerate(layers):
        cfg.layers[k] = v
    cfg.problem = pkg.ProblemSpec(kind="heston2", mu_a=0.05, phi_r=0.05, g="call_mean", strike=1.0, u_clamp=True,
                                  q3=False, **prob).to_c()
    ctx = ctypes.c_void_p()
    rc = lib.dbsde_create(ctypes.byref(cfg), ctypes.byref(ctx))
    return rc, ctx, lib.dbsde_last_error(None)


def test_create_refuses_an_odd_state_and_a_bad_rho(lib):
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    rc, ctx, msg = _create(pkg, lib, [6, 16, 16, 16, 16, 1], kappa=2.0, theta=0.2, sigma=0.3, rho=0.8)   # D = 5
    assert rc == E and not ctx.value and b"even" in msg
    rc, ctx, msg = _create(pkg, lib, [5, 16, 16, 16, 16, 1], kappa=2.0, theta=0.2, sigma=0.3, rho=1.5)
    assert rc == E and not ctx.value and b"rho" in msg


def _mc(lib, prob, D=4, L=None, delta=None):
    """Pointers are never dereferenced on these paths: 1 stands for 'not NULL'."""
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    return lib.dbsde_mc_value(ctypes.byref(prob), D, 1.0, vp(L), vp(1), vp(1), 1, 4, 16, 0, 0, vp(1), None, vp(delta),
                              None)


def test_mc_value_refusals_for_kind_2(lib):
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    h2 = pkg.ProblemSpec(kind="heston2", mu_a=0.05, phi_r=0.05, g="call_mean", strike=1.0, g_cols=2, kappa=2.0,
                         theta=0.2, sigma=0.3, rho=0.8).to_c()
    assert h2.kind == 2
    assert _mc(lib, h2, D=5) == E
    assert b"even" in lib.dbsde_last_error(None)
    assert _mc(lib, h2, D=4, L=1) == E
    assert b"DIAG" in lib.dbsde_last_error(None)
    assert _mc(lib, h2, D=4, delta=1) == E
    assert b"Heston" in lib.dbsde_last_error(None) and b"delta" in lib.dbsde_last_error(None)
    bad = pkg.ProblemSpec(kind="heston2", g="call_mean", rho=-1.25).to_c()
    assert _mc(lib, bad, D=4) == E
    assert b"rho" in lib.dbsde_last_error(None)


def test_exact_kind_4_validates_before_any_hip_call(lib):
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    one = ctypes.c_void_p(1)
    p = (ctypes.c_double * 6)(0.05, 1.0, 2.0, 0.2, 0.3, 0.8)
    for D in (1, 3, 4):
        assert lib.dbsde_exact(4, one, one, 1, D, 1.0, p, one, one, None) == E, D
    assert lib.dbsde_exact(4, None, one, 1, 2, 1.0, p, one, one, None) == E
    assert lib.dbsde_exact(4, one, None, 1, 2, 1.0, p, one, one, None) == E
    assert lib.dbsde_exact(4, one, one, 1, 2, 1.0, None, one, one, None) == E
    assert lib.dbsde_exact(4, one, one, 1, 2, 1.0, p, None, one, None) == E
    assert lib.dbsde_exact(4, one, one, 0, 2, 1.0, p, one, one, None) == E
    assert lib.dbsde_exact(5, one, one, 1, 2, 1.0, p, one, one, None) == E
    with pytest.raises(ValueError, match="unknown exact"):
        pkg.exact("heston1", None, None, 1.0, ())
