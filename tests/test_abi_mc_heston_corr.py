"""DBSDE_PROB_HESTON_CORR (dbsde_mc_value's kind for the correlated k-asset
Heston) without a GPU: the header value, unchanged exports and ABI version,
every refusal before any HIP call, dbsde_create's refusal, the Python checks
that need no device, and the numpy restatement the GPU tests compare against
(tests/mc_heston_corr_reference.py) on the case the correlation shows in."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mc_heston_corr_reference as hr
from conftest import load_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the exported symbols of ABI version 3
EXPORTED = sorted([
    "dbsde_abi_version", "dbsde_create", "dbsde_destroy", "dbsde_last_error", "dbsde_set_stream", "dbsde_param_count",
    "dbsde_param_used_mask", "dbsde_matrix_form", "dbsde_brownian_dim", "dbsde_set_corr", "dbsde_brownian",
    "dbsde_prefetch", "dbsde_prefetch_cancel", "dbsde_loss_grad", "dbsde_net_u", "dbsde_net_u_vjp", "dbsde_net_u_xvjp",
    "dbsde_net_u_jet", "dbsde_pde_residual", "dbsde_optimizer_step", "dbsde_exact", "dbsde_hjb_mc", "dbsde_mc_value",
    "dbsde_profile_enable", "dbsde_profile_count", "dbsde_profile_read", "dbsde_profile_reset", "dbsde_vec_reduce",
    "dbsde_vec_axpby", "dbsde_lbfgs_direction", "dbsde_train_step", "dbsde_stream_order_by_events",
])


@pytest.fixture(scope="module")
def lib():
    pkg = load_pkg()
    importlib.import_module(pkg.__name__ + ".build_lib").build(verbose=False)
    return pkg._lib.load()


def test_header_defines_kind_3_and_nothing_else_moves(lib):
    pkg = load_pkg()
    header = open(os.path.join(ROOT, "include", "dbsde.h")).read()
    kinds = dict(re.findall(r"#define (DBSDE_PROB_\w+) (\d+)", header))
    assert kinds == {"DBSDE_PROB_DIAG": "0", "DBSDE_PROB_HESTON": "1", "DBSDE_PROB_HESTON2": "2",
                     "DBSDE_PROB_HESTON_CORR": "3"}
    assert pkg._lib.PROB_HESTON_CORR == 3
    assert pkg._lib.PROBLEM_KINDS == {"diag": 0, "heston": 1, "heston2": 2}     # kind 3 is not a context kind
    assert re.search(r"#define DBSDE_ABI_VERSION 3\b", header)
    assert lib.dbsde_abi_version() == pkg._lib.ABI_VERSION == 3
    assert sorted(pkg._lib.EXPORTED) == EXPORTED
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert sorted(set(re.findall(r"\bT (dbsde_\w+)", out))) == EXPORTED


def _mc(lib, prob, D=4, L=1, delta=None, n_steps=4):
    """Pointers are never dereferenced on these paths: 1 stands for 'not NULL'
    (every call here must be rejected before any HIP call; there is no device)."""
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    rc = lib.dbsde_mc_value(ctypes.byref(prob), D, 1.0, vp(L), vp(1), vp(1), 1, n_steps, 16, 0, 0, vp(1), None,
                            vp(delta), None)
    return rc, lib.dbsde_last_error(None)


def _kind3(pkg):
    prob = hr.spec_for(pkg, 2).to_c()
    prob.kind = pkg._lib.PROB_HESTON_CORR
    return prob


def test_every_refusal_of_kind_3_is_einval_before_any_hip_call(lib):
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    prob = _kind3(pkg)
    rc, msg = _mc(lib, prob, L=None)
    assert rc == E and re.search(rb"\bL\b", msg), msg
    rc, msg = _mc(lib, prob, D=5)
    assert rc == E and b"even" in msg, msg
    rc, msg = _mc(lib, prob, delta=1)
    assert rc == E and b"Heston" in msg and b"delta" in msg, msg
    kind1 = hr.spec_for(pkg, 2).to_c()
    rc1, msg1 = _mc(lib, kind1, L=None, delta=1)
    assert rc1 == E and msg1 == msg                                   # kind 1's wording
    rc, msg = _mc(lib, prob, D=2 * 512)
    assert rc == E and b"511" in msg, msg
    rc, msg = _mc(lib, prob, n_steps=4 * 65535 + 1)                   # the increment launch's grid.y
    assert rc == E and b"n_steps" in msg, msg
    # what the other kinds refused before, they still refuse
    rc, msg = _mc(lib, kind1, L=1)
    assert rc == E and b"DIAG" in msg, msg
    prob.kind = 7
    assert _mc(lib, prob)[0] == E
    with pytest.raises(ValueError):
        pkg._lib.check(E)


def test_create_refuses_kind_3(lib):
    pkg = load_pkg()
    cfg = pkg._lib.Config()
    layers = [5, 16, 16, 16, 16, 1]
    cfg.mode, cfg.activation, cfg.n_layers = pkg._lib.MODES["Naisnet"], 0, len(layers)
    for k, v in enumerate(layers):
        cfg.layers[k] = v
    cfg.problem = _kind3(pkg)
    ctx = ctypes.c_void_p()
    rc = lib.dbsde_create(ctypes.byref(cfg), ctypes.byref(ctx))
    msg = lib.dbsde_last_error(None)
    assert rc == pkg._lib.DBSDE_EINVAL and not ctx.value
    assert b"dbsde_set_corr" in msg and b"DBSDE_PROB_HESTON" in msg, msg


def test_python_surface_checks_the_factor_without_a_device():
    """The shape of L ([k, k] for kind "heston", no longer [D, D]) and the
    two-factor model's refusal come before anything touches a device: the
    tensors here are host tensors."""
    pkg = load_pkg()
    k = 3
    t, X = torch.zeros(2), torch.ones(2, 2 * k)
    spec = hr.spec_for(pkg, k)
    for shape in ((2 * k, 2 * k), (k, k + 1), (k + 1, k + 1), (k,)):
        with pytest.raises(ValueError, match=rf"L must be \[{k}, {k}\]"):
            pkg.mc_value(spec, t, X, 1.0, 4, L=np.zeros(shape, np.float32))
    with pytest.raises(ValueError, match=r"L must be \[2, 2\]"):      # an odd state: k = D // 2 cannot be right
        pkg.mc_value(spec, t, torch.ones(2, 5), 1.0, 4, L=np.eye(2, dtype=np.float32))
    h2 = pkg.ProblemSpec(kind="heston2", g="call_mean", strike=1.0, g_cols=k, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8)
    with pytest.raises(ValueError, match="two-factor"):
        pkg.mc_value(h2, t, X, 1.0, 4, L=np.eye(k, dtype=np.float32))
    with pytest.raises(ValueError, match=r"L must be \[6, 6\]"):      # diag problems keep [D, D]
        pkg.mc_value(pkg.ProblemSpec(sig_a=0.2, g="call_mean"), t, X, 1.0, 4, L=np.eye(k, dtype=np.float32))
    # a right factor passes these checks and stops at the device check
    with pytest.raises(ValueError, match="HIP device"):
        pkg.mc_value(spec, t, X, 1.0, 4, L=np.eye(k, dtype=np.float32))


def test_restatement_shows_the_correlation():
    """k = 8, equicorrelation 0.9, S = 1, v = 0.2, T = 1, 10 steps, call on the
    mean at strike 1, 2^14 samples: the correlated and the independent value
    differ by more than 6 x the sum of their standard errors (at 4096 samples:
    0.107 against a summed standard error of 0.024)."""
    pkg = load_pkg()
    corr, ind = hr.gap_case(pkg)
    print("correlated", corr, "independent", ind)
    gap = abs(corr["value"][0] - ind["value"][0])
    assert gap > 6 * (corr["stderr"][0] + ind["stderr"][0])
    assert 0.08 < gap < 0.13 and ind["value"][0] < corr["value"][0]
    # L = None is mc_reference's Heston branch, L = I draws the same increments
    import mc_reference as mr
    t, X = hr.gap_point()
    spec = hr.spec_for(pkg, hr.GAP_K)
    want = mr.mc_value(spec, t, X, 1.0, hr.GAP_STEPS, 512, seed=3)
    for L in (None, np.eye(hr.GAP_K)):
        got = hr.mc_value(spec, t, X, 1.0, hr.GAP_STEPS, 512, seed=3, L=L)
        np.testing.assert_array_equal(got["value"], want["value"])
        np.testing.assert_array_equal(got["stderr"], want["stderr"])


def test_restatement_product_orders_agree_to_rounding():
    """The two evaluations of L . (sqrt(dt) z) the restatement offers -- an fp64
    product rounded once, and fp32 sums in 16-wide chunks -- are fp32 roundings of
    the same product: they differ by at most the bound of a k-term fp32 sum,
    k eps sum_j |L_dj| max |dw_j|, and they do differ."""
    k, mc, n = 40, 32, 5
    L = hr.equicorr_factor(k, 0.5)
    a = hr.increments(2, 0, mc, n, k, 0.5, L, "fp64")
    b = hr.increments(2, 0, mc, n, k, 0.5, L, "fp32_chunks")
    dw = hr.increments(2, 0, mc, n, k, 0.5, None)
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (mc, n, k)
    rows = np.abs(L).sum(1).max()
    assert 0 < np.abs(a - b).max() <= k * np.finfo(np.float32).eps * rows * np.abs(dw).max()
