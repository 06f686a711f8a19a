"""The put payoffs at the C boundary: terminal conditions DBSDE_G_PUT_SUM /
PUT_MEAN / SMOOTH_PUT (5..7) and closed forms DBSDE_EXACT_BS_PUT /
BASKET_AVG_PUT / BASKET_MEAN_PUT / HESTON_PUT (5..8) ride on the existing entry
points: the header values equal the binding's tables, the ABI version is 3,
g_kind 9 and exact kind 9 are still refused, and the new values pass the
argument checks.  No GPU needed."""
import ctypes
import importlib
import os
import re

import pytest
import torch

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "dbsde.h")
G = {"put_sum": ("DBSDE_G_PUT_SUM", 5), "put_mean": ("DBSDE_G_PUT_MEAN", 6), "smooth_put": ("DBSDE_G_SMOOTH_PUT", 7)}
EXACT = {"bs_put": ("DBSDE_EXACT_BS_PUT", 5), "basket_avg_put": ("DBSDE_EXACT_BASKET_AVG_PUT", 6),
         "basket_mean_put": ("DBSDE_EXACT_BASKET_MEAN_PUT", 7), "heston_put": ("DBSDE_EXACT_HESTON_PUT", 8)}


@pytest.fixture(scope="module")
def lib():
    pkg = load_pkg()
    importlib.import_module(pkg.__name__ + ".build_lib").build(verbose=False)
    return pkg._lib.load()


def header_values():
    return {n: int(v) for n, v in re.findall(r"^#define (DBSDE_\w+) (-?\d+)\b", open(HEADER).read(), flags=re.M)}


def test_header_values_equal_the_binding_tables():
    pkg = load_pkg()
    hv = header_values()
    for name, (macro, value) in G.items():
        assert hv[macro] == value == pkg._lib.G_KINDS[name], name
        assert pkg.ProblemSpec(g=name).to_c().g_kind == value
    for name, (macro, value) in EXACT.items():
        assert hv[macro] == value == pkg._lib.EXACT_KINDS[name], name
    # the existing values keep theirs, and nothing else moved
    assert [pkg._lib.G_KINDS[n] for n in ("sumsq", "call_sum", "call_mean", "log", "smooth_call")] == [0, 1, 2, 3, 4]
    assert [pkg._lib.EXACT_KINDS[n] for n in ("bsb", "bs_call", "basket_avg", "basket_mean", "heston")] == [0, 1, 2, 3, 4]
    assert hv["DBSDE_ABI_VERSION"] == pkg._lib.ABI_VERSION == 3
    assert len(pkg._lib.EXPORTED) == 32
    for name in ("PutOption", "BasketPutOption"):
        assert hasattr(pkg, name) and name in pkg.__all__
    assert issubclass(pkg.PutOption, pkg.CallOption) and issubclass(pkg.BasketPutOption, pkg.BasketCallOption)


def _mc(lib, prob, t, x, value, D=4):
    vp = lambda v: ctypes.c_void_p(v)
    return lib.dbsde_mc_value(ctypes.byref(prob), D, 1.0, None, vp(t), vp(x), 1, 4, 16, 0, 0, vp(value), None, None, None)


def test_the_pins_still_hold(lib):
    """Every call here is refused before any HIP call: 1 stands for 'not NULL'."""
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    bad = pkg.ProblemSpec().to_c()
    bad.g_kind = 9
    assert _mc(lib, bad, 1, 1, 1) == E
    assert b"unknown terminal condition" in lib.dbsde_last_error(None)
    bad.g_kind = 8
    assert _mc(lib, bad, 1, 1, 1) == E
    one = ctypes.c_void_p(1)
    p = (ctypes.c_double * 6)(0.05, 1.0, 2.0, 0.2, 0.3, 0.8)
    assert lib.dbsde_exact(9, one, one, 1, 2, 1.0, p, one, one, None) == E
    al = ctypes.c_void_p(4096)
    assert lib.dbsde_exact(9, al, al, 1, 2, 1.0, p, al, al, None) == E
    # an address that cannot hold floats is refused for every kind, old and new, before any launch
    for kind in range(9):
        for bad in range(4):
            ptrs = [one if k == bad else al for k in range(4)]
            assert lib.dbsde_exact(kind, ptrs[0], ptrs[1], 1, 2, 1.0, p, ptrs[2], ptrs[3], None) == E, (kind, bad)
    for D in (1, 3, 4):                           # the Heston put needs x = (S, v), as the call does
        assert lib.dbsde_exact(8, one, one, 1, D, 1.0, p, one, one, None) == E, D
    for kind in (5, 6, 7, 8):
        assert lib.dbsde_exact(kind, None, one, 1, 2, 1.0, p, one, one, None) == E
        assert lib.dbsde_exact(kind, one, one, 0, 2, 1.0, p, one, one, None) == E
    cfg = pkg._lib.Config()
    cfg.mode, cfg.activation, cfg.n_layers = 1, 0, 6
    for k, v in enumerate([5, 16, 16, 16, 16, 1]):
        cfg.layers[k] = v
    cfg.problem = pkg.ProblemSpec().to_c()
    cfg.problem.g_kind = 9
    ctx = ctypes.c_void_p()
    assert lib.dbsde_create(ctypes.byref(cfg), ctypes.byref(ctx)) == E and not ctx.value
    assert b"unknown terminal condition" in lib.dbsde_last_error(None)
    with pytest.raises(ValueError, match="unknown terminal"):
        pkg.ProblemSpec(g="put_max").to_c()
    with pytest.raises(ValueError, match="unknown exact"):
        pkg.exact("put", None, None, 1.0, ())


def test_the_new_values_pass_the_argument_checks(lib):
    """dbsde_mc_value and dbsde_exact no longer refuse the new values.  Without
    a device the calls stop at the first HIP call (DBSDE_ENOMEM / DBSDE_EHIP)
    and never read their pointers; with one they run on real one-point
    buffers and succeed."""
    pkg = load_pkg()
    gpu = torch.cuda.is_available()
    if gpu:
        t = torch.zeros(1, device="cuda:0")
        x = torch.ones(4, device="cuda:0")
        out = torch.empty(4, device="cuda:0")
        dlt = torch.empty(4, device="cuda:0")
        tp, xp, op, dp = (v.data_ptr() for v in (t, x, out, dlt))
    else:
        tp = xp = op = dp = 4096                     # never read: aligned like a buffer, as the entry points require
    vp = ctypes.c_void_p
    p = (ctypes.c_double * 6)(0.05, 1.0, 2.0, 0.2, 0.3, 0.8)
    for name in G:
        rc = _mc(lib, pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, g=name, strike=1.0, g_alpha=10.0).to_c(),
                 tp, xp, op)
        assert rc != pkg._lib.DBSDE_EINVAL and (rc == pkg._lib.DBSDE_OK) == gpu, (name, rc, lib.dbsde_last_error(None))
    for name, (_, kind) in EXACT.items():
        D = 2 if name == "heston_put" else 4
        rc = lib.dbsde_exact(kind, vp(tp), vp(xp), 1, D, 1.0, p, vp(op), vp(dp), None)
        assert rc != pkg._lib.DBSDE_EINVAL and (rc == pkg._lib.DBSDE_OK) == gpu, (name, rc)
    if gpu:
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
