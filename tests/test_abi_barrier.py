"""The knock-out problem (problem kind 11, DBSDE_PROB_BARRIER) and its closed
forms (DBSDE_EXACT_BARRIER_CALL 15, _PUT 16) at the C boundary, without a GPU:
the kind rides on the existing struct (the barrier level in h_kappa) and the
existing entry points -- no new symbol, ABI version 3, the same struct size, the
header's literal-value lists unchanged -- every refusal is DBSDE_EINVAL before
any HIP call at dbsde_create, dbsde_mc_value and dbsde_exact with a message
naming the field, kinds 5, 6, 7, 9, 10 and 12 are still unknown, exact kinds 9,
12 and 13 still refused."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "dbsde.h")


@pytest.fixture(scope="module")
def lib():
    pkg = load_pkg()
    importlib.import_module(pkg.__name__ + ".build_lib").build(verbose=False)
    return pkg._lib.load()


def bar(pkg, **over):
    kw = dict(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=0.0, g="call_mean", strike=1.0, q3=False, barrier=0.9)
    kw.update(over)
    return pkg.ProblemSpec(**kw)


def compiled(tmp_path, expr, fmt="%d", cast="int"):
    """An expression as a C compiler sees it (the header is plain C)."""
    src, exe = tmp_path / "v.c", tmp_path / "v"
    src.write_text(f'#include <stdio.h>\n#include "dbsde.h"\nint main(void) {{ printf("{fmt}\\n", ({cast})({expr})); return 0; }}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    return int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)


def test_the_kind_is_bound_to_the_header_value(tmp_path):
    pkg = load_pkg()
    text = open(HEADER).read()
    hv = {n: int(v) for n, v in re.findall(r"^#define (DBSDE_\w+) (-?\d+)\b", text, flags=re.M)}
    assert compiled(tmp_path, "DBSDE_PROB_BARRIER") == 11 == pkg._lib.PROB_BARRIER
    assert compiled(tmp_path, "DBSDE_PROB_GEO_ASIAN") == 8 and compiled(tmp_path, "DBSDE_PROB_ASIAN") == 4
    assert "DBSDE_PROB_BARRIER" not in hv                                   # an expression, not a literal
    # the literal-value lists: problem kinds 0..3, exact kinds without 9, 12 and 13
    assert sorted(v for n, v in hv.items() if n.startswith("DBSDE_PROB_")) == [0, 1, 2, 3]
    assert sorted(v for n, v in hv.items() if n.startswith("DBSDE_EXACT_")) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 14, 15, 16]
    assert hv["DBSDE_EXACT_BARRIER_CALL"] == 15 == pkg._lib.EXACT_KINDS["barrier_call"]
    assert hv["DBSDE_EXACT_BARRIER_PUT"] == 16 == pkg._lib.EXACT_KINDS["barrier_put"]
    assert hv["DBSDE_ABI_VERSION"] == pkg._lib.ABI_VERSION == 3
    assert len(pkg._lib.EXPORTED) == 32
    assert pkg._lib.PROBLEM_KINDS == {"diag": 0, "heston": 1, "heston2": 2}
    # the struct is the one before the kind: 18 members, pen last, the ctypes mirror of the same size
    assert compiled(tmp_path, "sizeof(dbsde_problem)", "%d", "int") == ctypes.sizeof(pkg._lib.Problem) == 18 * 4
    assert [f[0] for f in pkg._lib.Problem._fields_][-1] == "pen" and len(pkg._lib.Problem._fields_) == 18
    assert "kind BARRIER: h_kappa is the barrier level B" in re.sub(r"\s*\n \*\s*", " ", text)


def test_the_library_exports_the_same_32_symbols(lib):
    pkg = load_pkg()
    out = os.popen(f"nm -D --defined-only {pkg._lib.LIB_PATH}").read()
    names = sorted(set(re.findall(r"\bT (dbsde_\w+)", out)))
    assert names == sorted(pkg._lib.EXPORTED) and len(names) == 32
    assert lib.dbsde_abi_version() == 3


def test_problem_spec_sends_kind_11_and_the_level_in_h_kappa():
    pkg = load_pkg()
    names = list(pkg.ProblemSpec.__dataclass_fields__)
    assert names[-3:] == ["barrier", "penalty", "average"] and pkg.ProblemSpec().barrier == 0.0
    c = bar(pkg, barrier=0.875).to_c()
    assert c.kind == 11 and c.h_kappa == 0.875 and c.h_theta == 0 and c.h_sigma == 0 and c.h_rho == 0 and c.pen == 0
    plain = bar(pkg, barrier=0.0).to_c()
    assert plain.kind == 0 and plain.h_kappa == 0.0
    assert pkg.ProblemSpec(kind="heston", kappa=2.0).to_c().h_kappa == 2.0
    for over, word in ((dict(kind="heston"), "Heston"), (dict(average=True, g_cols=1), "Asian"),
                       (dict(kappa=1.0), "h_kappa"), (dict(rho=0.5), "Heston coefficients")):
        with pytest.raises(ValueError, match=word):
            bar(pkg, **over).to_c()


def _create(pkg, lib, layers, prob, mode="Naisnet"):
    cfg = pkg._lib.Config()
    cfg.mode, cfg.activation, cfg.n_layers = pkg._lib.MODES[mode], 0, len(layers)
    for k, v in enumerate(layers):
        cfg.layers[k] = v
    cfg.problem = prob
    cfg.T = 1.0
    ctx = ctypes.c_void_p()
    rc = lib.dbsde_create(ctypes.byref(cfg), ctypes.byref(ctx))
    return rc, ctx, lib.dbsde_last_error(None)


def _refusals(pkg):
    """(problem, word of the message): every refusal the header lists."""
    out = []
    for B in (-0.5, float("nan"), float("inf")):
        out.append((bar(pkg, barrier=B).to_c(), b"h_kappa"))
    zero = bar(pkg).to_c()
    zero.h_kappa = 0.0
    out.append((zero, b"h_kappa"))
    out.append((bar(pkg, g="call_mean", strike=1.0, barrier=1.01).to_c(), b"<= strike"))
    out.append((bar(pkg, g="call_sum", strike=3.0, barrier=3.5).to_c(), b"<= strike"))
    out.append((bar(pkg, g="put_mean", strike=1.0, barrier=0.99).to_c(), b">= strike"))
    out.append((bar(pkg, g="put_sum", strike=3.0, barrier=2.5).to_c(), b">= strike"))
    for g in ("sumsq", "log", "smooth_call", "smooth_put"):
        out.append((bar(pkg, g=g, g_alpha=10.0, barrier=1.0).to_c(), b"g_kind"))
    pen = bar(pkg).to_c()
    pen.pen = 10.0
    out.append((pen, b"pen"))
    out.append((bar(pkg, q3=True).to_c(), b"q3"))
    out.append((bar(pkg, u_clamp=True).to_c(), b"u_clamp"))
    for field in ("h_theta", "h_sigma", "h_rho"):
        p = bar(pkg).to_c()
        setattr(p, field, 0.25)
        out.append((p, field.encode()))
    return out


UNKNOWN_KINDS = (5, 6, 7, 9, 10, 12, -1)


def test_create_refuses_before_any_hip_call(lib):
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    lay = [4, 16, 16, 16, 16, 1]
    for prob, word in _refusals(pkg):
        rc, ctx, msg = _create(pkg, lib, lay, prob)
        assert rc == E and not ctx.value and word in msg, (word, rc, msg)
    for kind in UNKNOWN_KINDS:
        prob = bar(pkg).to_c()
        prob.kind = kind
        rc, ctx, msg = _create(pkg, lib, lay, prob)
        assert rc == E and not ctx.value and b"unknown problem kind" in msg, kind
    # the regular barriers at the strike itself, both directions, get past every argument check: with a device the
    # context is created (DIAG's Brownian dimension), without one it stops at the first HIP call
    for over in (dict(), dict(barrier=1.0), dict(g="put_sum", strike=3.0, barrier=3.0), dict(g="call_sum", strike=3.0, barrier=2.0)):
        rc, ctx, msg = _create(pkg, lib, lay, bar(pkg, **over).to_c())
        if torch.cuda.is_available():
            assert rc == pkg._lib.DBSDE_OK and ctx.value, (over, msg)
            assert lib.dbsde_brownian_dim(ctx) == 3
            lib.dbsde_destroy(ctx)
        else:
            assert rc == pkg._lib.DBSDE_EHIP and not ctx.value, (over, rc, msg)


def _mc(lib, prob, D=3, L=None, delta=None, t=1, x=1, value=1):
    """Pointers are never dereferenced on the refused paths: 1 stands for 'not NULL'."""
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    return lib.dbsde_mc_value(ctypes.byref(prob), D, 1.0, vp(L), vp(t), vp(x), 1, 4, 16, 0, 0, vp(value), None, vp(delta),
                              None)


def test_mc_value_refuses_before_any_hip_call(lib):
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    for prob, word in _refusals(pkg):
        assert _mc(lib, prob) == E and word in lib.dbsde_last_error(None), (word, lib.dbsde_last_error(None))
    assert _mc(lib, bar(pkg).to_c(), delta=1) == E
    assert b"bump and reprice" in lib.dbsde_last_error(None)
    assert _mc(lib, bar(pkg).to_c(), D=129) == E
    assert b"128" in lib.dbsde_last_error(None)
    assert _mc(lib, bar(pkg).to_c(), D=129, L=1) == E
    assert b"128" in lib.dbsde_last_error(None)
    assert _mc(lib, bar(pkg, phi_zz=1.0).to_c()) == E
    assert b"phi_zz" in lib.dbsde_last_error(None)
    for kind in UNKNOWN_KINDS:
        prob = bar(pkg).to_c()
        prob.kind = kind
        assert _mc(lib, prob) == E and b"unknown problem kind" in lib.dbsde_last_error(None)
    if not torch.cuda.is_available():          # past the argument checks: the call stops at its first HIP call
        assert _mc(lib, bar(pkg).to_c(), D=128, t=4096, x=4096, value=4096) != E
        assert _mc(lib, bar(pkg).to_c(), D=128, L=4096, t=4096, x=4096, value=4096) != E


def test_exact_kinds(lib):
    """15 and 16 are known: they refuse NULL, R < 1, misaligned pointers and bad
    parameters before any launch and pass the argument checks otherwise (without
    a device the call stops at the launch); 9, 12 and 13 stay refused."""
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    gpu = torch.cuda.is_available()
    one, al = ctypes.c_void_p(1), ctypes.c_void_p(4096)
    good = {15: (0.05, 0.2, 1.0, 0.1, 0.9, 50.0), 16: (0.05, 0.2, 1.0, 0.1, 1.1, 0.0)}
    for kind in (9, 12, 13, 17, -1):
        assert lib.dbsde_exact(kind, al, al, 1, 2, 1.0, (ctypes.c_double * 6)(*good[15]), al, al, None) == E, kind
    for kind in (15, 16):
        p = (ctypes.c_double * 6)(*good[kind])
        for badp in range(4):
            ptrs = [one if k == badp else al for k in range(4)]
            assert lib.dbsde_exact(kind, ptrs[0], ptrs[1], 1, 2, 1.0, p, ptrs[2], ptrs[3], None) == E, (kind, badp)
        assert lib.dbsde_exact(kind, None, al, 1, 2, 1.0, p, al, al, None) == E
        assert lib.dbsde_exact(kind, al, al, 1, 2, 1.0, None, al, al, None) == E
        assert lib.dbsde_exact(kind, al, al, 0, 2, 1.0, p, al, al, None) == E
        nan, inf = float("nan"), float("inf")
        wrong_side = 1.1 if kind == 15 else 0.9
        for i, v, word in ((0, nan, b"r and b"), (3, inf, b"r and b"), (1, 0.0, b"sigma"), (1, nan, b"sigma"), (2, -1.0, b"K"),
                           (4, 0.0, b"B must be > 0"), (4, nan, b"B must be > 0"), (4, wrong_side, b"needs B"),
                           (5, -1.0, b"n_mon"), (5, nan, b"n_mon")):
            q = list(good[kind])
            q[i] = v
            assert lib.dbsde_exact(kind, al, al, 1, 2, 1.0, (ctypes.c_double * 6)(*q), al, al, None) == E, (kind, i, v)
            assert word in lib.dbsde_last_error(None), (kind, i, v, lib.dbsde_last_error(None))
        if gpu:
            t, x = torch.zeros(1, device="cuda:0"), torch.tensor([1.0, 1.05], device="cuda:0")
            out, dl = torch.empty(2, device="cuda:0"), torch.empty(2, device="cuda:0")
            vp = lambda v: ctypes.c_void_p(v.data_ptr())
            assert lib.dbsde_exact(kind, vp(t), vp(x), 1, 2, 1.0, p, vp(out), vp(dl), None) == pkg._lib.DBSDE_OK
            assert lib.dbsde_exact(kind, vp(t), vp(x), 1, 2, 1.0, p, vp(out), None, None) == pkg._lib.DBSDE_OK
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dl).all())
        else:
            rc = lib.dbsde_exact(kind, al, al, 1, 2, 1.0, p, al, al, None)
            assert rc != E and rc != pkg._lib.DBSDE_OK, (kind, rc)


def test_python_checks_that_need_no_device():
    pkg = load_pkg()
    with pytest.raises(ValueError, match="bump and reprice"):
        pkg.mc_value(bar(pkg), torch.zeros(1), torch.ones(1, 3), 1.0, 4, delta=True)
    with pytest.raises(ValueError, match=r"params = \(r, sigma, K, b, B, n_mon\)"):
        pkg.exact("barrier_call", torch.zeros(1), torch.ones(1, 1), 1.0, (0.05, 0.2, 1.0))
    assert {"BarrierCallOption", "BarrierPutOption", "BarrierBasketCallOption", "BarrierBasketPutOption"} <= set(pkg.__all__)
    for name, base in (("BarrierCallOption", pkg.CallOption), ("BarrierPutOption", pkg.PutOption),
                       ("BarrierBasketCallOption", pkg.BasketCallOption), ("BarrierBasketPutOption", pkg.BasketPutOption)):
        assert issubclass(getattr(pkg, name), base)
        assert not hasattr(getattr(pkg, name), "mc_greeks")
