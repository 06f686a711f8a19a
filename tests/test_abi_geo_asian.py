"""The geometric-average Asian problem (problem kind 8, DBSDE_PROB_GEO_ASIAN)
and its closed forms (DBSDE_EXACT_GEO_ASIAN 10, _PUT 11) at the C boundary,
without a GPU: the new values ride on the existing entry points (no new symbol,
ABI version 3, PROBLEM_KINDS unchanged), every refusal is DBSDE_EINVAL before
any HIP call at dbsde_create, dbsde_mc_value and dbsde_exact, kinds 5 to 7 and
9 and above are still unknown, exact kind 9 is still refused."""
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


def geo(pkg, **over):
    kw = dict(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=0.0, g="call_mean", strike=1.0, g_alpha=10.0, g_cols=1, q3=False,
              average="geometric")
    kw.update(over)
    return pkg.ProblemSpec(**kw)


def compiled_value(tmp_path, macro):
    """The macro as a C compiler sees it (the header is plain C)."""
    src, exe = tmp_path / "v.c", tmp_path / "v"
    src.write_text(f'#include <stdio.h>\n#include "dbsde.h"\nint main(void) {{ printf("%d\\n", (int)({macro})); return 0; }}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    return int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)


def test_the_kind_is_bound_to_the_header_value(tmp_path):
    pkg = load_pkg()
    hv = {n: int(v) for n, v in re.findall(r"^#define (DBSDE_\w+) (-?\d+)\b", open(HEADER).read(), flags=re.M)}
    assert compiled_value(tmp_path, "DBSDE_PROB_GEO_ASIAN") == 8 == pkg._lib.PROB_GEO_ASIAN
    assert compiled_value(tmp_path, "DBSDE_PROB_ASIAN") == 4 == pkg._lib.PROB_ASIAN
    assert hv["DBSDE_EXACT_GEO_ASIAN"] == 10 == pkg._lib.EXACT_KINDS["geo_asian"]
    assert hv["DBSDE_EXACT_GEO_ASIAN_PUT"] == 11 == pkg._lib.EXACT_KINDS["geo_asian_put"]
    assert 9 not in [v for n, v in hv.items() if n.startswith("DBSDE_EXACT_")]
    assert hv["DBSDE_ABI_VERSION"] == pkg._lib.ABI_VERSION == 3
    assert len(pkg._lib.EXPORTED) == 32
    assert pkg._lib.PROBLEM_KINDS == {"diag": 0, "heston": 1, "heston2": 2}
    assert [hv[n] for n in ("DBSDE_PROB_DIAG", "DBSDE_PROB_HESTON", "DBSDE_PROB_HESTON2", "DBSDE_PROB_HESTON_CORR")] \
        == [0, 1, 2, 3]
    assert "DBSDE_PROB_GEO_ASIAN" not in hv                                  # an expression, not a literal
    assert geo(pkg).to_c().kind == 8
    sp = pkg.ProblemSpec()
    assert sp.average is False and list(sp.__dataclass_fields__)[-1] == "average" and sp.to_c().kind == 0


def test_the_library_exports_the_same_32_symbols(lib):
    pkg = load_pkg()
    out = os.popen(f"nm -D --defined-only {pkg._lib.LIB_PATH}").read()
    names = sorted(set(re.findall(r"\bT (dbsde_\w+)", out)))
    assert names == sorted(pkg._lib.EXPORTED) and len(names) == 32
    assert lib.dbsde_abi_version() == 3


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


REFUSALS = [(dict(phi_c=1.0), b"phi_c"), (dict(g_cols=0), b"g_cols"), (dict(g_cols=2), b"g_cols"),
            (dict(g="sumsq"), b"sumsq"), (dict(g="log"), b"sumsq"), (dict(sig_b=0.1), b"sig_b"),
            (dict(sig_b=-1e-3), b"sig_b")]
UNKNOWN_KINDS = (5, 6, 7, 9, 10, 12, -1)


def test_create_refuses_before_any_hip_call(lib):
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    lay = [5, 16, 16, 16, 16, 1]                                  # D = 4: [G, S_1..S_3]
    for over, word in REFUSALS:
        rc, ctx, msg = _create(pkg, lib, lay, geo(pkg, **over).to_c())
        assert rc == E and not ctx.value and word in msg, (over, rc, msg)
    rc, ctx, msg = _create(pkg, lib, [2, 16, 16, 16, 16, 1], geo(pkg).to_c())      # D = 1: no asset
    assert rc == E and not ctx.value and b"D must be >= 2" in msg
    for kind in UNKNOWN_KINDS:
        prob = geo(pkg).to_c()
        prob.kind = kind
        rc, ctx, msg = _create(pkg, lib, lay, prob)
        assert rc == E and not ctx.value and b"unknown problem kind" in msg, kind
    # the accepted problem gets past every argument check: with a device it is created, without one it
    # stops at the first HIP call
    rc, ctx, msg = _create(pkg, lib, lay, geo(pkg, q3=True).to_c())                 # q3 is ignored
    if torch.cuda.is_available():
        assert rc == pkg._lib.DBSDE_OK and ctx.value
        assert lib.dbsde_brownian_dim(ctx) == 3
        lib.dbsde_destroy(ctx)
    else:
        assert rc == pkg._lib.DBSDE_EHIP and not ctx.value, (rc, msg)


def _mc(lib, prob, D=4, L=None, delta=None, t=1, x=1, value=1):
    """Pointers are never dereferenced on the refused paths: 1 stands for 'not NULL'."""
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    return lib.dbsde_mc_value(ctypes.byref(prob), D, 1.0, vp(L), vp(t), vp(x), 1, 4, 16, 0, 0, vp(value), None, vp(delta),
                              None)


def test_mc_value_refuses_before_any_hip_call(lib):
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    for over, word in REFUSALS:
        assert _mc(lib, geo(pkg, **over).to_c()) == E, over
        assert word in lib.dbsde_last_error(None), (over, lib.dbsde_last_error(None))
    assert _mc(lib, geo(pkg).to_c(), D=1) == E
    assert b"D must be >= 2" in lib.dbsde_last_error(None)
    assert _mc(lib, geo(pkg).to_c(), D=130, L=1) == E                  # 129 assets under a factor
    assert b"128" in lib.dbsde_last_error(None)
    assert _mc(lib, geo(pkg, phi_zz=1.0).to_c()) == E
    assert b"phi_zz" in lib.dbsde_last_error(None)
    for kind in UNKNOWN_KINDS:
        prob = geo(pkg).to_c()
        prob.kind = kind
        assert _mc(lib, prob) == E and b"unknown problem kind" in lib.dbsde_last_error(None)
    # the arithmetic kind still takes sig_b != 0: past the argument checks (without a device the call stops
    # at its first HIP call and never reads its pointers; with one tests/test_gpu_asian.py runs it)
    arith = geo(pkg, average=True, sig_b=0.1).to_c()
    assert arith.kind == 4
    if not torch.cuda.is_available():
        assert _mc(lib, arith, t=4096, x=4096, value=4096) != E


def test_mc_value_accepts_the_kind(lib):
    """Past the argument checks: without a device the call stops at its first
    HIP call and never reads its pointers; with one it runs on one-point
    buffers (with and without delta)."""
    pkg = load_pkg()
    gpu = torch.cuda.is_available()
    if gpu:
        t, x = torch.zeros(1, device="cuda:0"), torch.tensor([1.0, 1.0, 1.1, 0.9], device="cuda:0")
        out, dl = torch.empty(1, device="cuda:0"), torch.empty(4, device="cuda:0")
        tp, xp, op, dp = (v.data_ptr() for v in (t, x, out, dl))
    else:
        tp = xp = op = dp = 4096
    for g in ("call_sum", "call_mean", "smooth_call", "put_sum", "put_mean", "smooth_put"):
        for delta in (None, dp):
            rc = _mc(lib, geo(pkg, g=g).to_c(), t=tp, x=xp, value=op, delta=delta)
            assert rc != pkg._lib.DBSDE_EINVAL and (rc == pkg._lib.DBSDE_OK) == gpu, (g, rc, lib.dbsde_last_error(None))
    if gpu:
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dl).all())


def test_exact_kinds(lib):
    """Kind 9 is refused with aligned pointers; 10 and 11 refuse NULL, R < 1,
    D < 2 and misaligned pointers before any launch, and pass the argument
    checks otherwise (without a device the call stops at the launch)."""
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    gpu = torch.cuda.is_available()
    one, al = ctypes.c_void_p(1), ctypes.c_void_p(4096)
    p = (ctypes.c_double * 6)(0.05, 0.05, 0.2, 1.0, 1.0, 1.0 / 3)
    assert lib.dbsde_exact(9, al, al, 1, 4, 1.0, p, al, al, None) == E
    for kind in (12, 13, -1):
        assert lib.dbsde_exact(kind, al, al, 1, 4, 1.0, p, al, al, None) == E
    for kind in (10, 11):
        for bad in range(4):
            ptrs = [one if k == bad else al for k in range(4)]
            assert lib.dbsde_exact(kind, ptrs[0], ptrs[1], 1, 4, 1.0, p, ptrs[2], ptrs[3], None) == E, (kind, bad)
        assert lib.dbsde_exact(kind, al, al, 1, 4, 1.0, ctypes.c_void_p(4100), al, al, None) == E      # params: doubles
        assert lib.dbsde_exact(kind, None, al, 1, 4, 1.0, p, al, al, None) == E
        assert lib.dbsde_exact(kind, al, al, 1, 4, 1.0, None, al, al, None) == E
        assert lib.dbsde_exact(kind, al, al, 0, 4, 1.0, p, al, al, None) == E
        assert lib.dbsde_exact(kind, al, al, 1, 1, 1.0, p, al, al, None) == E                         # no asset
        if gpu:
            t, x = torch.zeros(1, device="cuda:0"), torch.tensor([1.0, 1.0, 1.1, 0.9], device="cuda:0")
            out, dl = torch.empty(1, device="cuda:0"), torch.empty(4, device="cuda:0")
            vp = lambda v: ctypes.c_void_p(v.data_ptr())
            assert lib.dbsde_exact(kind, vp(t), vp(x), 1, 4, 1.0, p, vp(out), vp(dl), None) == pkg._lib.DBSDE_OK
            assert lib.dbsde_exact(kind, vp(t), vp(x), 1, 4, 1.0, p, vp(out), None, None) == pkg._lib.DBSDE_OK
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dl).all())
        else:
            rc = lib.dbsde_exact(kind, al, al, 1, 4, 1.0, p, al, al, None)
            assert rc != E and rc != pkg._lib.DBSDE_OK, (kind, rc)


def test_python_checks_that_need_no_device():
    pkg = load_pkg()
    with pytest.raises(ValueError, match="Heston"):
        pkg.ProblemSpec(kind="heston2", average="geometric").to_c()
    with pytest.raises(ValueError, match="unknown average"):
        pkg.ProblemSpec(average="geo").to_c()
    with pytest.raises(ValueError, match=r"L must be \[3, 3\]"):
        pkg.mc_value(geo(pkg), torch.zeros(1), torch.ones(1, 4), 1.0, 4, L=[[1.0, 0.0], [0.0, 1.0]])
    with pytest.raises(ValueError, match="unknown exact"):
        pkg.exact("geo", None, None, 1.0, ())
