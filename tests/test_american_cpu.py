"""The penalised American put without a GPU: the cotangent formulas the
kernels implement against autograd, the conditions on the inputs of
tests/test_gpu_american.py (checked on the fp64 oracle alone), the numpy tree
against known values, and the C boundary (dbsde_problem.pen, exact kind 14):
layouts, and every refusal DBSDE_EINVAL with its word before any HIP call."""
import ctypes
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import american_reference as ar
import put_reference as pr
from conftest import ROOT, load_pkg
from oracle import fbsnn_ref as fr

HEADER = os.path.join(ROOT, "include", "dbsde.h")


@pytest.fixture(scope="module")
def lib():
    pkg = load_pkg()
    importlib.import_module(pkg.__name__ + ".build_lib").build(verbose=False)
    return pkg._lib.load()


# ------------------------------------------------------------------ the formulas
@pytest.mark.parametrize("payoff,base", [("put_sum", "call"), ("put_mean", "basket")])
def test_hand_written_cotangents_equal_autograd(payoff, base):
    """One small FC network in fp64, D = 4, M = 20, N = 3, penalty 100: the
    gradient from residual rows, ubar with (1 + (phi_r + pen 1[g > Y]) dt) and
    the unchanged zbar (ar.hand_gradient) equals autograd of the oracle's loss of
    AmericanProblem to 1e-12 of the largest gradient entry; both branches occur."""
    D = 4
    torch.manual_seed(3)
    model = fr.build_model("FC", [D + 1, 16, 16, 16, 1], "Tanh").double()
    t, W = fr.fetch_minibatch(ar.M, ar.N, D, ar.T, rng=np.random.RandomState(7), dtype=torch.float64)
    Xi = torch.ones((1, D), dtype=torch.float64)
    prob = ar.AmericanProblem(base, D, payoff, pr.strike_of(payoff, D))
    # the output bias moves every Y alike: put the median interior row on the exercise boundary
    out_bias = ar.output_bias(model)
    with torch.no_grad():
        out_bias.fill_(0.0)
    r0 = fr.loss_and_grads(model, prob, t, W, Xi, ar.M, D)
    gap = ar.payoff_np(payoff, prob.strike, r0["X"][:, :-1, :]) - r0["Y"][:, :-1, 0]
    with torch.no_grad():
        out_bias.fill_(round(float(np.median(gap)), 2))
    params = list(model.parameters())
    loss = fr.loss_function(model, prob, t, W, Xi.clone().requires_grad_(True), ar.M, D)[0]
    auto = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, params)]).numpy()
    hl, hand = ar.hand_gradient(model, prob, pr.COEF[base], t, W, Xi, ar.M)
    marg, ind = ar.margins(dict(ref64=fr.loss_and_grads(model, prob, t, W, Xi, ar.M, D), problem=prob))
    print(f"{payoff}: exercise rows {ind.mean():.2f}, smallest margin {marg.min():.2e}, "
          f"max |hand - autograd| / max |autograd| = {np.abs(hand - auto).max() / np.abs(auto).max():.2e}")
    assert 0.1 < ind.mean() < 0.9                      # both branches of the indicator occur
    assert abs(hl - float(loss)) <= 1e-12 * abs(float(loss))
    assert np.abs(hand - auto).max() <= 1e-12 * np.abs(auto).max()


# ------------------------------------------------------------------ conditions on the GPU tests' inputs
@pytest.mark.parametrize("site,payoff", ar.RUNS, ids=[f"{s}-{p}" for s, p in ar.RUNS])
def test_gpu_inputs_sit_away_from_the_exercise_boundary(site, payoff):
    """penalty 100 and the case's strike: every interior row's margin
    |g(X) - Y| / (1 + |Y|) is >= 1e-3, and each branch of the indicator holds at
    least 20 % of the interior rows; no row is left out."""
    b = ar.reference(site, payoff)
    marg, ind = ar.margins(b)
    assert marg.shape == (ar.M, ar.N) == ind.shape
    print(f"{site} {payoff}: K = {ar.strike_of(site, payoff)}, bias {ar.case_of(site, payoff)[1]}, "
          f"smallest margin {marg.min():.3e}, in exercise {ind.mean():.3f}")
    assert marg.min() >= ar.MARGIN_MIN
    assert ar.BRANCH_MIN <= ind.mean() <= 1.0 - ar.BRANCH_MIN
    # the fp32 oracle decides every row the same way
    Y32, X32 = b["ref32"]["Y"][:, :-1, 0], b["ref32"]["X"][:, :-1, :]
    assert np.array_equal(ar.payoff_np(payoff, ar.strike_of(site, payoff), X32) > Y32, ind)


def test_plugin_case_sits_away_from_the_exercise_boundary():
    marg, ind = ar.margins(ar.plugin_reference())
    print(f"plugin case: smallest margin {marg.min():.3e}, in exercise {ind.mean():.3f}")
    assert marg.min() >= ar.MARGIN_MIN and ar.BRANCH_MIN <= ind.mean() <= 1.0 - ar.BRANCH_MIN


# ------------------------------------------------------------------ the numpy tree
def test_crr_european_tree_converges_to_black_scholes():
    """pen = 0 is the European tree.  Its distance from the closed form is the
    tree's own O(1 / n) error: at n and at 2 n it stays below K sigma sqrt(tau) /
    n (the size of one node spacing's worth of payoff, spread over n steps),
    and the two trees differ by no more than the sum of those bounds."""
    for S, K, r, sig, b, tau in [(36.0, 40.0, 0.06, 0.2, 0.06, 1.0), (1.0, 1.0, 0.05, 0.2, 0.10, 1.0),
                                 (1.1, 1.0, 0.05, 0.2, 0.05, 0.3)]:
        bs = ar.bs_put_carry(S, K, r, sig, b, tau)
        for n in (500, 1000):
            e = abs(ar.crr(S, K, r, sig, b, tau, n, 0.0)[0] - bs)
            bound = K * sig * np.sqrt(tau) / n
            print(f"S {S} K {K} n {n}: |tree - closed form| {e:.2e}, bound {bound:.2e}")
            assert e <= bound


def test_crr_american_value_and_monotonicity():
    v, d = ar.crr(36.0, 40.0, 0.06, 0.2, 0.06, 1.0, 2000, math.inf)
    print(f"American put S = 36, K = 40: {v:.5f}, delta {d:.5f}")
    assert abs(v - 4.4867) <= 1e-3 and -1.0 <= d <= 0.0
    # the issue's table: K = 1, r = b = 0.05, sigma = 0.2, T = 1, S = 1 on 2000 steps
    tab = {0.0: 0.05573, 10.0: 0.05989, 100.0: 0.06078, 1000.0: 0.06089, math.inf: 0.06090}
    vals = {pen: ar.crr(1.0, 1.0, 0.05, 0.2, 0.05, 1.0, 2000, pen)[0] for pen in tab}
    print("penalised values", vals)
    for pen, want in tab.items():
        assert abs(vals[pen] - want) <= 1.5e-5, (pen, vals[pen])
    for S in (0.8, 0.9, 1.0, 1.1, 1.2):
        vs = [ar.crr(S, 1.0, 0.05, 0.2, 0.05, 1.0, 400, pen)[0] for pen in (0.0, 1.0, 10.0, 100.0, 1000.0, math.inf)]
        assert all(a <= b_ + 1e-15 for a, b_ in zip(vs, vs[1:])), (S, vs)      # monotone in pen
        assert vs[-1] >= max(1.0 - S, 0.0) - 1e-15                              # >= the payoff
        assert all(v_ >= vs[0] - 1e-15 for v_ in vs)                            # >= the European value
    assert ar.crr(0.9, 1.0, 0.05, 0.2, 0.05, 0.0, 10, math.inf) == (pytest.approx(0.1), -1.0)
    assert ar.crr(1.0, 1.0, 0.05, 0.2, 0.05, 0.0, 10, 5.0) == (0.0, -0.5)
    assert ar.crr(1.1, 1.0, 0.05, 0.2, 0.05, -0.1, 10, 5.0) == (0.0, 0.0)


# ------------------------------------------------------------------ ABI
def test_pen_is_the_last_member_and_layouts_agree(tmp_path):
    pkg = load_pkg()
    L = pkg._lib
    assert L.Problem._fields_[-1] == ("pen", ctypes.c_float) and len(L.Problem._fields_) == 18
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dbsde.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %d\\n", sizeof(dbsde_problem), offsetof(dbsde_problem, pen), '
                   'offsetof(dbsde_problem, h_rho), sizeof(dbsde_config), offsetof(dbsde_config, T), '
                   'DBSDE_EXACT_AMERICAN_PUT);\n  return 0;\n}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    size, off_pen, off_rho, csize, off_T, kind = (int(v) for v in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == ctypes.sizeof(L.Problem) and off_pen == L.Problem.pen.offset == size - 4
    assert off_rho == L.Problem.h_rho.offset == off_pen - 4
    assert csize == ctypes.sizeof(L.Config) and off_T == L.Config.T.offset
    assert kind == 14 == L.EXACT_KINDS["american_put"]
    assert L.ABI_VERSION == 3 and len(L.EXPORTED) == 32
    # the 17 members before pen, positionally: pen = 0
    p17 = L.Problem(0, 0.05, 0.2, 0.0, 0.05, 1.0, 0.0, 5, 1.0, 0, 0, 0.0, 0, 0.0, 0.0, 0.0, 0.0)
    assert p17.pen == 0.0
    fields = list(pkg.ProblemSpec.__dataclass_fields__)
    assert fields[-1] == "average" and fields[-2] == "penalty" and pkg.ProblemSpec().penalty == 0.0
    assert pkg.ProblemSpec().to_c().pen == 0.0
    assert pkg.ProblemSpec(g="put_sum", penalty=100.0).to_c().pen == 100.0


def put(pkg, **over):
    kw = dict(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=1.0, g="put_sum", strike=4.0, penalty=100.0)
    kw.update(over)
    return pkg.ProblemSpec(**kw)


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


def test_create_refuses_before_any_hip_call(lib):
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    lay = [5, 16, 16, 16, 16, 1]

    def raw(pen, **fields):
        prob = put(pkg, penalty=0.0).to_c()
        prob.pen = pen
        for k, v in fields.items():
            setattr(prob, k, v)
        return prob

    asian = pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, g="put_mean", strike=1.0, g_cols=1, q3=False, average=True).to_c()
    geo = pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, g="put_mean", strike=1.0, g_cols=1, q3=False,
                          average="geometric").to_c()
    asian.pen = geo.pen = 100.0
    bad = [raw(-1.0), raw(float("nan")), raw(float("inf")), raw(-float("inf")), raw(100.0, u_clamp=1),
           raw(100.0, kind=1, g_kind=6, g_cols=2), raw(100.0, kind=2, g_kind=6, g_cols=2), asian, geo]
    for prob in bad:
        rc, ctx, msg = _create(pkg, lib, lay, prob)
        assert rc == E and not ctx.value and b"pen" in msg, (prob.kind, prob.pen, rc, msg)
    # accepted: DIAG with any g_kind, with q3: past every argument check (without a device the call stops at
    # its first HIP call)
    for g_kind in range(8):
        rc, ctx, msg = _create(pkg, lib, lay, raw(100.0, g_kind=g_kind, q3=1))
        if torch.cuda.is_available():
            assert rc == pkg._lib.DBSDE_OK and ctx.value, msg
            lib.dbsde_destroy(ctx)
        else:
            assert rc == pkg._lib.DBSDE_EHIP and not ctx.value, (g_kind, rc, msg)


def test_mc_value_refuses_the_penalised_problem(lib):
    pkg = load_pkg()
    vp = ctypes.c_void_p
    prob = put(pkg).to_c()
    rc = lib.dbsde_mc_value(ctypes.byref(prob), 4, 1.0, None, vp(4096), vp(4096), 1, 4, 16, 0, 0, vp(4096), None, None, None)
    msg = lib.dbsde_last_error(None)
    assert rc == pkg._lib.DBSDE_EINVAL and b"pen" in msg and b"not a linear" in msg and b"DBSDE_EXACT_AMERICAN_PUT" in msg
    with pytest.raises(ValueError, match="DBSDE_EXACT_AMERICAN_PUT"):
        pkg.mc_value(put(pkg), torch.zeros(1), torch.ones(1, 4), 1.0, 4)


def test_exact_kind_14(lib):
    """Kinds 9, 12, 13 and -1 stay refused; kind 14 refuses NULL and misaligned
    pointers, R or D < 1, sigma or K <= 0, pen negative or NaN and n_tree outside
    [2, 4096] or fractional, each before any launch; good arguments get past
    the checks (without a device the call stops at the launch)."""
    pkg = load_pkg()
    E = pkg._lib.DBSDE_EINVAL
    one, al = ctypes.c_void_p(1), ctypes.c_void_p(4096)
    P = lambda *v: (ctypes.c_double * 6)(*v)
    good = P(0.05, 0.2, 1.0, 0.05, 100.0, math.inf)
    for kind in (9, 12, 13, -1):
        assert lib.dbsde_exact(kind, al, al, 1, 2, 1.0, good, al, al, None) == E
    call = lambda p, t=al, x=al, R=1, D=2, price=al, delta=al: lib.dbsde_exact(14, t, x, R, D, 1.0, p, price, delta, None)
    for bad in ("t", "x", "price", "delta"):
        assert call(good, **{bad: one}) == E, bad
    assert call(ctypes.c_void_p(4100)) == E and call(None) == E
    assert call(good, t=None) == E and call(good, x=None) == E and call(good, price=None) == E
    assert call(good, R=0) == E and call(good, D=0) == E
    words = [(P(0.05, 0.0, 1.0, 0.05, 100.0, 0.0), b"sigma"), (P(0.05, -0.2, 1.0, 0.05, 100.0, 0.0), b"sigma"),
             (P(0.05, 0.2, 0.0, 0.05, 100.0, 0.0), b"K"), (P(0.05, 0.2, -1.0, 0.05, 100.0, 0.0), b"K"),
             (P(0.05, 0.2, 1.0, 0.05, 100.0, -1.0), b"pen"), (P(0.05, 0.2, 1.0, 0.05, 100.0, math.nan), b"pen"),
             (P(0.05, 0.2, 1.0, 0.05, 1.0, 0.0), b"n_tree"), (P(0.05, 0.2, 1.0, 0.05, 4097.0, 0.0), b"n_tree"),
             (P(0.05, 0.2, 1.0, 0.05, 100.5, 0.0), b"n_tree"), (P(0.05, 0.2, 1.0, 0.05, math.nan, 0.0), b"n_tree")]
    for p, word in words:
        assert call(p) == E and word in lib.dbsde_last_error(None), (list(p), lib.dbsde_last_error(None))
    if not torch.cuda.is_available():
        for p in (good, P(0.05, 0.2, 1.0, 0.1, 2.0, 0.0), P(0.05, 0.2, 1.0, 0.05, 4096.0, 100.0)):
            rc = call(p)
            assert rc != E and rc != pkg._lib.DBSDE_OK, (list(p), rc)
            assert call(p, delta=None) != E


def test_python_checks_that_need_no_device():
    pkg = load_pkg()
    for kw, word in [(dict(kind="heston", g="put_mean"), "Heston"), (dict(kind="heston2", g="put_mean"), "Heston"),
                     (dict(average=True, g="put_mean", g_cols=1, phi_c=0.0), "Asian"),
                     (dict(average="geometric", g="put_mean", g_cols=1, phi_c=0.0), "Asian"),
                     (dict(u_clamp=True), "u_clamp"), (dict(penalty=-1.0), "penalty"),
                     (dict(penalty=math.inf), "penalty"), (dict(penalty=math.nan), "penalty")]:
        with pytest.raises(ValueError, match=word):
            put(pkg, **kw).to_c()
    with pytest.raises(ValueError, match="r, sigma, K"):
        pkg.exact("american_put", torch.zeros(1), torch.ones(1, 1), 1.0, 0.05, 0.2)
    for bad in (1, 4097, 100.5, math.inf, math.nan):
        with pytest.raises(ValueError, match="n_tree"):
            pkg.exact("american_put", torch.zeros(1), torch.ones(1, 1), 1.0, 0.05, 0.2, 1.0, n_tree=bad)
    for kw in (dict(b=0.1), dict(n_tree=100), dict(penalty=1.0), dict(sigma=0.2), dict(K=1.0)):
        with pytest.raises(ValueError, match="american_put"):
            pkg.exact("bs_put", torch.zeros(1), torch.ones(1, 1), 1.0, (0.05, 0.2, 1.0), **kw)
    with pytest.raises(ValueError, match="same HIP device"):          # params by keyword: past the argument checks
        pkg.exact("bs_put", torch.zeros(1), torch.ones(1, 1), 1.0, params=(0.05, 0.2, 1.0))
    with pytest.raises(ValueError, match="same HIP device"):          # r, sigma, K as one sequence
        pkg.exact("american_put", torch.zeros(1), torch.ones(1, 1), 1.0, (0.05, 0.2, 1.0), n_tree=10)
    assert all(math.isnan(v) for v in ar.crr(1.0, 1.0, 0.05, 0.2, 0.5, 1.0, 2, 0.0))       # p > 1: no tree value
    hv = {n: int(v) for n, v in re.findall(r"^#define (DBSDE_EXACT_\w+) (-?\d+)\b", open(HEADER).read(), flags=re.M)}
    assert hv["DBSDE_EXACT_AMERICAN_PUT"] == 14 and 12 not in hv.values() and 13 not in hv.values()
    assert {"AmericanPutOption", "AmericanBasketPutOption"} <= set(pkg.__all__)
    assert issubclass(pkg.AmericanPutOption, pkg.PutOption) and issubclass(pkg.AmericanBasketPutOption, pkg.BasketPutOption)
    # the probe's formulas carry the penalty term
    gen = importlib.import_module(pkg.__name__ + ".generic")
    f = gen.spec_functions(put(pkg))
    X, Y, Z = torch.full((2, 4), 0.9), torch.tensor([[0.1], [0.7]]), torch.zeros(2, 4)
    want = 0.05 * Y - 100.0 * torch.relu(torch.tensor([[0.4], [0.4]]) - Y)
    assert torch.allclose(f["phi_tf"](None, X, Y, Z), want, rtol=1e-6, atol=1e-6)
