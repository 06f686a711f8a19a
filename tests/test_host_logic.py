"""Host-side logic of the package against the oracle and the reference's
golden vectors (layouts, initialisation, problem coefficients, schedule).  CPU."""
import glob
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_pkg
from oracle import fbsnn_ref as fr
from oracle import timeparallel as tp

G1 = sorted(p for p in glob.glob(os.path.join(GOLDEN, "g1_*.npz")) if "train_" not in p)
MODES = ["FC", "NAIS-Net", "Resnet", "Naisnet"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layers", [[5, 16, 16, 16, 16, 1], [101, 110, 110, 110, 110, 1], [2, 8, 8, 1],
                                    [5, 16, 16, 16, 1]])
def test_param_layout_matches_reference_modules(mode, layers):
    from importlib import import_module
    nets = import_module(load_pkg().__name__ + ".networks")
    m = nets.make_model(mode, layers, "Sine")
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == [(k, tuple(s)) for k, s in tp.param_layout(mode, layers)]
    ref = fr.build_model(mode, layers, "Sine")
    assert [k for k in ref.state_dict()] == [k for k, _ in got]


@pytest.mark.parametrize("path", G1, ids=[os.path.basename(p)[3:-4] for p in G1])
def test_initialisation_reproduces_reference(path):
    """torch.manual_seed(s) + the package's model builder == the reference's
    own construction (the fixture's params were drawn by the reference)."""
    from importlib import import_module
    nets = import_module(load_pkg().__name__ + ".networks")
    z = np.load(path)
    if "rtr_norms" in z.files:
        pytest.skip("Q4 not-taken fixture: weights rescaled after the reference init")
    torch.manual_seed(int(z["seed"]))
    layers = [int(v) for v in z["layers"]]
    if str(z["problem"]) == "heston":      # the reference builds on [D+1, ...] and replaces the input layers
        m = nets.make_heston_model(str(z["mode"]), [2] + layers[1:], str(z["activation"]), layers[0])
    else:
        m = nets.make_model(str(z["mode"]), layers, str(z["activation"]))
    flat = torch.cat([p.reshape(-1) for p in m.state_dict().values()]).numpy()
    np.testing.assert_array_equal(flat, z["params"])


def test_problem_specs_match_oracle_table():
    pkg = load_pkg()
    ns = types.SimpleNamespace(strike=4.0, D=4)
    cases = {"call": pkg.CallOption, "call1d": pkg.CallOption1D, "basket": pkg.BasketCallOption,
             "bspde_test": pkg.BSPDETestCase, "hjb": pkg.HamiltonJacobiBellman, "bsb": pkg.BlackScholesBarenblatt}
    g_map = {"sumsq": "sumsq", "call_sum": "call_sum", "call_mean": "call_mean", "log": "log"}
    for kind, cls in cases.items():
        spec = cls.problem_spec(ns)
        mu_a, sig_a, sig_b, phi_r, phi_c, phi_zz, gk = tp.PROBLEMS[kind]
        assert np.allclose([spec.mu_a, spec.sig_a, spec.sig_b, spec.phi_r, spec.phi_c, spec.phi_zz],
                           [mu_a, sig_a, sig_b, phi_r, phi_c, phi_zz]), kind
        assert g_map[spec.g] == gk, kind


def test_problem_torch_expressions_match_oracle():
    """phi_tf/g_tf/mu_tf/sigma_tf of the package classes == the reference's (via the oracle)."""
    pkg = load_pkg()
    D = 4
    torch.manual_seed(0)
    X, Z, Y, t = torch.rand(3, D) + 0.5, torch.randn(3, D), torch.randn(3, 1), torch.zeros(3, 1)
    for kind, cls in {"call": pkg.CallOption, "basket": pkg.BasketCallOption, "hjb": pkg.HamiltonJacobiBellman,
                      "bsb": pkg.BlackScholesBarenblatt, "bspde_test": pkg.BSPDETestCase}.items():
        ref = fr.make_problem(kind, D)
        self = types.SimpleNamespace(strike=ref.strike, D=D)
        self_cls = type("S", (cls,), {})
        obj = object.__new__(self_cls)
        obj.__dict__.update(self.__dict__)
        assert torch.allclose(obj.phi_tf(t, X, Y, Z), ref.phi(t, X, Y, Z)), kind
        assert torch.allclose(obj.g_tf(X), ref.g(X)), kind
        assert torch.allclose(obj.mu_tf(t, X, Y, Z), ref.mu(t, X, Y, Z)), kind
        assert torch.allclose(obj.sigma_tf(t, X, Y), ref.sigma(t, X, Y)), kind


@pytest.mark.parametrize("schedule,Mm", [("nd", 50 ** (1 / 5)), ("nd", 5.0)])
def test_n_schedule(schedule, Mm):
    pkg = load_pkg()
    obj = object.__new__(pkg.CallOption)
    obj.schedule, obj.Mm, obj.N = schedule, Mm, 50
    for it in (0, 100, 3999, 4000, 8000, 12000, 16000, 19999):
        obj._schedule_n(it)
        assert obj.N == fr.n_schedule(it, Mm, 50), it


def test_corr_schedule_collapses_like_reference():
    """with_corr...:406-409 re-applies N**(1/5) to the mutated N."""
    pkg = load_pkg()
    obj = object.__new__(pkg.BasketCallOption)
    obj.schedule, obj.Mm, obj.N = "corr", 50 ** (1 / 5), 200
    seq = []
    for it in range(4):
        obj._schedule_n(it)
        seq.append(obj.N)
    assert seq == [3, 2, 2, 2]


def test_correlation_matrix_recipe_matches_reference_fixture():
    """generate_correlation_matrix (Q10) reproduces the reference's matrix from
    the same numpy stream (fixture drawn by the reference constructor)."""
    pkg = load_pkg()
    z = np.load(os.path.join(GOLDEN, "g1_corr_basket_Naisnet_ReLU.npz"))
    np.random.seed(int(z["seed"]))
    obj = object.__new__(pkg.BasketCallOption)
    obj.correlation_type = "random_correlation"
    np.testing.assert_allclose(obj.generate_correlation_matrix(4), z["corr"], rtol=0, atol=1e-12)


def test_heston_spec_and_expressions():
    """HestonFBSNN problem spec and torch expressions vs heston_dnnpde.py:546-609
    (via the oracle's restatement, k = 1 and k = 3)."""
    pkg = load_pkg()
    for k, payoff in ((1, "discontinuous"), (3, "continuous")):
        obj = object.__new__(pkg.HestonFBSNN)
        obj.__dict__.update(n_assets=k, strike=1.0, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8, v0=0.2,
                            payoff_type=payoff, device=torch.device("cpu"))
        spec = obj.problem_spec()
        assert spec.kind == "heston" and spec.g_cols == k and spec.u_clamp and not spec.q3
        assert spec.g == ("call_mean" if payoff == "discontinuous" else "smooth_call")
        h = fr.Heston(k=k, payoff=payoff)
        torch.manual_seed(k)
        X = torch.rand(5, 2 * k) + 0.5
        assert torch.allclose(obj.g_tf(X), h.g(X[:, :k]))
        mu = obj.mu_tf(None, X)
        assert torch.allclose(mu[:, :k], 0.05 * X[:, :k]) and torch.allclose(mu[:, k:], 2.0 * (0.2 - X[:, k:]))
        full = obj._full_state(np.ones((1, k)))
        assert full.shape == (1, 2 * k) and torch.all(full[0, k:] == 0.2)


def test_optimizer_defaults_are_torch_defaults():
    """OPT_DEFAULTS mirror optim.X(params, lr=lr) of torch (nd_BSPDE_case.py:331-350)."""
    from importlib import import_module
    fb = import_module(load_pkg().__name__ + ".fbsnn")
    p = [torch.nn.Parameter(torch.zeros(2))]
    for name, kw in fb.OPT_DEFAULTS.items():
        d = getattr(torch.optim, name)(p, lr=1e-3).defaults
        for k, v in kw.items():
            assert d[k] == v, (name, k)


def test_optimizer_names():
    pkg = load_pkg()
    obj = object.__new__(pkg.CallOption)
    with pytest.raises(ValueError):
        obj._check_optimizer("Nadam")
    for name in ("Adam", "SGD", "RMSprop", "AdamW", "Adadelta", "Adagrad", "Adamax", "ASGD", "LBFGS"):
        obj._check_optimizer(name)


class _CpuVecSolver:
    """CPU stand-in for the three native L-BFGS vector primitives (test only):
    the same contracts as dbsde_vec_reduce / dbsde_vec_axpby /
    dbsde_lbfgs_direction, in float64-accumulated torch."""

    def vec_reduce(self, op, a, b=None):
        a64 = a.double()
        if op == "dot":
            return float((a64 * b.double()).sum())
        return float(a64.abs().sum() if op == "asum" else a64.abs().max())

    def vec_axpby(self, z, x, alpha, y=None, beta=0.0):
        v = np.float32(alpha) * x
        z.copy_(v + np.float32(beta) * y if y is not None else v)

    def lbfgs_direction(self, g, S, Y, slots, ro, h_diag, d):
        q = -g.clone()
        al = {}
        for i in range(len(slots) - 1, -1, -1):
            al[i] = np.float32(self.vec_reduce("dot", S[slots[i]], q)) * np.float32(ro[i])
            q = q + (-al[i]) * Y[slots[i]]
        q = q * np.float32(h_diag)
        for i in range(len(slots)):
            be = np.float32(self.vec_reduce("dot", Y[slots[i]], q)) * np.float32(ro[i])
            q = q + (al[i] - be) * S[slots[i]]
        d.copy_(q)


@pytest.mark.parametrize("lr", [1.0, 0.05])
def test_lbfgs_driver_matches_torch_lbfgs(lr):
    """FBSNN._lbfgs_step (torch.optim.LBFGS.step restated over the native
    vector primitives) against torch.optim.LBFGS on a smooth test function:
    three steps, each up to 20 inner iterations with closure re-evaluation
    (nd_BSPDE_case.py:347-348,357-361,380-381)."""
    pkg = load_pkg()
    torch.manual_seed(0)
    n = 40
    A = torch.randn(n, n) / n ** 0.5
    Q = A @ A.T + 0.1 * torch.eye(n)
    c = torch.randn(n)

    def f(x):
        return 0.5 * x @ Q @ x - c @ x + 0.25 * torch.sum(torch.sin(x) ** 2)

    x0 = torch.randn(n)
    ref = x0.clone().requires_grad_(True)
    topt = torch.optim.LBFGS([ref], lr=lr)

    def tclosure():
        topt.zero_grad()
        loss = f(ref)
        loss.backward()
        return loss

    obj = object.__new__(pkg.CallOption)
    obj.device = torch.device("cpu")
    obj.params = x0.clone()
    obj.grad = torch.zeros(n)
    obj.solver = _CpuVecSolver()

    def closure():
        x = obj.params.clone().requires_grad_(True)
        loss = f(x)
        loss.backward()
        obj.grad.copy_(x.grad)
        return float(loss)

    st = obj._lbfgs_state(lr)
    for _ in range(3):
        topt.step(tclosure)
        obj._lbfgs_step(st, closure)
    torch.testing.assert_close(obj.params, ref.detach(), rtol=1e-3, atol=1e-4)
    # the stopping tests compare fp32 scalars against 1e-9 tolerances: the
    # fixed-order fp64 dots may end a converged step one evaluation apart
    assert abs(st["func_evals"] - topt.state[ref]["func_evals"]) <= 2
    assert abs(st["n_iter"] - topt.state[ref]["n_iter"]) <= 2


def test_lbfgs_driver_does_not_take_a_nan_gradient_for_converged():
    """torch tests `flat_grad.abs().max() <= tolerance_grad`, which is False for
    a NaN gradient: LBFGS.step goes on (and evaluates the closure again).
    _lbfgs_step over a vec_reduce whose AMAX propagates NaN (the contract of
    DBSDE_VEC_AMAX, include/dbsde.h) does the same, evaluation for evaluation;
    an AMAX that dropped the NaN (C fmax) would return after the first one."""
    pkg = load_pkg()
    n = 6
    x0 = torch.linspace(-1.0, 1.0, n)

    def f(x):      # sqrt(x_0 - 2) is NaN here: the gradient's first element is NaN, the rest finite
        return torch.sum(x ** 2) + torch.sqrt(x[0] - 2.0) * 0.0

    ref = x0.clone().requires_grad_(True)
    topt = torch.optim.LBFGS([ref], lr=1.0)

    def tclosure():
        topt.zero_grad()
        loss = f(ref)
        loss.backward()
        return loss

    topt.step(tclosure)
    assert topt.state[ref]["func_evals"] > 1

    obj = object.__new__(pkg.CallOption)
    obj.device = torch.device("cpu")
    obj.params = x0.clone()
    obj.grad = torch.zeros(n)
    obj.solver = _CpuVecSolver()
    assert np.isnan(obj.solver.vec_reduce("amax", torch.tensor([1.0, float("nan"), 0.5])))

    def closure():
        x = obj.params.clone().requires_grad_(True)
        loss = f(x)
        loss.backward()
        obj.grad.copy_(x.grad)
        return float(loss)

    st = obj._lbfgs_state(1.0)
    obj._lbfgs_step(st, closure)
    assert torch.isnan(obj.grad).any()
    assert st["func_evals"] == topt.state[ref]["func_evals"] > 1
    assert st["n_iter"] == topt.state[ref]["n_iter"]


def _rne16(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32 (v_cvt_pk_bf16_f32)."""
    u = x.view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)).view(np.float32)


def _split3(x):
    hi = _rne16(x)
    r1 = (x - hi).astype(np.float32)
    mid = _rne16(r1)
    return hi, mid, (r1 - mid).astype(np.float32)


def test_split_bf16_parts_are_exact():
    """The split-bf16 matrix form (csrc/phase.hpp split_two, the pack kernel):
    x = hi + mid + lo holds exactly for fp32 x (hi, mid rounded to nearest
    even, lo the remainder), each part is a bf16 value, and the six kept
    products reproduce the product w x within 2^-24 |w x| -- the fp32 rounding
    bound of the product itself -- with no bias."""
    rs = np.random.RandomState(11)
    n = 400000
    x = (rs.standard_normal(n) * np.exp(rs.uniform(-30, 30, n))).astype(np.float32)
    w = rs.standard_normal(n).astype(np.float32)
    xh, xm, xl = _split3(x)
    wh, wm, wl = _split3(w)
    for p in (xh, xm, xl, wl):   # bf16 values: the low 16 bits are clear
        assert np.all((p.view(np.uint32) & np.uint32(0xFFFF)) == 0)
    np.testing.assert_array_equal(xh.astype(np.float64) + xm + xl, x.astype(np.float64))
    d = np.float64
    six = d(wl) * xh + d(wh) * xl + d(wm) * xm + d(wm) * xh + d(wh) * xm + d(wh) * xh
    exact = d(w) * d(x)
    rel = (six - exact) / np.abs(exact)
    assert np.abs(rel).max() <= 2.0 ** -24
    assert abs(rel.mean()) < 1e-10 and np.abs(rel).mean() < 1e-8


def test_split_bf16_operand_order_is_the_register_layout():
    """x3_off (csrc/kernels.hpp): the image's k slot (q, j) of 32-wide block kb
    is input column 32 kb + 16 (j >> 2) + 4 q + (j & 3) -- exactly the columns
    lane (cl, q) holds in output register blocks 2 kb (j < 4) and 2 kb + 1
    (j >= 4) of the previous layer -- and the map is a bijection onto the
    [hi | mid | lo] fragment slots."""
    def x3_off(o, i, tout):   # restated from kernels.hpp
        ii = i & 31
        q = (ii >> 2) & 3
        j = ((ii >> 4) << 2) | (ii & 3)
        f = (i >> 5) * tout + (o >> 4)
        return f * 1536 + ((o & 15) + 16 * q) * 8 + j

    TO, TI = 7, 7
    seen = set()
    for o in range(16 * TO):
        for i in range(16 * TI):
            off = x3_off(o, i, TO)
            f, rem = divmod(off, 1536)
            lane, j = divmod(rem, 8)
            assert rem < 512                          # the hi part; mid / lo at +512 / +1024
            cl, q = lane & 15, lane >> 4
            kb = f // TO
            assert cl == o % 16 and f % TO == o // 16
            # the column lane (cl, q) holds in register block t = 2 kb + (j >> 2), component j & 3
            t = 2 * kb + (j >> 2)
            assert i == 16 * t + 4 * q + (j & 3)
            seen.add(off)
    assert len(seen) == 16 * TO * 16 * TI
