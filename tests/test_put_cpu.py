"""The put payoffs without a GPU: the fp64 closed forms the device is compared
with (put-call parity, a deep out-of-the-money put), the Python surface
(plugin matching, the problem classes, option_type), and the conditions on the
inputs of tests/test_gpu_put.py: the tie rows really sit in, at and out of the
money, no terminal row of the oracle batches lies near the kink, and the
Monte-Carlo seeds keep the restatement's ambiguity cap.

References and case tables: tests/put_reference.py."""
import dataclasses
import importlib

import numpy as np
import pytest
import torch

import heston2_reference as h2
import mc_reference as mr
import put_reference as pr
from conftest import load_pkg
from oracle import fbsnn_ref as fr


# ------------------------------------------------------------------ closed forms
def test_black_scholes_parity_to_1e_12():
    """C - P = S - K e^{-r tau} to 1e-12 relative (of |C| + |P|) over the
    domain, the call by the same survival-function arithmetic."""
    rs = np.random.RandomState(3)
    S, tau = rs.uniform(0.5, 2.0, 200), rs.uniform(0.05, 2.0, 200)
    for sig in (0.2, 0.4, 1.0):
        c, cd = pr.bs_call(S, 1.0, tau, 0.05, sig)
        p, pd = pr.bs_put(S, 1.0, tau, 0.05, sig)
        err = np.abs(c - p - (S - np.exp(-0.05 * tau))) / (np.abs(c) + np.abs(p))
        print(f"sigma {sig}: max parity error {err.max():.2e}, max |delta parity| {np.abs(cd - pd - 1).max():.2e}")
        assert err.max() <= 1e-12
        assert np.abs(cd - pd - 1.0).max() <= 1e-12


def test_heston_parity_within_the_quadrature_bound():
    """On the kernel's nodes the two quadrature sums cancel in C - P, so parity
    holds far inside the rule's stated 2e-7."""
    worst = 0.0
    for rho, tau, v, m in h2.domain_grid():
        c, cd, p, pd = pr.heston_both(m, v, tau, rho=rho)
        worst = max(worst, abs(float(c - p) - (m - np.exp(-h2.R_RATE * tau))), abs(float(cd - pd) - 1.0))
        assert p >= -2e-7 and -1.0 - 2e-7 <= pd <= 2e-7
        call, delta = h2.closed_form(m, v, tau, rho=rho)
        assert float(call) == float(c) and float(delta) == float(cd)       # the call is heston2_reference's
    print(f"max parity error {worst:.2e}")
    assert worst <= 2e-7


def test_deep_out_of_the_money_put_needs_the_direct_formula():
    """S / K = 2, tau = 0.05: the kernel's formula (erfc-based N) against
    scipy.stats.norm.logsf-based arithmetic to 1e-10 relative, price and delta,
    at sigma = 0.4 (the GPU test's point) and at sigma = 0.2 (1e-56: fp64 only);
    the call minus parity misses both."""
    S, tau = pr.DEEP_OTM["S"], pr.DEEP_OTM["tau"]
    r, K = pr.BS["r"], pr.BS["K"]
    for sig, lo, hi in ((pr.BS["sig"], 1e-17, 1e-13), (0.2, 1e-60, 1e-50)):
        p, d = (float(v) for v in pr.bs_put(S, K, tau, r, sig))
        want, dwant = (float(v) for v in pr.bs_put(S, K, tau, r, sig, logsf=True))
        c, _ = pr.bs_call(S, K, tau, r, sig)
        by_parity = float(c) - (S - K * np.exp(-r * tau))
        print(f"sigma {sig}: put {p:.6e}, logsf {want:.6e}, rel {abs(p - want) / want:.2e}, "
              f"call minus parity {by_parity:.6e}")
        assert lo < want < hi
        assert abs(p - want) <= 1e-10 * want
        assert abs(d - dwant) <= 1e-10 * abs(dwant)
        assert abs(by_parity - want) > 1e-3 * want
    assert pr.bs_put(S, K, tau, r, pr.BS["sig"])[0] > 2.0 ** -126      # a normal fp32 number


def test_maturity_returns_the_payoff_and_its_gradient():
    p, d = pr.bs_put(np.array([1.5, 1.0, 0.5]), 1.0, np.array([0.0, 0.0, -0.1]), 0.05, 0.2)
    np.testing.assert_array_equal(p, [0.0, 0.0, 0.5])
    np.testing.assert_array_equal(d, [0.0, -0.5, -1.0])
    c, cd, p, d = pr.heston_both([1.5, 1.0, 0.5], 0.2, [0.0, 0.0, -0.1])
    np.testing.assert_array_equal(p, [0.0, 0.0, 0.5])
    np.testing.assert_array_equal(d, [0.0, -0.5, -1.0])
    X = np.array([[1.2, 0.9, 0.7], [0.6, 1.1, 1.4]])
    tau = np.array([0.5, 1.5])
    per, _ = pr.exact_put("bs_put", X, tau, 0.05, 0.2, 1.0)
    mean, _ = pr.exact_put("basket_mean_put", X, tau, 0.05, 0.2, 1.0)
    np.testing.assert_allclose(mean[:, 0], per.mean(1), rtol=1e-15)
    avg, _ = pr.exact_put("basket_avg_put", X, tau, 0.05, 0.2, 1.0)
    want, _ = pr.bs_put(X.mean(1), 1.0, tau, 0.05, 0.2 / np.sqrt(3.0))
    np.testing.assert_array_equal(avg[:, 0], want)


# ------------------------------------------------------------------ the Python surface
def test_spec_functions_have_the_put_payoffs_with_the_tie_split():
    pkg = load_pkg()
    gen = importlib.import_module(pkg.__name__ + ".generic")
    X = torch.tensor([[1.0, 1.0, 1.0, 7.0], [1.5, 1.25, 1.0, 7.0], [0.5, 0.75, 1.0, 7.0]], dtype=torch.float64)
    for payoff in pr.PAYOFFS:
        K = 3.0 if payoff == "put_sum" else 1.0
        f = gen.spec_functions(pkg.ProblemSpec(g=payoff, strike=K, g_alpha=10.0, g_cols=3))
        prob = pr.PutProblem("basket", 3, payoff, K)
        torch.testing.assert_close(f["g_tf"](X), prob.g(X[:, :3]), rtol=0, atol=0)
        dg = f["Dg_tf"](X)
        assert bool((dg[:, 3] == 0).all())
        if payoff != "smooth_put":
            n = 1.0 if payoff == "put_sum" else 3.0
            np.testing.assert_array_equal(dg[:, :3].numpy(), np.array([[-0.5], [0.0], [-1.0]]) / n * np.ones((1, 3)))
        spec = pkg.ProblemSpec(g=payoff, strike=K, g_alpha=10.0, g_cols=3)
        g, dgr, _ = pr.payoff(spec, X.numpy())
        np.testing.assert_allclose(g, f["g_tf"](X).numpy()[:, 0], rtol=1e-15)
        np.testing.assert_allclose(dgr, dg.numpy(), rtol=1e-14, atol=1e-16)


def test_a_plugin_put_selects_the_native_spec():
    """A reference-style subclass whose g_tf is maximum(K - mean, 0) agrees with
    the put_mean spec on the probes (so it runs the native table) and differs
    from the call spec it inherits."""
    pkg = load_pkg()
    gen = importlib.import_module(pkg.__name__ + ".generic")
    fbm = importlib.import_module(pkg.__name__ + ".fbsnn")

    class UserPut(pkg.BasketCallOption):
        def problem_spec(self):
            return dataclasses.replace(super().problem_spec(), g="put_mean")

        def g_tf(self, X):
            return torch.maximum(self.strike - torch.mean(X, dim=1, keepdim=True), torch.tensor(0.0, device=X.device))

    D = 5
    obj = object.__new__(UserPut)
    obj.strike, obj.D, obj.M, obj.device = 1.0, D, 4, torch.device("cpu")
    assert obj.problem_spec().g == "put_mean"
    assert gen.coefficient_mismatches(obj, fbm.FBSNN, obj.problem_spec(), D, 1.0, torch.ones(1, D), "cpu") == []
    call = pkg.BasketCallOption.problem_spec(obj)
    assert gen.coefficient_mismatches(obj, fbm.FBSNN, call, D, 1.0, torch.ones(1, D), "cpu") == ["g_tf"]


def test_put_classes_agree_with_their_specs():
    pkg = load_pkg()
    gen = importlib.import_module(pkg.__name__ + ".generic")
    fbm = importlib.import_module(pkg.__name__ + ".fbsnn")
    for cls, parent, D, strike, g in ((pkg.PutOption, pkg.CallOption, 5, 5.0, "put_sum"),
                                      (pkg.BasketPutOption, pkg.BasketCallOption, 5, 1.0, "put_mean")):
        obj = object.__new__(cls)
        obj.D = D
        assert cls._default_strike(obj) == strike == parent._default_strike(obj)     # the parent's strike default
        obj.strike, obj.M, obj.device = strike, 4, torch.device("cpu")
        spec = obj.problem_spec()
        assert spec == dataclasses.replace(parent.problem_spec(obj), g=g)
        assert gen.coefficient_mismatches(obj, fbm.FBSNN, spec, D, 1.0, torch.ones(1, D), "cpu") == [], cls.__name__
        assert cls.train is parent.train and cls.schedule == parent.schedule


def _bare_heston(pkg, cls, k, payoff_type, option_type):
    m = object.__new__(cls)
    m.kappa, m.theta, m.sigma, m.rho, m.v0 = 2.0, 0.2, 0.3, 0.8, 0.2
    m.payoff_type, m.option_type, m.n_assets, m.strike, m.T = payoff_type, option_type, k, 1.0, 1.0
    m.layers, m.device = [1 + 2 * k, 16, 16, 16, 16, 1], torch.device("cpu")
    m.Xi = torch.tensor(h2.xi_state(k), dtype=torch.float32)
    return m


@pytest.mark.parametrize("payoff_type", ["discontinuous", "continuous"])
def test_heston_option_type_selects_the_put(payoff_type):
    pkg = load_pkg()
    want = {"discontinuous": ("call_mean", "put_mean"), "continuous": ("smooth_call", "smooth_put")}[payoff_type]
    X = torch.tensor(np.random.RandomState(2).uniform(0.5, 1.5, (6, 6)), dtype=torch.float32)
    X[0, :3] = 1.0                                    # a row at the kink
    for cls, kind in ((pkg.HestonFBSNN, "heston"), (pkg.HestonTwoFactorFBSNN, "heston2")):
        call = _bare_heston(pkg, cls, 3, payoff_type, "call")
        put = _bare_heston(pkg, cls, 3, payoff_type, "put")
        assert call.problem_spec().g == want[0] and put.problem_spec().g == want[1]
        assert dataclasses.replace(put.problem_spec(), g=want[0]) == call.problem_spec()
        assert put._select_problem().kind == kind and put.native_coefficients
        h = pr.PutHeston(k=3, payoff=payoff_type)
        torch.testing.assert_close(put.g_tf(X), h.g(X[:, :3]), rtol=0, atol=0)
        torch.testing.assert_close(call.g_tf(X), fr.Heston(k=3, payoff=payoff_type).g(X[:, :3]), rtol=0, atol=0)
        # the put is the call in the mirrored moneyness
        a = torch.mean(X[:, :3], dim=1, keepdim=True) - 1.0
        torch.testing.assert_close(put.g_tf(X), call.g_tf(torch.cat([X[:, :3] - 2 * a, X[:, 3:]], 1)), rtol=0, atol=1e-6)


def test_an_unknown_option_type_is_refused():
    pkg = load_pkg()
    for cls in (pkg.HestonFBSNN, pkg.HestonTwoFactorFBSNN):
        with pytest.raises(ValueError, match="option type"):
            cls(np.ones((1, 1)), 1.0, 4, 4, 1, None, [2, 16, 16, 16, 16, 1], "Naisnet", "Sine", option_type="straddle")
    with pytest.raises(ValueError, match="payoff type"):           # the existing refusal comes first and stays
        pkg.HestonFBSNN(np.ones((1, 1)), 1.0, 4, 4, 1, None, [2, 16, 16, 16, 16, 1], "Naisnet", "Sine",
                        payoff_type="smooth", option_type="put")
    put = _bare_heston(pkg, pkg.HestonTwoFactorFBSNN, 2, "discontinuous", "put")
    with pytest.raises(ValueError, match="one asset"):
        put.closed_form([1.0], [0.2], [0.0])
    put = _bare_heston(pkg, pkg.HestonTwoFactorFBSNN, 1, "continuous", "put")
    with pytest.raises(ValueError, match="discontinuous"):
        put.closed_form([1.0], [0.2], [0.0])


# ------------------------------------------------------------------ conditions on the GPU tests' inputs
@pytest.mark.parametrize("site,payoff", [(s, p) for s in pr.TIE_SITES for p in pr.TIE_PAYOFFS])
def test_tie_inputs_sit_at_in_and_out_of_the_money(site, payoff):
    """X_N = Xi bit for bit (fp32 and fp64 oracle), K - sum / mean is exactly
    0, negative, positive, and the oracle's terminal gradient is the 1/2 split
    on the tie row.  What the GPU test can see of a wrong split (0: relu's
    gradient at the tie, or the full -1: clamp's): the worst parameter tensor's
    gradient moves by more than 10 of its bounds (the zbar side), and the
    terminal Z-term by more than 10 times 1e-5 of the loss, the tolerance of the
    GPU test's Z-term comparison (the loss bound alone would not notice it at
    D = 100 with the mean payoff: 1.9 bounds)."""
    import copy
    import depth_cases as dc
    b = pr.tie_reference(site, payoff)
    D = pr.site_dim(site)
    n = 1.0 if payoff == "put_sum" else float(D)
    for ref in (b["ref32"], b["ref64"]):
        XN = ref["X"][:, -1, :]
        np.testing.assert_array_equal(XN, b["Xi"])
        np.testing.assert_array_equal(ref["X"][:, 0, :], b["Xi"])
    a = pr.moneyness(b, payoff, 1.0)
    assert a[0] == 0.0 and a[1] < 0.0 and a[2] > 0.0, a
    XN = torch.tensor(b["ref64"]["X"][:, -1, :], requires_grad=True)
    dg = fr.dg(b["problem"], XN).detach().numpy()
    np.testing.assert_array_equal(dg, np.array([[-0.5], [0.0], [-1.0]]) / n * np.ones((1, D)))
    Z = b["ref64"]["Z"][0, -1, :]
    here = np.sum((Z + 0.5 / n) ** 2)
    moved = min(abs(np.sum(Z ** 2) - here), abs(np.sum((Z + 1.0 / n) ** 2) - here))
    print(f"{site} {payoff}: loss {b['ref64']['loss']:.6e}, a wrong split moves the Z-term by at least {moved:.3e}")
    assert moved > 10 * pr.TIE_ZTERM_RTOL * abs(b["ref64"]["loss"])

    class WrongSplit(pr.PutProblem):
        def g(self, X):
            s = torch.sum(X, dim=1, keepdim=True) if self.payoff == "put_sum" else torch.mean(X, dim=1, keepdim=True)
            return self.split(self.strike - s)

    t, W, Xi = (torch.tensor(b[k]).double() for k in ("t", "W", "Xi"))
    for split in (torch.relu, lambda a: torch.clamp(a, min=0.0)):
        w = WrongSplit("bsb", D, payoff, pr.strike_of(payoff, D, 1.0))
        w.split = split
        r = fr.loss_and_grads(copy.deepcopy(b["model"]).double(), w, t[..., None], W, Xi, len(pr.TIE_LEVELS), D)
        e = dc.errors(r, b["ref64"], b["tensors"])
        print(f"  wrong split: loss {e['loss']:.3g}, grad {e['grad']:.3g}, tensor {e['tensor']:.3g} of the bounds")
        assert e["tensor"] > 10


@pytest.mark.parametrize("site,payoff", pr.RUNS)
def test_oracle_batches_are_well_conditioned(site, payoff):
    """No terminal row of a kinked payoff so near the kink that an fp32 row sum
    could sit on its other side: |K - s| above twice the worst-case rounding of
    a D-term fp32 sum, 2 D 2^-24 |s| (X itself is bit-equal to the fp32
    oracle's).  Rows on both sides of the kink, and the fp32 oracle within 5 %
    of each bound from the fp64 one (tests/depth_cases.py's rule)."""
    import depth_cases as dc
    b = pr.reference(site, payoff)
    a = pr.moneyness(b, payoff)
    print(f"{site} {payoff}: min |K - s| = {np.abs(a).min():.3e}, in the money {int((a > 0).sum())} of {a.size}")
    D = pr.site_dim(site)
    if payoff != "smooth_put":
        assert np.abs(a).min() > 2 * D * 2.0 ** -24 * pr.strike_of(payoff, D)
    assert 0 < (a > 0).sum() < a.size
    e = dc.errors(b["ref32"], b["ref64"], b["tensors"])
    print({k: v for k, v in e.items()})
    for k in ("loss", "Y", "Z", "grad", "tensor"):
        assert e[k] <= 0.05, (k, e[k])


@pytest.mark.parametrize("shape", pr.MC_SHAPES)
@pytest.mark.parametrize("name", pr.MC_DIAG)
def test_mc_seeds_keep_the_ambiguity_cap(name, shape):
    """The restatement alone: at most 4 samples per point within 2e-5 of the
    kink, as tests/test_gpu_mc.py tolerates for the calls; at maturity the
    payoff and its -1 / -1/2 / 0 gradient."""
    pkg = load_pkg()
    ref = pr.mc_diag_case(pkg, name, shape)
    print("ambiguous", ref["ambiguous"], "value", ref["value"])
    assert ref["ambiguous"].max() <= 4
    assert np.all(np.isfinite(ref["value"])) and np.all(ref["stderr"][[0, 1, 2, 4]] > 0) and ref["stderr"][3] == 0
    spec, _ = pr.mc_diag_spec(pkg, name, shape[0])
    g, dg, _ = pr.payoff(spec, pr.mc_points(shape[0])[3:4])
    assert ref["value"][3] == g[0] and np.all(ref["delta"][3] == dg[0])
    if name != "smooth_put":                         # (the smoothed payoff dips below 0 out of the money)
        assert np.all(ref["value"] >= 0) and np.all(ref["delta"][[0, 1, 2, 4]] <= 0)


@pytest.mark.parametrize("kind,g", pr.MC_HESTON)
def test_mc_heston_seeds_keep_the_ambiguity_cap(kind, g):
    pkg = load_pkg()
    ref = pr.mc_heston_case(pkg, kind, g)
    print("ambiguous", ref["ambiguous"], "value", ref["value"])
    assert ref["ambiguous"].max() <= 4
    assert np.all(np.isfinite(ref["value"])) and np.all(ref["stderr"][[0, 1, 2, 4]] > 0)


def test_put_payoff_mirrors_the_call_restatement():
    """tests/put_reference.py's payoff against tests/mc_reference.py's call
    payoff on mirrored states: g_put(X) = g_call(2 K' - X) with dg negated."""
    pkg = load_pkg()
    X = np.random.RandomState(5).uniform(0.5, 1.5, (50, 4))
    X[0, :3] = 1.0
    for g in pr.PAYOFFS:
        K = 3.0 if g == "put_sum" else 1.0
        put = pkg.ProblemSpec(g=g, strike=K, g_alpha=10.0, g_cols=3)
        call = dataclasses.replace(put, g=pr.CALL_OF[g])
        mirror = X.copy()
        mirror[:, :3] = 2.0 - X[:, :3]                # sum -> 6 - sum, mean -> 2 - mean
        gp, dp, ap = pr.payoff(put, X)
        gc, dc_, ac = mr.payoff(call, mirror)
        np.testing.assert_allclose(gp, gc, rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(dp, -dc_, rtol=1e-13, atol=1e-15)
        if ap is not None:
            np.testing.assert_allclose(ap, ac, rtol=0, atol=1e-15)
            assert dp[0, 0] == (-0.5 if g == "put_sum" else -0.5 / 3)
