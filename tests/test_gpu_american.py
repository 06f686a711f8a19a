"""The penalised American put on the device (dbsde_problem.pen, ProblemSpec
penalty; exact kind "american_put"): the Y-nonlinear driver at every place of
the engine that forms a step residual, pen = 0 against the problem without the
field, the device-mode step, the plugin path against the native one, the PDE
residual, the binomial-tree kernel and the problem classes.  Needs an MI355X.

Every expectation is computed on the CPU: oracle/fbsnn_ref.py with the
penalised driver as a duck-typed problem and the numpy tree of
tests/american_reference.py; tests/test_american_cpu.py holds those to
references of their own and checks the conditions on these tests' inputs (every
interior row at least 1e-3 away from g = Y, both branches populated).

Bounds: loss / Y / Z / gradient tests/depth_cases.py's BOUNDS against the fp64
oracle; the PDE residual's phi tests/test_gpu_jet.py's 2e-4 max|phi|; the tree
the fp32 rounding of an fp64 value (tests/test_gpu_put.py fp32_close).

Measured on an MI355X when these tests were written, the largest fraction of
its bound over the 16 site x payoff cases: loss 0.0409 (forward-only the same),
Y 0.0135, Z 0.0078, gradient 0.0107, worst tensor 0.0129; plugin and native both
loss 0.0115, Y 0.0032, Z 0.0032, gradient 0.0044, worst tensor 0.0053; the
device-mode loss of step 1 equal to its parity replay to every printed digit
(327.2307); phi of the PDE residual within 1.4e-7 of its largest value (bound
2e-4); tree price and delta at most 0.50 of 2^-23 relative.
"""
import math

import numpy as np
import pytest
import torch

import american_reference as ar
import depth_cases as dc
import put_reference as pr
import test_gpu_put as tp
from conftest import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


# ------------------------------------------------------------------ 1. every cotangent site
@pytest.mark.parametrize("site,payoff", ar.RUNS, ids=[f"{s}-{p}" for s, p in ar.RUNS])
def test_loss_and_gradients_match_the_fp64_oracle(pkg, dev, site, payoff):
    """M = 20, N = 3, parity-mode W, penalty 100: X bit-equal to the fp32
    oracle, loss / Y / Z / gradient (global and per tensor) within BOUNDS of the
    fp64 oracle of the penalised problem, the forward-only loss within
    BOUNDS["loss"], and the profiled repeat ran the site's kernels."""
    b = ar.reference(site, payoff)
    D = pr.site_dim(site)
    s = tp.site_solver(pkg, dev, site, ar.spec_for(pkg, site, payoff))
    r = tp.loss_grad(s, dev, b, D)
    names = tp.ran(s, dev, b, D)
    print(f"{site} {payoff}: matrix_form {s.matrix_form}, ran {sorted(names)}")
    dc.check(r, b, f"american {site} {payoff}")
    tp.check_site(s, site, names)
    fwd = tp.loss_grad(s, dev, b, D, grad=False)
    rel = abs(float(fwd["loss"][0]) - b["ref64"]["loss"]) / abs(b["ref64"]["loss"])
    print(f"american {site} {payoff}: forward-only loss error / bound {rel / dc.BOUNDS['loss']:.3g}")
    assert rel <= dc.BOUNDS["loss"]
    # the penalty is in the numbers: the same inputs without it give another loss
    s0 = tp.site_solver(pkg, dev, site, ar.spec_for(pkg, site, payoff, pen=0.0))
    r0 = tp.loss_grad(s0, dev, b, D, grad=False)
    assert abs(float(r0["loss"][0]) - b["ref64"]["loss"]) > 100 * dc.BOUNDS["loss"] * abs(b["ref64"]["loss"])


# ------------------------------------------------------------------ 2. pen = 0 is today's problem
@pytest.mark.parametrize("site", ["fused110", "chain110", "wide130"])
def test_zero_penalty_is_the_put_bit_for_bit(pkg, dev, site):
    payoff = "put_sum"
    b = ar.reference(site, payoff)
    D = pr.site_dim(site)
    base = pr.site_base(site, payoff)
    amer = ar.spec_for(pkg, site, payoff, pen=0.0)
    plain = pkg.ProblemSpec(g=payoff, strike=ar.strike_of(site, payoff), g_alpha=pr.ALPHA, **pr.COEF[base])
    assert "penalty" not in pr.COEF[base] and amer.penalty == 0.0
    ra = tp.loss_grad(tp.site_solver(pkg, dev, site, amer), dev, b, D)
    rp = tp.loss_grad(tp.site_solver(pkg, dev, site, plain), dev, b, D)
    for k in ("loss", "Y", "Z", "grad"):
        assert np.all(np.isfinite(ra[k])), k
        np.testing.assert_array_equal(ra[k], rp[k], err_msg=k)


# ------------------------------------------------------------------ 3. the device-mode step
def test_device_mode_steps_prefetched_and_not(pkg, dev):
    """AmericanBasketPutOption, D = 4, correlated, M = 64, N = 4: three Adam
    steps with each next rollout prefetched and three without give identical
    parameters and finite losses; the loss of step 1 equals a parity-mode
    replay on dbsde_brownian's exported (t, W) within BOUNDS["loss"]."""
    D, M, N = 4, 64, 4
    layers = [D + 1] + 4 * [16] + [1]

    def make():
        np.random.seed(5)
        torch.manual_seed(5)
        return pkg.AmericanBasketPutOption(np.ones((1, D)), 1.0, M, N, D, 1.0, layers, "NAIS-Net", "Sine",
                                           "restricted_random_correlation", device=dev)

    a, b_, c = make(), make(), make()
    assert a.native_coefficients and a.spec.penalty == 100.0 and a._L is not None
    assert np.array_equal(a._L, b_._L) and torch.equal(a.params, b_.params) and torch.equal(a.params, c.params)
    t, W = c.solver.brownian(M, N, seed=3)
    replay = float(c._run(t.unsqueeze(-1), W, c.Xi, want=())["loss"])
    oa, ob = a.new_optimizer_state("Adam", 1e-3), b_.new_optimizer_state("Adam", 1e-3)
    la, lb = [], []
    for it, seed in enumerate((3, 4, 5)):
        la.append(float(a.device_step(oa, 1e-3, seed=seed, next_seed=seed + 1 if it < 2 else None)))
        lb.append(float(b_.device_step(ob, 1e-3, seed=seed)))
    torch.cuda.synchronize()
    print("prefetched", la, "in-step", lb, "parity replay of step 1", replay)
    assert all(np.isfinite(la)) and la == lb
    assert torch.equal(a.params, b_.params) and not torch.equal(a.params, c.params)
    assert abs(la[0] - replay) <= dc.BOUNDS["loss"] * abs(replay)


# ------------------------------------------------------------------ 4. plugin against native
def test_plugin_and_native_agree_with_the_oracle(pkg, dev):
    """A PutOption subclass without a spec whose phi_tf carries the penalty runs
    generic.py; AmericanPutOption runs the kernels.  On the same parameters and
    parity batch (D = 4, M = 20, N = 3) both lie within BOUNDS of the fp64 oracle."""
    c = ar.PLUGIN
    b = ar.plugin_reference()
    D = c["D"]

    class Plugin(pkg.PutOption):
        def _default_strike(self):
            return c["strike"]

        def problem_spec(self):
            return None

        def phi_tf(self, t, X, Y, Z):
            return super().phi_tf(t, X, Y, Z) - ar.PEN * torch.relu(self.g_tf(X) - Y)

    class Native(pkg.AmericanPutOption):
        def _default_strike(self):
            return c["strike"]

    args = (np.ones((1, D)), ar.T, ar.M, ar.N, D, 1.0, c["layers"], c["mode"], c["act"])
    p, n = Plugin(*args, device=dev), Native(*args, device=dev)
    assert not p.native_coefficients and n.native_coefficients and n.spec.penalty == ar.PEN and n.spec.strike == c["strike"]
    t = torch.from_numpy(b["t"]).to(dev).unsqueeze(-1)
    W = torch.from_numpy(b["W"]).to(dev)
    for name, m in (("plugin", p), ("native", n)):
        m.params.copy_(torch.from_numpy(b["params"]).to(dev))
        g = torch.full_like(m.params, float("nan"))
        out = m._run(t, W, m.Xi, grad=g, want=("X", "Y", "Z"))
        torch.cuda.synchronize()
        got = {k: out[k].detach().cpu().numpy() for k in ("loss", "X", "Y", "Z")}
        got["Y"] = got["Y"].reshape(ar.M, ar.N + 1, 1)
        got["grad"] = g.cpu().numpy()
        if name == "plugin":       # its rollout is torch's: X within rounding, checked here, not bit for bit
            np.testing.assert_allclose(got["X"], b["ref32"]["X"], rtol=2e-6, atol=0)
            got["X"] = b["ref32"]["X"]
        dc.check(got, b, f"american {name}")


# ------------------------------------------------------------------ 5. pde_residual
def test_pde_residual_phi_carries_the_penalty(pkg, dev):
    """R = 16 points, D = 4, on both sides of g = u: phi == phi_r (u - phi_c x.Du)
    - pen relu(g(x) - u) recomputed in numpy from the returned u and net_u's Du,
    within tests/test_gpu_jet.py's bound for a term (2e-4 of its largest value);
    residual = u_t + drift + diffusion - phi with that phi.  The points are the
    first 16 of a fixed list of 64 whose margin |g - u| / (1 + |u|) is >= 1e-3."""
    D, R = 4, 16
    np.random.seed(6)
    torch.manual_seed(6)
    m = pkg.AmericanPutOption(np.ones((1, D)), 1.0, 8, 5, D, 1.0, [D + 1] + 4 * [16] + [1], "Naisnet", "Tanh", device=dev)
    assert m.native_coefficients
    rs = np.random.RandomState(5)
    Xc = rs.uniform(0.7, 1.3, (64, D)).astype(np.float32)
    tc = rs.uniform(0.0, 0.9, 64).astype(np.float32)
    gc = np.maximum(m.strike - Xc.astype(np.float64).sum(1), 0.0)
    # the output bias moves every u alike: put the median candidate on the exercise boundary
    bias = ar.output_bias(m.model)
    with torch.no_grad():
        bias.fill_(0.0)
        u0 = m.pde_residual(tc, Xc)["u"].cpu().numpy()[:, 0].astype(np.float64)
        bias.fill_(round(float(np.median(gc - u0)), 2))
    uc = m.pde_residual(tc, Xc)["u"].cpu().numpy()[:, 0].astype(np.float64)
    keep = np.flatnonzero(np.abs(gc - uc) / (1.0 + np.abs(uc)) >= 1e-3)[:R]
    assert keep.size == R
    t, X = tc[keep], Xc[keep]
    got = {k: v.cpu().numpy()[:, 0].astype(np.float64) for k, v in m.pde_residual(t, X).items()}
    u, du = m.net_u(torch.from_numpy(t).to(dev), torch.from_numpy(X).to(dev))
    torch.cuda.synchronize()
    du = du.detach().cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got["u"], u.detach().cpu().numpy()[:, 0].astype(np.float64), rtol=1e-6, atol=1e-7)
    g = np.maximum(m.strike - X.astype(np.float64).sum(1), 0.0)
    ex = g > got["u"]
    print(f"pde_residual: {int(ex.sum())} of {R} points in exercise, smallest margin "
          f"{(np.abs(g - got['u']) / (1 + np.abs(got['u']))).min():.2e}")
    assert 3 <= ex.sum() <= R - 3
    want = 0.05 * (got["u"] - 1.0 * np.sum(X.astype(np.float64) * du, 1)) - m.penalty * np.maximum(g - got["u"], 0.0)
    err = np.abs(got["phi"] - want).max()
    print(f"phi: max|err| = {err:.3e} = {err / np.abs(want).max():.3e} max|ref| (bound 2e-04)")
    assert err <= 2e-4 * np.abs(want).max()
    lin = 0.05 * (got["u"] - np.sum(X.astype(np.float64) * du, 1))
    assert np.abs(want - lin).max() > 100 * 2e-4 * np.abs(want).max()          # the penalty is what is being checked
    res = got["u_t"] + got["drift"] + got["diffusion"] - got["phi"]
    assert np.abs(got["residual"] - res).max() <= 2e-4 * np.abs(got["scale"]).max()


# ------------------------------------------------------------------ 6. the tree kernel
TREE_X = np.array([[0.8, 1.0], [0.9, 1.1], [0.95, 1.0], [1.2, 0.7], [1.0, 1.05]], np.float32)
TREE_T = np.array([0.0, 0.7, 1.0, 0.0, 0.7], np.float32)            # tau = 1, 0.3, 0, 1, 0.3
R_RATE, SIGMA, STRIKE = 0.05, 0.2, 1.0


@pytest.mark.parametrize("n_tree", [2, 3, 255, 256, 257, 1000])
def test_tree_kernel_matches_the_numpy_recursion(pkg, dev, n_tree):
    """R = 5 points x D = 2 (every coordinate on its own), pen in {0, 100, inf},
    b in {r, 2 r}: price and delta equal the fp64 numpy recursion within the fp32
    rounding of an fp64 value; the tau = 0 row is the payoff and its delta; two
    calls are bitwise equal."""
    t, X = torch.from_numpy(TREE_T).to(dev), torch.from_numpy(TREE_X).to(dev)
    tau = np.float64(np.float32(1.0)) - TREE_T.astype(np.float64)
    for pen in (0.0, 100.0, math.inf):
        for b in (R_RATE, 2 * R_RATE):
            price, delta = pkg.exact("american_put", t, X, 1.0, R_RATE, SIGMA, STRIKE, b=b, n_tree=n_tree, penalty=pen)
            p2, d2 = pkg.exact("american_put", t, X, 1.0, R_RATE, SIGMA, STRIKE, b=b, n_tree=n_tree, penalty=pen)
            torch.cuda.synchronize()
            assert price.shape == (5, 2) == delta.shape
            assert torch.equal(price, p2) and torch.equal(delta, d2)
            want = np.array([[ar.crr(TREE_X[i, j], STRIKE, R_RATE, SIGMA, b, tau[i], n_tree, pen) for j in range(2)]
                             for i in range(5)])
            tp.fp32_close(price.cpu().numpy(), want[..., 0], f"n {n_tree} pen {pen} b {b} price")
            tp.fp32_close(delta.cpu().numpy(), want[..., 1], f"n {n_tree} pen {pen} b {b} delta")
            np.testing.assert_array_equal(price.cpu().numpy()[2], np.maximum(np.float32(STRIKE) - TREE_X[2], 0))
            np.testing.assert_array_equal(delta.cpu().numpy()[2], [-1.0, -0.5])


def test_tree_defaults_bound_the_european_put(pkg, dev):
    """The defaults (b = r, 2000 steps, the American value) lie above Black-Scholes."""
    t, X = torch.from_numpy(TREE_T).to(dev), torch.from_numpy(TREE_X).to(dev)
    amer = pkg.exact("american_put", t, X, 1.0, R_RATE, SIGMA, STRIKE)[0]
    eur = pkg.exact("bs_put", t, X, 1.0, (R_RATE, SIGMA, STRIKE))[0]
    torch.cuda.synchronize()
    assert bool((amer >= eur - 1e-4).all()) and bool((amer > eur + 1e-4).any())


def test_tree_without_a_risk_neutral_probability_is_nan(pkg, dev):
    """n_tree = 2, b = 1: e^{b dt} > u at tau = 1 and at tau = 0.3, p > 1 -- NaN in
    price and delta on the device and in the numpy recursion; the tau = 0 point
    keeps its payoff."""
    t, X = torch.from_numpy(TREE_T).to(dev), torch.from_numpy(TREE_X).to(dev)
    price, delta = pkg.exact("american_put", t, X, 1.0, R_RATE, SIGMA, STRIKE, b=1.0, n_tree=2)
    torch.cuda.synchronize()
    for tau in (1.0, 0.3):
        assert all(math.isnan(v) for v in ar.crr(1.0, STRIKE, R_RATE, SIGMA, 1.0, tau, 2, math.inf))
    live = TREE_T < 1.0
    assert bool(torch.isnan(price[live]).all()) and bool(torch.isnan(delta[live]).all())
    np.testing.assert_array_equal(price.cpu().numpy()[2], np.maximum(np.float32(STRIKE) - TREE_X[2], 0))


# ------------------------------------------------------------------ 7. the objects
def test_european_twin_keeps_the_correlation(pkg, dev):
    """european() of a randomly correlated basket is the same problem: the same
    correlation matrix and Cholesky factor (not a new draw), penalty 0, and the
    caller's numpy and torch random streams untouched; its mc_value runs."""
    D = 4
    np.random.seed(8)
    torch.manual_seed(8)
    m = pkg.AmericanBasketPutOption(np.ones((1, D)), 1.0, 16, 4, D, 1.0, [D + 1] + 4 * [16] + [1], "Naisnet", "Tanh",
                                    "random_correlation", device=dev)
    assert m._L is not None and np.abs(np.tril(m._L, -1)).max() > 0
    ns, ts = np.random.get_state(), torch.get_rng_state()
    eu = m.european()
    assert eu.penalty == 0.0 and eu.spec.penalty == 0.0 and eu.correlation_type == "random_correlation"
    np.testing.assert_array_equal(eu._L, m._L)
    np.testing.assert_array_equal(eu.correlation_matrix, m.correlation_matrix)
    assert eu._L is not m._L
    ns2 = np.random.get_state()
    assert ns[0] == ns2[0] and np.array_equal(ns[1], ns2[1]) and ns[2:] == ns2[2:] and torch.equal(ts, torch.get_rng_state())
    # the context holds the same factor: the device-mode increments of both objects are the same
    _, Wm = m.solver.brownian(8, 4, seed=2)
    _, We = eu.solver.brownian(8, 4, seed=2)
    assert torch.equal(Wm, We)
    pts = np.full((3, D), 1.0, np.float32)
    val, err, _ = eu.mc_value(np.zeros(3, np.float32), pts, mc=2048)
    want, _, _ = pkg.mc_value(eu.problem_spec(), torch.zeros(3, device=dev), torch.from_numpy(pts).to(dev), 1.0, eu.N,
                              mc=2048, L=m._L)
    torch.cuda.synchronize()
    assert torch.equal(val, want) and bool((val > 0).all())


def test_american_objects(pkg, dev, tmp_path):
    """AmericanPutOption at D = 1: tree_value >= european().closed_form >= 0 at
    five points, the penalised tree in between; mc_value raises and names
    tree_value; three training steps run; save_model / load_model round-trip."""
    np.random.seed(7)
    torch.manual_seed(7)
    m = pkg.AmericanPutOption(np.ones((1, 1)), 1.0, 16, 6, 1, 1.0, [2] + 4 * [16] + [1], "Naisnet", "Tanh", device=dev)
    assert m.native_coefficients and m.penalty == 100.0 and m.spec.penalty == 100.0 and m.strike == 1.0
    tpts, Xpts = np.array([0.0, 0.2, 0.5, 0.8, 0.0], np.float32), np.array([0.8, 0.9, 1.0, 1.1, 1.2], np.float32)
    amer, ad = m.tree_value(tpts, Xpts)
    pen, _ = m.tree_value(tpts, Xpts, n_tree=500, penalised=True)
    amer500, _ = m.tree_value(tpts, Xpts, n_tree=500)
    eu = m.european()
    assert type(eu) is type(m) and eu.penalty == 0.0 and eu.spec.penalty == 0.0 and eu.native_coefficients
    cf, cd = eu.closed_form(tpts, Xpts)
    torch.cuda.synchronize()
    print("american", amer[:, 0].tolist(), "penalised", pen[:, 0].tolist(), "european", cf[:, 0].tolist())
    assert amer.shape == (5, 1) == cf.shape
    assert bool((amer >= cf - 1e-4).all()) and bool((cf >= 0).all()) and bool(((ad <= 0) & (ad >= -1)).all())
    assert bool((amer500 >= pen - 1e-7).all()) and bool((pen >= cf - 1e-4).all())
    # b = mu_a + phi_r phi_c = 0.10 for PutOption's coefficients, not r
    want = np.array([ar.bs_put_carry(float(x), 1.0, 0.05, 0.2, 0.10, 1.0 - float(t_)) for t_, x in zip(tpts, Xpts)])
    np.testing.assert_allclose(cf[:, 0].cpu().numpy(), want, rtol=1e-5, atol=1e-7)
    val, err, _ = eu.mc_value(tpts, Xpts.reshape(-1, 1), mc=4096, n_steps=50)
    assert float((val - cf).abs().max()) < 0.02
    with pytest.raises(ValueError, match="tree_value"):
        m.mc_value(tpts, Xpts.reshape(-1, 1), mc=64)
    with pytest.raises(ValueError, match="no closed form"):
        m.closed_form(tpts, Xpts)
    with pytest.raises(ValueError, match="D = 1"):
        pkg.AmericanBasketPutOption(np.ones((1, 3)), 1.0, 8, 4, 3, 1.0, [4] + 4 * [16] + [1], "Naisnet", "Tanh",
                                    device=dev).tree_value(tpts, np.ones((5, 3), np.float32))
    before = m.params.clone()
    out = m.train(3, 1e-3)
    torch.cuda.synchronize()
    assert np.isfinite(out[1]) and float((m.params - before).abs().max()) > 0
    path = str(tmp_path / "american.pt")
    m.save_model(path)
    kept = m.params.clone()
    with torch.no_grad():
        m.params.zero_()
    m.load_model(path)
    assert torch.equal(m.params, kept)
