"""The two-factor Heston problem on the device (problem kind "heston2", exact
kind "heston"): rollout_heston2_kernel in every role (increments, paths,
parity batches, shards, prefetch), the loss and gradient on both matrix forms,
the PDE residual, the Monte-Carlo comparator, the closed form, and
HestonTwoFactorFBSNN.  Needs an MI355X.

Every expectation is computed on the CPU from oracle/philox.py,
oracle/fbsnn_ref.py and tests/heston2_reference.py (held to fp64 references of
its own by tests/test_heston2_cpu.py).

Shapes: k in {1, 3, 17, 70} (one thread per path; a ragged 16-block; D = 140
takes the wide per-layer path), M in {24, 7}, N = 6 (the last 4-step Philox
block is half used), 16-wide Naisnet-Sine networks; the loss test adds k = 50
at width 110, the shape whose kernels have a split-bf16 and an fp32 form (16-wide
networks have one form).  Bounds: increments the
documented normal error (rtol = atol = 2e-6, tests/test_gpu_device_rng.py);
paths bit-equal to the numpy chain on the device's own increments; loss / Y /
Z / gradient as tests/test_gpu_heston_corr.py's check; PDE terms 2e-4 max|term|;
Monte-Carlo and closed form RTOL, ATOL = 2e-5, 2e-6 (tests/test_gpu_mc.py)."""
import os

import numpy as np
import pytest
import torch

import heston2_reference as h2
import heston_corr_reference as hc
import jet_reference as jr
from conftest import load_pkg
from oracle import philox as ph

pytestmark = pytest.mark.gpu
T, N = h2.T, h2.N
KS = list(h2.KS)
MS = h2.MS
SEED = 4
RTOL, ATOL = 2e-5, 2e-6
FP32_ENV = {"DBSDE_X3": "0", "DBSDE_TNW_X3": "0"}
X3_ENV = {"DBSDE_X3": "1", "DBSDE_TNW_X3": "1"}


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def make_solver(pkg, dev, k, layers=None, env=None, kind="heston2", act="Sine"):
    """A context of the kind (env: variables set while it is created)."""
    layers = layers or [1 + 2 * k, 16, 16, 16, 16, 1]
    old = {n: os.environ.get(n) for n in (env or {})}
    os.environ.update(env or {})
    try:
        s = pkg.NativeSolver("Naisnet", layers, act, h2.spec(pkg, k, kind=kind), T, dev)
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
    assert s.D == 2 * k and s.nb == (2 * k if kind == "heston2" else k)
    return s


_SOLVERS = {}


def solver(pkg, dev, k):
    if k not in _SOLVERS:
        _SOLVERS[k] = make_solver(pkg, dev, k)
    return _SOLVERS[k]


def xi_dev(dev, k):
    return torch.as_tensor(h2.xi_state(k), dtype=torch.float32).to(dev).contiguous()


def device_step(s, dev, params, M, xi, seed, path0=0, grad=False, t=None, W=None):
    """(X [M, N+1, 2k], loss, grad) of a loss_grad."""
    X = torch.empty(M * (N + 1) * s.D, device=dev)
    loss = torch.empty(1, device=dev)
    g = torch.empty_like(params) if grad else None
    s.loss_grad(params, M, N, xi, seed=seed, path0=path0, loss=loss, X=X, grad=g, t=t, W=W)
    torch.cuda.synchronize()
    return X.cpu().numpy().reshape(M, N + 1, s.D), float(loss), (g.cpu().numpy() if grad else None)


# ------------------------------------------------------------------ 4. increments and paths
@pytest.mark.parametrize("k", KS)
def test_increments_t_and_W(pkg, dev, k):
    s = solver(pkg, dev, k)
    for M in MS:
        t, dW = s.brownian(M, N, seed=SEED, increments=True)
        t2, W = s.brownian(M, N, seed=SEED)
        torch.cuda.synchronize()
        dW = dW.cpu().numpy()
        assert dW.shape == (M, N, 2 * k)
        ref = ph.increments(SEED, 0, 0, M, N, 2 * k, T)
        print(f"k={k} M={M}: max|dW err| = {np.abs(dW - ref).max():.3e}, max|ref| = {np.abs(ref).max():.3e}")
        np.testing.assert_allclose(dW, ref, rtol=2e-6, atol=2e-6)
        np.testing.assert_array_equal(t.cpu().numpy(), np.broadcast_to(ph.time_grid(N, T), (M, N + 1)))
        np.testing.assert_array_equal(t2.cpu().numpy(), t.cpu().numpy())
        np.testing.assert_array_equal(W.cpu().numpy(), ph.brownian_W(dW))


@pytest.mark.parametrize("k", KS)
def test_paths_are_the_chain_on_the_device_increments(pkg, dev, k):
    s = solver(pkg, dev, k)
    zero = torch.zeros(s.nparams, device=dev)
    for M in MS:
        _, dW = s.brownian(M, N, seed=SEED, increments=True)
        X, _, _ = device_step(s, dev, zero, M, xi_dev(dev, k), SEED)
        Xr, _ = h2.rollout(h2.xi_state(k), dW.cpu().numpy(), T, **h2.HESTON)
        np.testing.assert_array_equal(X, Xr)
        assert np.abs(X[:, -1, k:] - 0.2).max() > 1e-3          # the variance moves


@pytest.mark.parametrize("k", [1, 17, 70])
def test_parity_batch_on_the_fetched_W(pkg, dev, k):
    """External t / W [M, N+1, 2k]: the chain on the fp32 differences of W, and
    the device-mode paths again where those differences are the increments."""
    s = solver(pkg, dev, k)
    zero, xi, M = torch.zeros(s.nparams, device=dev), xi_dev(dev, k), 7
    t, W = s.brownian(M, N, seed=SEED)
    torch.cuda.synchronize()
    Xp, _, _ = device_step(s, dev, zero, M, xi, SEED, t=t.contiguous(), W=W.contiguous())
    Wn = W.cpu().numpy()
    Xr, _ = h2.rollout(h2.xi_state(k), Wn[:, 1:] - Wn[:, :-1], T, **h2.HESTON)
    np.testing.assert_array_equal(Xp, Xr)
    # fed increments that are exact fp32 differences (a W of one step), the two modes agree bit for bit
    t1, W1 = s.brownian(M, 1, seed=SEED)
    torch.cuda.synchronize()
    X1 = torch.empty(M * 2 * s.D, device=dev)
    Xd = torch.empty(M * 2 * s.D, device=dev)
    s.loss_grad(zero, M, 1, xi, seed=SEED, X=Xd, loss=torch.empty(1, device=dev))
    s.loss_grad(zero, M, 1, xi, t=t1.contiguous(), W=W1.contiguous(), X=X1, loss=torch.empty(1, device=dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(X1.cpu().numpy(), Xd.cpu().numpy())


@pytest.mark.parametrize("k", [3, 70])
def test_shards_and_prefetch(pkg, dev, k):
    s = solver(pkg, dev, k)
    zero, xi = torch.zeros(s.nparams, device=dev), xi_dev(dev, k)
    X24, _, _ = device_step(s, dev, zero, 24, xi, SEED)
    parts = [device_step(s, dev, zero, m, xi, SEED, path0=p0)[0] for p0, m in ((0, 7), (7, 9), (16, 8))]
    np.testing.assert_array_equal(np.concatenate(parts), X24)
    params = torch.from_numpy(h2.loss_model(k)[2].astype(np.float32)).to(dev)     # (not clamped away)
    ref = device_step(s, dev, params, 24, xi, 5, grad=True)
    other = device_step(s, dev, params, 24, xi, 6, grad=True)
    assert np.isfinite(ref[1]) and np.abs(ref[2]).max() > 0
    s.prefetch(24, N, xi, seed=5)                     # prefetched, consumed by the next step
    got = device_step(s, dev, params, 24, xi, 5, grad=True)
    s.prefetch(24, N, xi, seed=5)                     # held back over a step of another batch
    mid = device_step(s, dev, params, 24, xi, 6, grad=True)
    late = device_step(s, dev, params, 24, xi, 5, grad=True)
    for a, b in ((got, ref), (late, ref), (mid, other)):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1]
        np.testing.assert_array_equal(a[2], b[2])


def test_a_factor_is_refused(pkg, dev):
    s = solver(pkg, dev, 3)
    with pytest.raises(ValueError, match="two-factor"):
        s.set_corr(np.eye(6))
    s.set_corr(None)                                  # clearing what was never set is accepted


# ------------------------------------------------------------------ 5. loss and gradient
def check(r, ref):
    """tests/test_gpu_heston_corr.py's check."""
    for key in ("loss", "Y", "Z", "grad"):
        a, b = np.asarray(r[key], np.float64).ravel(), np.asarray(ref[key], np.float64).ravel()
        print(f"{key}: max|err| = {np.abs(a - b).max():.3e}, max|ref| = {np.abs(b).max():.3e}")
    np.testing.assert_allclose(r["X"], ref["X"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["loss"][0], ref["loss"], rtol=1e-4)
    np.testing.assert_allclose(r["Y"], ref["Y"], rtol=0, atol=1e-4 * max(1.0, np.abs(ref["Y"]).max()))
    np.testing.assert_allclose(r["Z"], ref["Z"], rtol=0, atol=1e-4 * max(1.0, np.abs(ref["Z"]).max()))
    used = ref["used"]
    assert np.all(r["grad"][~used] == 0)
    np.testing.assert_allclose(r["grad"][used], ref["grad"][used], rtol=0, atol=2e-4 * np.abs(ref["grad"]).max())


LOSS_CASES = h2.LOSS_CASES
_LOSS_REFS = {}


def loss_reference(case, dW):
    """The fp64 oracle on the device's own increments, computed once (both
    matrix forms draw the same batch: the path kernel is the same)."""
    k, M, width = LOSS_CASES[case]
    if case not in _LOSS_REFS:
        _, model, _ = h2.loss_model(k, width)
        _LOSS_REFS[case] = (dW, h2.loss_and_grads(model, k, ph.time_grid(N, T), dW, h2.xi_state(k), **h2.HESTON))
    np.testing.assert_array_equal(dW, _LOSS_REFS[case][0])
    return _LOSS_REFS[case][1]


@pytest.mark.parametrize("form", ["x3", "fp32"])
@pytest.mark.parametrize("case", list(LOSS_CASES))
def test_loss_and_gradient_match_oracle(pkg, dev, case, form):
    k, M, width = LOSS_CASES[case]
    layers, _, flat = h2.loss_model(k, width)
    s = make_solver(pkg, dev, k, layers, FP32_ENV if form == "fp32" else X3_ENV)
    print(f"{case} {form}: matrix_form = {s.matrix_form}")
    _, dW = s.brownian(M, N, seed=h2.LOSS_SEED + k, increments=True)
    torch.cuda.synchronize()
    ref = loss_reference(case, dW.cpu().numpy())
    params = torch.from_numpy(flat.astype(np.float32)).to(dev)
    out = dict(loss=torch.empty(1, device=dev), X=torch.empty(M * (N + 1) * 2 * k, device=dev),
               Y=torch.empty(M * (N + 1), device=dev), Z=torch.empty(M * (N + 1) * 2 * k, device=dev))
    grad = torch.empty_like(params)
    s.loss_grad(params, M, N, xi_dev(dev, k), seed=h2.LOSS_SEED + k, grad=grad, **out)
    torch.cuda.synchronize()
    r = {n: v.cpu().numpy() for n, v in out.items()}
    r["X"], r["Z"] = r["X"].reshape(M, N + 1, 2 * k), r["Z"].reshape(M, N + 1, 2 * k)
    r["Y"], r["grad"] = r["Y"].reshape(M, N + 1, 1), grad.cpu().numpy()
    check(r, ref)


# ------------------------------------------------------------------ 6. PDE residual
def native_terms(s, dev, flat, t, X):
    R = X.shape[0]
    out = {key: torch.empty(R, device=dev) for key in jr.TERMS}
    s.pde_residual(torch.from_numpy(flat).to(dev), torch.from_numpy(t.ravel().copy()).to(dev),
                   torch.from_numpy(X).to(dev).contiguous(), **out)
    torch.cuda.synchronize()
    return {key: v.cpu().numpy().reshape(R, 1) for key, v in out.items()}


@pytest.mark.parametrize("k", [1, 3])
def test_pde_residual_terms(pkg, dev, k):
    """R = 12 random points on tests/heston_corr_reference.py's pde_setup recipe
    (about half of the rows clamp); the diffusion of kind 1 at the same points
    and parameters differs by far more than the tolerance."""
    oracle, flat, t, X, clamped = hc.pde_setup(k=k, seed=7, R=12)
    layers = [1 + 2 * k, 16, 16, 16, 16, 1]
    want = h2.pde_terms(oracle, t, X, k, **h2.HESTON)
    got = native_terms(make_solver(pkg, dev, k, layers, act="Tanh"), dev, flat, t, X)
    smax = float(np.abs(want["scale"]).max())
    for key in jr.TERMS:
        top = smax if key == "residual" else float(np.abs(want[key]).max())
        err = float(np.abs(got[key] - want[key]).max())
        print(f"{key}: max|err| = {err:.3e} = {err / top:.3e} max|ref| (bound 2e-04)")
        assert top > 0 and np.all(np.isfinite(got[key]))
        np.testing.assert_allclose(got[key], want[key], rtol=0, atol=2e-4 * top)
        assert np.all(got[key][clamped] == 0), key
    one = native_terms(make_solver(pkg, dev, k, layers, kind="heston", act="Tanh"), dev, flat, t, X)
    top = float(np.abs(want["diffusion"]).max())
    gap = float(np.abs(one["diffusion"] - got["diffusion"]).max())
    print(f"diffusion: max|kind 1 - kind 2| = {gap:.3e} = {gap / top:.3e} max|ref|")
    assert gap > 10 * 2e-4 * top
    np.testing.assert_array_equal(one["drift"], got["drift"])        # the drift is kind 1's


# ------------------------------------------------------------------ 7. Monte-Carlo
def mc_device(pkg, dev, spec, t, X, n_steps, mc, seed, delta=False):
    v, e, d = pkg.mc_value(spec, torch.from_numpy(np.asarray(t, np.float32)).to(dev),
                           torch.from_numpy(np.asarray(X, np.float32)).to(dev), T, n_steps, mc=mc, seed=seed, delta=delta)
    torch.cuda.synchronize()
    return v.cpu().numpy()[:, 0], e.cpu().numpy()[:, 0]


@pytest.mark.parametrize("payoff", ["call_mean", "smooth_call"])
@pytest.mark.parametrize("k", [1, 2])
def test_mc_same_draws(pkg, dev, k, payoff):
    ref = h2.mc_case(pkg, k, payoff)
    assert ref["ambiguous"].max() <= 4
    spec = h2.spec(pkg, k, payoff)
    v, e = mc_device(pkg, dev, spec, h2.MC_T_POINTS, h2.mc_points(k), h2.MC_STEPS, h2.MC_SAMPLES, h2.MC_SEED)
    print("value", v, ref["value"], "stderr", e, ref["stderr"])
    np.testing.assert_allclose(v, ref["value"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(e, ref["stderr"], rtol=RTOL, atol=ATOL)
    one = mc_device(pkg, dev, h2.spec(pkg, k, payoff, kind="heston"), h2.MC_T_POINTS, h2.mc_points(k), h2.MC_STEPS,
                    h2.MC_SAMPLES, h2.MC_SEED)
    assert np.abs(one[0][:3] - v[:3]).max() > 100 * ATOL            # not the one-factor process
    with pytest.raises(ValueError, match="Heston"):
        mc_device(pkg, dev, spec, h2.MC_T_POINTS, h2.mc_points(k), h2.MC_STEPS, h2.MC_SAMPLES, h2.MC_SEED, delta=True)


def test_mc_point_does_not_depend_on_the_call(pkg, dev):
    k = 2
    spec, X, t = h2.spec(pkg, k), h2.mc_points(k), h2.MC_T_POINTS
    args = (h2.MC_STEPS, h2.MC_SAMPLES, h2.MC_SEED)
    a = mc_device(pkg, dev, spec, t, X, *args)
    b = mc_device(pkg, dev, spec, t, X, *args)
    one = mc_device(pkg, dev, spec, t[2:3], X[2:3], *args)
    X11 = np.concatenate([X, X, X[2:3]])[[0, 1, 3, 2, 4, 5, 6, 7, 8, 10, 9]]         # rows 3 and 9 <- X[2]
    t11 = np.concatenate([t, t, t[2:3]])[[0, 1, 3, 2, 4, 5, 6, 7, 8, 10, 9]]
    big = mc_device(pkg, dev, spec, t11, X11, *args)
    for u, w, o, g in zip(a, b, one, big):
        np.testing.assert_array_equal(u, w)
        assert o[0] == u[2] == g[3] == g[9]
    assert one[0][0] != a[0][0]


def test_mc_ties_to_the_closed_form(pkg, dev):
    """(S, v, t) = (1, 0.2, 0), K = 1, n_steps = 100, mc = 2^18:
    |mc - closed form| <= 4 stderr + 2 b, b the Euler bias bound of
    tests/heston2_reference.py (EULER_BIAS_100), and that bound is
    below a third of S P1 (1 - e^{-rT}), the gap to a formula that discounts
    the S P1 term as well: the comparison tells the two formulas apart.
    b = 2.10e-4 with standard error 0.43e-4 (below b / 4) from 92,274,688 CPU
    paths.  Measured: mc 0.198606 +- 8.0e-4, closed form 0.198421, difference
    1.85e-4, bound 3.63e-3, gap 2.94e-2."""
    c = h2.EULER_TIE
    spec = h2.spec(pkg, 1)
    v, e = mc_device(pkg, dev, spec, [c["t"]], [[c["S"], c["v"]]], c["n_steps"], c["mc"], seed=9)
    price, delta = pkg.exact("heston", torch.tensor([c["t"]], device=dev), torch.tensor([[c["S"], c["v"]]], device=dev),
                             T, (h2.R_RATE, 1.0, 2.0, 0.2, 0.3, 0.8))
    torch.cuda.synchronize()
    cf, p1 = float(price[0, 0]), float(delta[0, 0])
    bound = 4 * float(e[0]) + 2 * h2.EULER_BIAS_100
    gap = c["S"] * p1 * (1.0 - np.exp(-h2.R_RATE * T))
    print(f"mc {v[0]:.6f} +- {e[0]:.2e}, closed form {cf:.6f}, |diff| {abs(v[0] - cf):.2e}, bound {bound:.2e}, "
          f"discounting gap {gap:.2e}")
    assert bound < gap / 3
    assert abs(v[0] - cf) <= bound


# ------------------------------------------------------------------ 8. closed form
def closed_form_points():
    """64 points: tau = 0 on both sides of and at the kink, deep in and out of
    the money, the corners of the stated domain, then random points of it."""
    rs = np.random.RandomState(21)
    S = np.concatenate([[1.5, 1.0, 0.5, 2.0, 0.5, 2.0, 0.5, 2.0, 0.5], rs.uniform(0.5, 2.0, 55)])
    v = np.concatenate([[0.2, 0.2, 0.2, 0.01, 0.01, 1.0, 1.0, 0.01, 1.0], rs.uniform(0.01, 1.0, 55)])
    tau = np.concatenate([[0.0, 0.0, 0.0, 0.05, 0.05, 2.0, 2.0, 2.0, 0.05], rs.uniform(0.05, 2.0, 55)])
    return S.astype(np.float32), v.astype(np.float32), tau.astype(np.float32)


@pytest.mark.parametrize("rho", [0.8, -0.7])
def test_closed_form_on_the_device(pkg, dev, rho):
    S, v, tau = closed_form_points()
    Tm = 2.0
    t = (np.float32(Tm) - tau).astype(np.float32)
    tau64 = Tm - t.astype(np.float64)                  # what the kernel sees
    want_p, want_d = h2.closed_form(S.astype(np.float64), v.astype(np.float64), tau64, rho=rho)
    X = torch.from_numpy(np.stack([S, v], 1)).to(dev)
    params = (h2.R_RATE, 1.0, 2.0, 0.2, 0.3, rho)
    p, d = pkg.exact("heston", torch.from_numpy(t).to(dev), X, Tm, params)
    p2, d2 = pkg.exact("heston", torch.from_numpy(t).to(dev), X, Tm, params)
    torch.cuda.synchronize()
    assert p.shape == (64, 1) and d.shape == (64, 1)
    p, d = p.cpu().numpy()[:, 0], d.cpu().numpy()[:, 0]
    print(f"rho={rho}: max|price err| = {np.abs(p - want_p).max():.3e}, max|delta err| = {np.abs(d - want_d).max():.3e}")
    np.testing.assert_allclose(p, want_p, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(d, want_d, rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(p[:3], [0.5, 0.0, 0.0])
    np.testing.assert_array_equal(d[:3], [1.0, 0.5, 0.0])
    np.testing.assert_array_equal(p2.cpu().numpy()[:, 0], p)
    np.testing.assert_array_equal(d2.cpu().numpy()[:, 0], d)


# ------------------------------------------------------------------ 9. the Python surface
def test_python_surface(pkg, dev):
    M = 24
    np.random.seed(3)
    m = pkg.HestonTwoFactorFBSNN(np.ones((1, 1)), T, M, N, 1, None, [2] + 4 * [16] + [1], "Naisnet", "Sine", device=dev)
    assert m.native_coefficients and m.spec.kind == "heston2" and m.solver.nb == 2 and m.state_dim == 2
    t, W = m.fetch_minibatch()
    assert t.shape == (M, N + 1, 1) and W.shape == (M, N + 1, 2)
    td, Wd = m.fetch_minibatch_device(seed=7)
    assert td.shape == (M, N + 1, 1) and Wd.shape == (M, N + 1, 2)
    opt = m.new_optimizer_state("Adam", 1e-3)
    before = m.params.clone()
    losses = [float(m.device_step(opt, 1e-3, seed=s)) for s in (3, 4)]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)) and float((m.params - before).abs().max()) > 0
    S, v, Y = m.predict(np.ones((1, 1)), t, W)
    assert S.shape == (M, N + 1, 1) and v.shape == (M, N + 1, 1) and Y.shape == (M, N + 1, 1)
    R = 5
    Sp, vp, tp = np.linspace(0.8, 1.2, R), np.full(R, 0.2), np.linspace(0.0, 0.8, R)
    val, err, none = m.mc_value(tp, np.stack([Sp, vp], 1), mc=2048)
    assert val.shape == (R, 1) and err.shape == (R, 1) and none is None
    price, delta = m.closed_form(Sp, vp, tp)
    assert price.shape == (R, 1) and delta.shape == (R, 1)
    assert float((price - val).abs().max()) < 0.05 and bool(((delta > 0) & (delta < 1)).all())
    terms = m.pde_residual(tp, np.stack([Sp, vp], 1))
    assert set(terms) == set(jr.TERMS) and all(x.shape == (R, 1) for x in terms.values())
    Yg, dl, gm = m.calculate_greeks(Sp, vp, tp)
    assert Yg.shape == (R, 1) and dl.shape == (R, 1) and gm.shape == (R,)
    pm, dm, gmm = m.mc_greeks(Sp, vp, tp, mc=2048)
    assert pm.shape == (R, 1) and dm.shape == (R, 1) and gmm.shape == (R, 1)
    m2 = pkg.HestonTwoFactorFBSNN(np.ones((1, 2)), T, M, N, 2, None, [3] + 4 * [16] + [1], "Naisnet", "Sine", device=dev)
    assert m2.solver.nb == 4
    with pytest.raises(ValueError, match="one asset"):
        m2.closed_form([1.0], [0.2], [0.0])
