"""Correlated k-asset Heston in device mode: a Cholesky factor L [k, k] between
the assets' Brownian motions (dbsde_set_corr on a Heston context).  The
increment GEMM rollout_corrw_kernel at every k, the per-(path, asset) Euler
chain rollout_heston_chain_kernel, the fetch, prefetch and shards, the PDE
residual with the columns of Sigma(x) . L, and the FBSNN surface.  Needs an
MI355X.

Every expectation is computed on the CPU from oracle/philox.py,
oracle/fbsnn_ref.py and tests/heston_corr_reference.py.  Bounds: increments
2e-6 max|ref| sqrt(k) (the rule of tests/test_gpu_wide_state.py's
test_correlated_device_mode_wide: another fp32 summation order over k terms);
t, W and X bit-exact against the oracle run on the device's own increments;
loss / Y / Z / gradient as tests/test_gpu_wide_state.py's check(heston=True);
PDE terms as tests/test_gpu_jet.py's check_terms (2e-4 max|term|).

Shapes: N = 10 (crosses a 4-step Philox block and the chain's 8-step
look-ahead), M in {24, 7} (7: a partial 16-path group), k in {1, 3, 17, 50,
130}: one output block with seven idle waves, ragged blocks, a second output
block of wave 0."""
import ctypes
import os

import numpy as np
import pytest
import torch

import heston_corr_reference as hc
import jet_reference as jr
from conftest import load_pkg
from oracle import fbsnn_ref as fr
from oracle import philox as ph

pytestmark = pytest.mark.gpu
T, N = hc.T, hc.N
KS = [1, 3, 17, 50, 130]
MS = (24, 7)
SEED = 4
FP32_ENV = {"DBSDE_X3": "0", "DBSDE_TNW_X3": "0"}


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def heston_spec(pkg, k):
    return pkg.ProblemSpec(kind="heston", mu_a=0.05, phi_r=0.05, g="call_mean", strike=1.0, g_alpha=10.0, g_cols=k,
                           u_clamp=True, q3=False, **hc.HESTON)


def make_solver(pkg, dev, k, layers=None, env=None, L=None):
    """A Heston context (env: variables set while it is created), with L set."""
    layers = layers or [1 + 2 * k, 16, 16, 16, 16, 1]
    old = {n: os.environ.get(n) for n in (env or {})}
    os.environ.update(env or {})
    try:
        s = pkg.NativeSolver("Naisnet", layers, "Sine", heston_spec(pkg, k), T, dev)
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
    assert s.nb == k and s.D == 2 * k
    if L is not None:
        s.set_corr(L)
    return s


def xi_dev(dev, k):
    return torch.as_tensor(hc.xi_state(k), dtype=torch.float32).to(dev).contiguous()


def device_step(s, dev, params, M, xi, seed, path0=0, grad=False):
    """(X [M, N+1, 2k], loss, grad) of a device-mode loss_grad."""
    X = torch.empty(M * (N + 1) * s.D, device=dev)
    loss = torch.empty(1, device=dev)
    g = torch.empty_like(params) if grad else None
    s.loss_grad(params, M, N, xi, seed=seed, path0=path0, loss=loss, X=X, grad=g)
    torch.cuda.synchronize()
    return X.cpu().numpy().reshape(M, N + 1, s.D), float(loss), (g.cpu().numpy() if grad else None)


_SOLVERS = {}


def corr_solver(pkg, dev, k):
    """The correlated 16-wide context of k, created once (no test leaves it
    with another factor)."""
    if k not in _SOLVERS:
        _SOLVERS[k] = make_solver(pkg, dev, k, L=hc.random_factor(k))
    return _SOLVERS[k]


def random_params(s, dev, seed=3, scale=0.3):
    return torch.from_numpy(np.random.RandomState(seed).normal(scale=scale, size=s.nparams).astype(np.float32)).to(dev)


# ------------------------------------------------------------------ 1. increments
@pytest.mark.parametrize("k", KS)
def test_increments_t_and_W(pkg, dev, k):
    s, L = corr_solver(pkg, dev, k), hc.random_factor(k)
    for M in MS:
        t, dW = s.brownian(M, N, seed=SEED, increments=True)
        t2, W = s.brownian(M, N, seed=SEED)
        torch.cuda.synchronize()
        dW = dW.cpu().numpy()
        assert dW.shape == (M, N, k)
        ref = ph.increments(SEED, 0, 0, M, N, k, T, L=L.astype(np.float32))
        bound = 2e-6 * float(np.abs(ref).max()) * np.sqrt(k)
        print(f"k={k} M={M}: max|dW err| = {np.abs(dW - ref).max():.3e} (bound {bound:.3e})")
        np.testing.assert_allclose(dW, ref, rtol=0, atol=bound)
        if k > 1:      # the factor is applied: the uncorrelated draws are far outside the bound
            assert np.abs(dW - ph.increments(SEED, 0, 0, M, N, k, T)).max() > 100 * bound
        np.testing.assert_array_equal(t.cpu().numpy(), np.broadcast_to(ph.time_grid(N, T), (M, N + 1)))
        np.testing.assert_array_equal(t2.cpu().numpy(), t.cpu().numpy())
        np.testing.assert_array_equal(W.cpu().numpy(), ph.brownian_W(dW))


# ------------------------------------------------------------------ 2. paths
@pytest.mark.parametrize("k", KS)
def test_paths_are_the_oracle_rollout_of_the_device_increments(pkg, dev, k):
    s = corr_solver(pkg, dev, k)
    zero = torch.zeros(s.nparams, device=dev)
    for M in MS:
        _, dW = s.brownian(M, N, seed=SEED, increments=True)
        X, _, _ = device_step(s, dev, zero, M, xi_dev(dev, k), SEED)
        Xr, _ = ph.heston_rollout(hc.xi_state(k), dW.cpu().numpy(), T, **hc.HESTON)
        np.testing.assert_array_equal(X, Xr)


def test_paths_on_a_caller_grid(pkg, dev):
    """A device-mode batch (W = NULL) with the caller's t (rollout_heston_chain_kernel
    on p.t): X is the oracle rollout of the drawn increments on that grid.  M = 17
    is ragged against the 16-path groups, the grid differs from path to path."""
    k, M, Ng = 3, 17, 5
    s = corr_solver(pkg, dev, k)
    _, dW = s.brownian(M, Ng, seed=SEED, increments=True)
    tg = np.sort(np.random.RandomState(k).uniform(0, 1, size=(M, Ng + 1)), 1).astype(np.float32)
    tg[:, 0] = 0.0
    X = torch.empty(M * (Ng + 1) * s.D, device=dev)
    s.loss_grad(torch.zeros(s.nparams, device=dev), M, Ng, xi_dev(dev, k), t=torch.from_numpy(tg).to(dev), seed=SEED,
                X=X, loss=torch.empty(1, device=dev))
    torch.cuda.synchronize()
    Xr, _ = ph.heston_rollout(hc.xi_state(k), dW.cpu().numpy(), T, tgrid=tg, **hc.HESTON)
    np.testing.assert_array_equal(X.cpu().numpy().reshape(M, Ng + 1, 2 * k), Xr)
    assert not np.array_equal(Xr, ph.heston_rollout(hc.xi_state(k), dW.cpu().numpy(), T, **hc.HESTON)[0])   # the grid is felt


# ------------------------------------------------------------------ 3. identity and clearing
@pytest.mark.parametrize("k", [3, 50])
def test_identity_factor_and_clearing(pkg, dev, k):
    s = make_solver(pkg, dev, k)
    zero, xi, M = torch.zeros(s.nparams, device=dev), xi_dev(dev, k), 24
    X0, _, _ = device_step(s, dev, zero, M, xi, SEED)
    s.set_corr(np.eye(k))                 # products with 1 and sums with 0 are exact
    X1, _, _ = device_step(s, dev, zero, M, xi, SEED)
    np.testing.assert_array_equal(X1, X0)
    s.set_corr(hc.random_factor(k))
    X2, _, _ = device_step(s, dev, zero, M, xi, SEED)
    assert np.abs(X2 - X0).max() > 1e-3
    s.set_corr(None)
    X3, _, _ = device_step(s, dev, zero, M, xi, SEED)
    np.testing.assert_array_equal(X3, X0)
    with pytest.raises(ValueError):
        s.set_corr(np.eye(2 * k))
    # the library's own check (the wrapper above stops at the shape)
    big = np.ascontiguousarray(np.eye(2 * k, dtype=np.float32))
    rc = s.lib.dbsde_set_corr(s.ctx, big.ctypes.data_as(ctypes.c_void_p), 2 * k)
    assert rc == -1                       # DBSDE_EINVAL
    X4, _, _ = device_step(s, dev, zero, M, xi, SEED)
    np.testing.assert_array_equal(X4, X0)


# ------------------------------------------------------------------ 4. shards and prefetch
@pytest.mark.parametrize("k", [3, 130])
def test_shards_and_prefetch(pkg, dev, k):
    s = corr_solver(pkg, dev, k)
    zero, xi = torch.zeros(s.nparams, device=dev), xi_dev(dev, k)
    X24, _, _ = device_step(s, dev, zero, 24, xi, SEED)
    Xs, _, _ = device_step(s, dev, zero, 8, xi, SEED, path0=16)
    np.testing.assert_array_equal(Xs, X24[16:])
    params = random_params(s, dev, scale=0.05)
    ref = device_step(s, dev, params, 24, xi, 5, grad=True)
    other = device_step(s, dev, params, 24, xi, 6, grad=True)
    assert np.isfinite(ref[1]) and np.abs(ref[2]).max() > 0
    # prefetched, consumed by the next step
    s.prefetch(24, N, xi, seed=5)
    got = device_step(s, dev, params, 24, xi, 5, grad=True)
    # prefetched, held back over a step of another batch, then consumed
    s.prefetch(24, N, xi, seed=5)
    mid = device_step(s, dev, params, 24, xi, 6, grad=True)
    late = device_step(s, dev, params, 24, xi, 5, grad=True)
    for a, b in ((got, ref), (late, ref), (mid, other)):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1]
        np.testing.assert_array_equal(a[2], b[2])


# ------------------------------------------------------------------ 5. loss and gradient
def check(r, ref):
    """tests/test_gpu_wide_state.py's check(heston=True)."""
    for key in ("loss", "Y", "Z", "grad"):
        a, b = np.asarray(r[key], np.float64).ravel(), np.asarray(ref[key], np.float64).ravel()
        print(f"{key}: max|err| = {np.abs(a - b).max():.3e}, max|ref| = {np.abs(b).max():.3e}")
    xe = np.abs(r["X"] - ref["X"])
    print(f"X: max|err| = {xe.max():.3e}, max err / (1e-6 + 1e-5 |ref|) = {(xe / (1e-6 + 1e-5 * np.abs(ref['X']))).max():.3f}")
    np.testing.assert_allclose(r["X"], ref["X"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["loss"][0], ref["loss"], rtol=1e-4)
    np.testing.assert_allclose(r["Y"], ref["Y"], rtol=0, atol=1e-4 * max(1.0, np.abs(ref["Y"]).max()))
    np.testing.assert_allclose(r["Z"], ref["Z"], rtol=0, atol=1e-4 * max(1.0, np.abs(ref["Z"]).max()))
    used = ref["used"]
    assert np.all(r["grad"][~used] == 0)
    np.testing.assert_allclose(r["grad"][used], ref["grad"][used], rtol=0, atol=2e-4 * np.abs(ref["grad"]).max())


_LOSS_REFS = {}


def loss_reference(case, t, W):
    """The oracle on the device's exported (t, W) of a case, computed once
    (both matrix forms export the same batch: the path kernels are the same)."""
    if case not in _LOSS_REFS:
        k, _, M, _ = hc.LOSS_CASES[case]
        _, model, _ = hc.loss_case_model(case)
        ref = fr.heston_loss_and_grads(model, fr.Heston(k=k), torch.from_numpy(t)[..., None], torch.from_numpy(W),
                                       np.ones((1, k)), M)
        _LOSS_REFS[case] = (t, W, ref)
    t0, W0, ref = _LOSS_REFS[case]
    np.testing.assert_array_equal(t, t0)
    np.testing.assert_array_equal(W, W0)
    return ref


@pytest.mark.parametrize("form", ["default", "fp32_env"])
@pytest.mark.parametrize("case", list(hc.LOSS_CASES))
def test_loss_and_gradient_match_oracle(pkg, dev, case, form):
    k, _, M, seed = hc.LOSS_CASES[case]
    layers, _, flat = hc.loss_case_model(case)
    s = make_solver(pkg, dev, k, layers, FP32_ENV if form == "fp32_env" else None, L=hc.random_factor(k))
    print(f"{case} {form}: matrix_form = {s.matrix_form}")
    t, W = s.brownian(M, N, seed=seed)
    torch.cuda.synchronize()
    ref = loss_reference(case, t.cpu().numpy(), W.cpu().numpy())
    params = torch.from_numpy(flat.astype(np.float32)).to(dev)
    out = dict(loss=torch.empty(1, device=dev), X=torch.empty(M * (N + 1) * 2 * k, device=dev),
               Y=torch.empty(M * (N + 1), device=dev), Z=torch.empty(M * (N + 1) * 2 * k, device=dev))
    grad = torch.empty_like(params)
    s.loss_grad(params, M, N, xi_dev(dev, k), seed=seed, grad=grad, **out)
    torch.cuda.synchronize()
    r = {n: v.cpu().numpy() for n, v in out.items()}
    r["X"], r["Z"] = r["X"].reshape(M, N + 1, 2 * k), r["Z"].reshape(M, N + 1, 2 * k)
    r["Y"], r["grad"] = r["Y"].reshape(M, N + 1, 1), grad.cpu().numpy()
    check(r, ref)


# ------------------------------------------------------------------ 6. / 7. the FBSNN object
_OBJ = {}


def heston_object(pkg, dev):
    """HestonFBSNN(k = 3, "random_correlation") on the weights and points of
    hc.pde_setup (tests/test_gpu_jet.py's heston_setup recipe: about half of
    the rows clamp), created once."""
    if not _OBJ:
        k = hc.PDE_K
        oracle, flat, t, X, clamped = hc.pde_setup()
        np.random.seed(hc.PDE_SEED)
        m = pkg.HestonFBSNN(np.ones((1, k)), T, 24, N, k, None, [2] + 4 * [16] + [1], "Naisnet", "Tanh",
                            correlation_type="random_correlation", device=dev)
        assert m.native_coefficients
        assert list(m.model.state_dict())[-1].endswith("bias")
        np.testing.assert_array_equal(m._L, hc.object_factor(pkg))
        assert np.abs(np.tril(m._L, -1)).max() > 0
        _OBJ.update(m=m, oracle=oracle, flat=flat, t=t, X=X, clamped=clamped)
    m = _OBJ["m"]
    m.params.copy_(torch.from_numpy(_OBJ["flat"]).to(dev))
    return _OBJ


def test_pde_residual_of_a_correlated_object(pkg, dev):
    o = heston_object(pkg, dev)
    m, t, X, clamped = o["m"], o["t"], o["X"], o["clamped"]
    want = hc.pde_terms(o["oracle"], t, X, hc.PDE_K, L=m._L, kappa=m.kappa, theta=m.theta, sigma=m.sigma, rho=m.rho)
    got = m.pde_residual(t, X)
    torch.cuda.synchronize()
    # tests/test_gpu_jet.py's check_terms
    assert set(got) == set(jr.TERMS)
    smax = float(np.abs(want["scale"]).max())
    for key in jr.TERMS:
        g = got[key].cpu().numpy()
        assert g.shape == want[key].shape, (key, g.shape)
        top = smax if key == "residual" else float(np.abs(want[key]).max())
        err = float(np.abs(g - want[key]).max())
        print(f"{key}: max|err| = {err:.3e} = {err / top:.3e} max|ref| (bound 2e-04)")
        assert top > 0 and np.all(np.isfinite(g))
        np.testing.assert_allclose(g, want[key], rtol=0, atol=2e-4 * top)
        assert np.all(g[clamped] == 0), key


def test_python_surface(pkg, dev):
    m = heston_object(pkg, dev)["m"]
    k, M = hc.PDE_K, 24
    t, W = m.fetch_minibatch_device(seed=7)
    assert t.shape == (M, N + 1, 1) and W.shape == (M, N + 1, k)
    np.testing.assert_array_equal(W.cpu().numpy(), ph.brownian_W(
        m.solver.brownian(M, N, seed=7, increments=True)[1].cpu().numpy()))
    xi = m._device_xi(0, M)
    want = torch.empty(1, device=dev)
    m.solver.loss_grad(m.params, M, N, xi, seed=3, loss=want, grad=torch.empty_like(m.params))
    opt = m.new_optimizer_state("Adam", 1e-3)
    before = m.params.clone()
    loss = m.device_step(opt, 1e-3, seed=3).clone()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and float(loss) == float(want)
    assert float((m.params - before).abs().max()) > 0
    m.train_device(3, 1e-3)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(m.params).all())
    assert m.N == N                       # (no N schedule: Mm is None)
