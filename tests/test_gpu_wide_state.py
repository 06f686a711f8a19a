"""State dimensions above 126 (Dp = pad16(D + 2) in (128, 1024]): the per-layer
chain step with the column-tiled Z GEMM and the row kernel
(zrow_cotan_kernel), the split-K weight gradients at wide K, the path kernels
at wide rows and the wide correlated rollout (rollout_corrw_kernel).  Needs an
MI355X.

Every expectation is computed here, on the CPU, from oracle/fbsnn_ref.py and
oracle/philox.py.  Bounds are tests/test_gpu_parity.py's: X bit-exact, loss
rel 1e-4, Y / Z abs 1e-4 max(1, |ref|max), gradient abs 2e-4 max|ref grad|,
unused parameters exactly 0 (Heston X: rtol 1e-5 / atol 1e-6, the host's MKL
sqrt).  At these shapes the oracle's own fp32-vs-fp64 difference stays below
1 % of each bound, so a different fp32 summation order has room.

Shapes: Dp / 16 in {9, 13, 19, 32, 64} (the first block count past 8, a prime,
one that is no multiple of 8, the cap), R = M (N + 1) no multiple of 16, nb
just past 128.  ReLU is left out (kink flips between summation orders)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_pkg
from oracle import fbsnn_ref as fr
from oracle import philox as ph

pytestmark = pytest.mark.gpu
T = 1.0
FP32_ENV = {"DBSDE_X3": "0", "DBSDE_TNW_X3": "0"}


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def spec_for(pkg, problem, D):
    S = pkg.ProblemSpec
    return {
        "bsb": S(sig_a=0.4, phi_r=0.05, phi_c=1.0, g="sumsq"),
        "bspde_test": S(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=1.0, g="sumsq"),
        "call": S(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=1.0, g="call_sum", strike=1.0 * D),
        "basket": S(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=0.0, g="call_mean", strike=1.0),
        "hjb": S(sig_b=float(np.sqrt(2.0)), phi_zz=1.0, g="log"),
    }[problem]


def heston_spec(pkg, k):
    return pkg.ProblemSpec(kind="heston", mu_a=0.05, phi_r=0.05, g="call_mean", strike=1.0, g_alpha=10.0, g_cols=k,
                           u_clamp=True, q3=False, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8)


def make_solver(pkg, dev, mode, layers, act, spec, env=None):
    """env: variables set while the context is created."""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return pkg.NativeSolver(mode, layers, act, spec, T, dev)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def native(s, params, M, N, D, Xi, t, W, dev, want_grad=True):
    out = dict(loss=torch.empty(1, device=dev), X=torch.empty(M * (N + 1) * D, device=dev),
               Y=torch.empty(M * (N + 1), device=dev), Z=torch.empty(M * (N + 1) * D, device=dev))
    grad = torch.empty_like(params) if want_grad else None
    s.loss_grad(params, M, N, torch.as_tensor(Xi, dtype=torch.float32).to(dev).contiguous(),
                t=torch.as_tensor(t).float().to(dev).reshape(M, N + 1).contiguous(),
                W=torch.as_tensor(W).float().to(dev).contiguous(), grad=grad, **out)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    r["X"] = r["X"].reshape(M, N + 1, D)
    r["Z"] = r["Z"].reshape(M, N + 1, D)
    r["Y"] = r["Y"].reshape(M, N + 1, 1)
    if want_grad:
        r["grad"] = grad.cpu().numpy()
    return r


def check(r, ref, heston=False):
    for k in ("loss", "Y", "Z", "grad"):
        if k in r:
            a, b = np.asarray(r[k], np.float64).ravel(), np.asarray(ref[k], np.float64).ravel()
            print(f"{k}: max|err| = {np.abs(a - b).max():.3e}, max|ref| = {np.abs(b).max():.3e}")
    if heston:
        np.testing.assert_allclose(r["X"], ref["X"], rtol=1e-5, atol=1e-6)
    else:
        np.testing.assert_array_equal(r["X"], ref["X"])
    np.testing.assert_allclose(r["loss"][0], ref["loss"], rtol=1e-4)
    np.testing.assert_allclose(r["Y"], ref["Y"], rtol=0, atol=1e-4 * max(1.0, np.abs(ref["Y"]).max()))
    np.testing.assert_allclose(r["Z"], ref["Z"], rtol=0, atol=1e-4 * max(1.0, np.abs(ref["Z"]).max()))
    if "grad" in r:
        used = ref["used"]
        assert np.all(r["grad"][~used] == 0)
        np.testing.assert_allclose(r["grad"][used], ref["grad"][used], rtol=0, atol=2e-4 * np.abs(ref["grad"]).max())


# ------------------------------------------------------------------ 1. limits
@pytest.mark.parametrize("D", [127, 200, 510, 1022])
def test_solver_is_created_at_wide_D(pkg, dev, D):
    s = pkg.NativeSolver("NAIS-Net", [D + 1, 16, 16, 16, 16, 1], "Sine", spec_for(pkg, "bsb", D), T, dev)
    assert s.D == D and s.nb == D
    assert s.matrix_form == 0          # the fp32-input chain: no fused or split-bf16 form


def test_the_new_limit_is_reported(pkg, dev):
    with pytest.raises(ValueError, match="1022"):
        pkg.NativeSolver("NAIS-Net", [1024, 16, 16, 16, 16, 1], "Sine", spec_for(pkg, "bsb", 1023), T, dev)


def test_set_corr_accepts_129_and_mc_value_keeps_its_limit(pkg, dev):
    s = pkg.NativeSolver("NAIS-Net", [130, 16, 16, 16, 16, 1], "Sine", spec_for(pkg, "basket", 129), T, dev)
    s.set_corr(np.eye(129))
    s.set_corr(None)
    D = 200
    with pytest.raises(ValueError):
        pkg.mc_value(spec_for(pkg, "basket", D), torch.zeros(2, device=dev), torch.ones(2, D, device=dev), T, 4,
                     mc=256, L=np.eye(D))


# ------------------------------------------------------------------ 2. loss and gradient against the oracle
CASES = {
    "bsb127_nais48": ("bsb", "NAIS-Net", "Sine", 127, 48, 20, 3),
    "basket200_fc64": ("basket", "FC", "Tanh", 200, 64, 20, 3),
    "hjb300_resnet48": ("hjb", "Resnet", "Sine", 300, 48, 20, 3),
    "bsb510_fc96": ("bsb", "FC", "Tanh", 510, 96, 20, 2),
    "call1022_nais48": ("call", "NAIS-Net", "Sine", 1022, 48, 12, 2),
    "bspde144_naisnet32": ("bspde_test", "Naisnet", "Sine", 144, 32, 20, 3),
    "basket200_fc256": ("basket", "FC", "Tanh", 200, 256, 20, 3),
}
_REFS = {}


def reference(case):
    """Weights, batch and the oracle's results of one case, computed once and
    shared by the tests below (none of them changes it)."""
    if case not in _REFS:
        problem, mode, act, D, width, M, N = CASES[case]
        layers = [D + 1] + 4 * [width] + [1]
        torch.manual_seed(D + width)
        model = fr.build_model(mode, layers, act)
        params = fr.flat_params(model)
        t, W = fr.fetch_minibatch(M, N, D, T, rng=np.random.RandomState(7))
        Xi = np.zeros((1, D)) if problem == "hjb" else np.ones((1, D))
        ref = fr.loss_and_grads(model, fr.make_problem(problem, D), t, W, torch.as_tensor(Xi, dtype=torch.float32), M, D)
        _REFS[case] = dict(layers=layers, params=params, t=t.squeeze(-1).numpy(), W=W.numpy(), Xi=Xi, ref=ref)
    return _REFS[case]


def run_case(pkg, dev, case, env=None, want_grad=True):
    problem, mode, act, D, width, M, N = CASES[case]
    b = reference(case)
    s = make_solver(pkg, dev, mode, b["layers"], act, spec_for(pkg, problem, D), env)
    return native(s, torch.from_numpy(b["params"]).to(dev), M, N, D, b["Xi"], b["t"], b["W"], dev, want_grad)


@pytest.mark.parametrize("form", ["default", "fp32_env"])
@pytest.mark.parametrize("case", list(CASES))
def test_loss_grad_matches_oracle(pkg, dev, case, form):
    r = run_case(pkg, dev, case, FP32_ENV if form == "fp32_env" else None)
    check(r, reference(case)["ref"])
    r2 = run_case(pkg, dev, case, FP32_ENV if form == "fp32_env" else None)
    for k in ("loss", "Y", "Z", "grad"):          # fixed summation orders: a second call is bitwise equal
        np.testing.assert_array_equal(r[k], r2[k])


# ------------------------------------------------------------------ 3. forward only
@pytest.mark.parametrize("case", ["basket200_fc64", "call1022_nais48"])
def test_forward_only_loss(pkg, dev, case):
    full = run_case(pkg, dev, case)
    fwd = run_case(pkg, dev, case, want_grad=False)
    np.testing.assert_allclose(fwd["loss"][0], full["loss"][0], rtol=1e-6)
    np.testing.assert_allclose(fwd["loss"][0], reference(case)["ref"]["loss"], rtol=1e-4)


# ------------------------------------------------------------------ 4. train_step
@pytest.mark.parametrize("max_norm", [0.0, 1.0], ids=["adam", "adam_clip1"])
def test_train_step_equals_loss_grad_plus_optimizer_step(pkg, dev, max_norm):
    """Wide contexts take dbsde_train_step's two-call form; three steps give
    bit-identical parameters and moments to loss_grad + optimizer_step."""
    case = "basket200_fc64"
    problem, mode, act, D, width, M, N = CASES[case]
    b = reference(case)
    Xi = torch.ones(D, device=dev)
    res = []
    for fused in (True, False):
        s = make_solver(pkg, dev, mode, b["layers"], act, spec_for(pkg, problem, D))
        p = torch.from_numpy(b["params"]).to(dev).clone()
        g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
        state = torch.zeros(2, dtype=torch.float64, device=dev)
        loss = torch.empty(1, device=dev)
        for it in range(3):
            opt = dict(kind="Adam", lr=1e-3, max_norm=max_norm, step=it + 1, step_state=state, step_parity=it & 1)
            if fused:
                s.train_step(p, M, N, Xi, g, m, v, opt, seed=it, loss=loss)
            else:
                s.loss_grad(p, M, N, Xi, seed=it, grad=g, loss=loss)
                s.optimizer_step(p, g, m, v, **opt)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss))
        res.append((p.cpu(), m.cpu(), v.cpu(), state.cpu()))
    assert float((res[0][0] - torch.from_numpy(b["params"])).abs().max()) > 0
    for x, y in zip(*res):
        torch.testing.assert_close(x, y, rtol=0, atol=0)


# ------------------------------------------------------------------ 5. Heston
@pytest.mark.parametrize("k", [64, 100])
def test_heston_wide(pkg, dev, k):
    M, N = 16, 20
    layers = [1 + 2 * k, 16, 16, 16, 16, 1]
    s = pkg.NativeSolver("Naisnet", layers, "Sine", heston_spec(pkg, k), T, dev)
    assert s.nb == k
    Xi = np.concatenate([np.ones((1, k)), np.full((1, k), 0.2)], 1)
    # device mode: the rollout consumes the kernel's own increments
    _, dW = s.brownian(M, N, seed=2, increments=True)
    dW = dW.cpu().numpy()
    np.testing.assert_allclose(dW, ph.increments(2, 0, 0, M, N, k, T), rtol=2e-6, atol=2e-6)
    X = torch.empty(M * (N + 1) * 2 * k, device=dev)
    s.loss_grad(torch.zeros(s.nparams, device=dev), M, N, torch.as_tensor(Xi, dtype=torch.float32).to(dev), seed=2,
                loss=torch.empty(1, device=dev), X=X)
    torch.cuda.synchronize()
    Xr, _ = ph.heston_rollout(Xi, dW, T)
    np.testing.assert_array_equal(X.cpu().numpy().reshape(M, N + 1, 2 * k), Xr)
    # parity mode against the oracle
    torch.manual_seed(k)
    model = fr.build_heston_model("Naisnet", [2] + layers[1:], "Sine", k)
    params = fr.flat_params(model)
    t, W = fr.fetch_minibatch(M, N, k, T, rng=np.random.RandomState(7))
    ref = fr.heston_loss_and_grads(model, fr.Heston(k=k, payoff="discontinuous"), t, W, np.ones((1, k)), M)
    r = native(s, torch.from_numpy(params).to(dev), M, N, 2 * k, Xi, t.squeeze(-1), W, dev)
    check(r, ref, heston=True)


# ------------------------------------------------------------------ 6. device-mode diagonal rollout
def device_step(s, dev, params, M, N, Xi, seed, path0=0, grad=False):
    X = torch.empty(M * (N + 1) * s.D, device=dev)
    loss = torch.empty(1, device=dev)
    g = torch.empty_like(params) if grad else None
    s.loss_grad(params, M, N, Xi, seed=seed, path0=path0, loss=loss, X=X, grad=g)
    torch.cuda.synchronize()
    return X.cpu().numpy().reshape(M, N + 1, s.D), float(loss), (g.cpu().numpy() if grad else None)


@pytest.mark.parametrize("D", [200, 1022])
def test_device_rollout_wide(pkg, dev, D):
    s = pkg.NativeSolver("NAIS-Net", [D + 1, 16, 16, 16, 16, 1], "Sine", spec_for(pkg, "bsb", D), T, dev)
    M, N = 32, 50
    Xi_np = np.array([1.0, 0.5] * (D // 2))[None, :]
    Xi = torch.as_tensor(Xi_np, dtype=torch.float32).to(dev).contiguous()
    zero = torch.zeros(s.nparams, device=dev)
    _, dW = s.brownian(M, N, seed=9, increments=True)
    dW = dW.cpu().numpy()
    np.testing.assert_allclose(dW, ph.increments(9, 0, 0, M, N, D, T), rtol=2e-6, atol=2e-6)
    X, _, _ = device_step(s, dev, zero, M, N, Xi, 9)
    np.testing.assert_array_equal(X, ph.rollout(Xi_np, dW, T, 0.0, 0.4, 0.0))
    Xs, _, _ = device_step(s, dev, zero, 16, N, Xi, 9, path0=16)
    np.testing.assert_array_equal(Xs, X[16:])
    # a prefetched batch is the same step
    params = torch.from_numpy(np.random.RandomState(3).normal(scale=0.05, size=s.nparams).astype(np.float32)).to(dev)
    ref = device_step(s, dev, params, M, N, Xi, 5, grad=True)
    s.prefetch(M, N, Xi, seed=5)
    got = device_step(s, dev, params, M, N, Xi, 5, grad=True)
    np.testing.assert_array_equal(got[0], ref[0])
    assert got[1] == ref[1] and np.isfinite(ref[1])
    np.testing.assert_array_equal(got[2], ref[2])


# ------------------------------------------------------------------ 7. correlated device mode
@pytest.mark.parametrize("D", [129, 200, 510, 1022])
def test_correlated_device_mode_wide(pkg, dev, D):
    """with_corr...py:339-341: dW = L (sqrt(dt) z) by rollout_corrw_kernel."""
    rs = np.random.RandomState(D)
    A = rs.normal(size=(D, D))
    C = A @ A.T + D * np.eye(D)
    d = np.sqrt(np.diag(C))
    L = np.linalg.cholesky(C / np.outer(d, d))
    s = pkg.NativeSolver("NAIS-Net", [D + 1, 16, 16, 16, 16, 1], "Sine", spec_for(pkg, "basket", D), T, dev)
    s.set_corr(L)
    Xi_np = np.ones((1, D))
    Xi = torch.ones(D, device=dev)
    zero = torch.zeros(s.nparams, device=dev)
    N = 10
    for M in (24, 7):                  # 7: a partial path group
        t, dW = s.brownian(M, N, seed=4, increments=True)
        t2, W = s.brownian(M, N, seed=4)
        torch.cuda.synchronize()
        dW = dW.cpu().numpy()
        ref = ph.increments(4, 0, 0, M, N, D, T, L=L.astype(np.float32))
        scale = np.abs(ref).max()
        print(f"D={D} M={M}: max|dW err| = {np.abs(dW - ref).max():.3e} (bound {2e-6 * scale * np.sqrt(D):.3e})")
        np.testing.assert_allclose(dW, ref, rtol=0, atol=2e-6 * scale * np.sqrt(D))
        np.testing.assert_array_equal(t.cpu().numpy(), np.broadcast_to(ph.time_grid(N, T), (M, N + 1)))
        np.testing.assert_array_equal(t2.cpu().numpy(), t.cpu().numpy())
        np.testing.assert_array_equal(W.cpu().numpy(), ph.brownian_W(dW))
        X, _, _ = device_step(s, dev, zero, M, N, Xi, 4)
        np.testing.assert_array_equal(X, ph.rollout(Xi_np, dW, T, 0.05, 0.2, 0.0))
    # a shard draws what the full batch draws; a prefetched rollout is the same rollout
    Xs, _, _ = device_step(s, dev, zero, 8, N, Xi, 4, path0=16)
    X24, _, _ = device_step(s, dev, zero, 24, N, Xi, 4)
    np.testing.assert_array_equal(Xs, X24[16:])
    s.prefetch(24, N, Xi, seed=4)
    Xp, _, _ = device_step(s, dev, zero, 24, N, Xi, 4)
    np.testing.assert_array_equal(Xp, X24)
    s.set_corr(None)
    _, dWu = s.brownian(24, N, seed=4, increments=True)
    np.testing.assert_allclose(dWu.cpu().numpy(), ph.increments(4, 0, 0, 24, N, D, T), rtol=2e-6, atol=2e-6)


def test_correlated_device_mode_wide_on_a_caller_grid(pkg, dev):
    """A device-mode batch (W = NULL) with the caller's t on the wide correlated
    path (the Euler chains of rollout_chain_kernel on p.t): X is the oracle
    rollout of the drawn increments on that grid.  M = 17 is ragged against the
    16-path groups, the grid differs from path to path."""
    D, M, N = 130, 17, 5
    rs = np.random.RandomState(D)
    A = rs.normal(size=(D, D))
    C = A @ A.T + D * np.eye(D)
    d = np.sqrt(np.diag(C))
    s = pkg.NativeSolver("NAIS-Net", [D + 1, 16, 16, 16, 16, 1], "Sine", spec_for(pkg, "basket", D), T, dev)
    s.set_corr(np.linalg.cholesky(C / np.outer(d, d)))
    _, dW = s.brownian(M, N, seed=4, increments=True)
    tg = np.sort(rs.uniform(0, 1, size=(M, N + 1)), 1).astype(np.float32)
    tg[:, 0] = 0.0
    X = torch.empty(M * (N + 1) * D, device=dev)
    s.loss_grad(torch.zeros(s.nparams, device=dev), M, N, torch.ones(D, device=dev), t=torch.from_numpy(tg).to(dev),
                seed=4, X=X, loss=torch.empty(1, device=dev))
    torch.cuda.synchronize()
    ref = ph.rollout(np.ones((1, D)), dW.cpu().numpy(), T, 0.05, 0.2, 0.0, tgrid=tg)
    np.testing.assert_array_equal(X.cpu().numpy().reshape(M, N + 1, D), ref)
    assert not np.array_equal(ref, ph.rollout(np.ones((1, D)), dW.cpu().numpy(), T, 0.05, 0.2, 0.0))   # the grid is felt
