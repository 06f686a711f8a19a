"""The arithmetic-average (Asian) problem on the device (problem kind 4,
ProblemSpec(average=True)): rollout_asian_chain_kernel / rollout_asian_avg_kernel
in every role (increments, paths, the caller's grid and W, shards, prefetch, a
factor), the loss and gradient on every network form, the PDE residual, the
Monte-Carlo comparator and the problem classes.  Needs an MI355X.

Every expectation is computed on the CPU from oracle/philox.py,
oracle/fbsnn_ref.py and tests/asian_reference.py (held to references of its
own by tests/test_asian_cpu.py).

Shapes: k in {1, 3, 17, 70, 130} (the fused width-16 row; a ragged 16-block;
Dp > 128: the wide chain), M in {24, 7}, N = 6 (the last 4-step Philox block is
half used).  Bounds: increments the documented normal error (rtol = atol =
2e-6, tests/test_gpu_device_rng.py); paths bit-equal to the numpy chain on the
device's own increments; loss / Y / Z / gradient tests/depth_cases.py's BOUNDS
(the put tests' bounds) with tests/test_gpu_heston2.py's bound on X; PDE terms
tests/test_gpu_jet.py's 1e-4 / 2e-4 of max|ref|; Monte-Carlo tests/test_gpu_mc.py's
RTOL, ATOL = 2e-5, 2e-6 and kink slack."""
import os

import numpy as np
import pytest
import torch

import asian_reference as ar
import depth_cases as dc
import jet_reference as jr
import path_cases as pc
from conftest import load_pkg
from oracle import philox as ph

pytestmark = pytest.mark.gpu
T, N = ar.T, ar.N
KS = list(ar.KS)
MS = ar.MS
SEED = 4
RTOL, ATOL = 2e-5, 2e-6
ENV_KEYS = ("DBSDE_FUSED", "DBSDE_TNW", "DBSDE_X3", "DBSDE_TNW_X3", "DBSDE_CS", "DBSDE_CHUNKS", "DBSDE_W256",
            "DBSDE_TNW_ORDER")


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def make_solver(pkg, dev, k, mode="Naisnet", layers=None, env=None, act="Sine", spec=None):
    """A context of the kind (env holds while it is created, every other path switch unset)."""
    layers = layers or [k + 2, 16, 16, 16, 16, 1]
    old = {n: os.environ.pop(n, None) for n in ENV_KEYS}
    os.environ.update(env or {})
    try:
        s = pkg.NativeSolver(mode, layers, act, spec or ar.spec(pkg), T, dev)
    finally:
        for n, v in old.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v
    assert s.D == k + 1 and s.nb == k
    return s


_SOLVERS = {}


def solver(pkg, dev, k):
    if k not in _SOLVERS:
        _SOLVERS[k] = make_solver(pkg, dev, k)
    return _SOLVERS[k]


def xi_dev(dev, k, rows=1):
    xi = np.repeat(ar.xi_state(k), rows, 0)
    if rows > 1:                                                     # per-path states: A_0 and the prices differ
        xi = xi * np.linspace(0.8, 1.2, rows)[:, None] + np.concatenate([[[0.1]], np.zeros((1, k))], 1)
    return torch.as_tensor(xi, dtype=torch.float32).to(dev).contiguous()


def paths(s, dev, params, M, xi, seed, path0=0, grad=False, t=None, W=None, n=N):
    """(X [M, n+1, D], loss, grad or None) of a loss_grad into NaN-filled outputs."""
    X = torch.full((M * (n + 1) * s.D,), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    g = torch.full_like(params, float("nan")) if grad else None
    s.loss_grad(params, M, n, xi, seed=seed, path0=path0, loss=loss, X=X, grad=g, t=t, W=W)
    torch.cuda.synchronize()
    return X.cpu().numpy().reshape(M, n + 1, s.D), float(loss), (g.cpu().numpy() if grad else None)


def dirty_path_buffer(s, dev, M):
    """NaN into the rows the next rollout of this shape writes
    (tests/test_gpu_path_kernels.py's recipe): a device-mode step with Xi = NaN
    leaves NaN in every state column of xin and in the S columns of sdw, a
    net_u call with t = X = NaN in the t and state columns of xin, and a
    net_u_vjp with zbar = NaN -- on the fused contexts, whose phase C reads the
    cotangent from the sdw rows -- in every state column of sdw, the A column
    included.  No prefetch is pending, so all of them and the measured rollout
    use path buffer 0."""
    D, R = s.D, M * (N + 1)
    par = torch.zeros(s.nparams, device=dev)
    nan = lambda n: torch.full((n,), float("nan"), device=dev)
    s.loss_grad(par, M, N, nan(D), seed=77, loss=torch.empty(1, device=dev))
    s.net_u(par, nan(R), nan(R * D), torch.empty(R, device=dev), torch.empty(R * D, device=dev))
    s.net_u_vjp(par, torch.zeros(R, device=dev), torch.ones(R * D, device=dev), torch.zeros(R, device=dev), nan(R * D),
                torch.empty(s.nparams, device=dev))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 1. increments and paths
@pytest.mark.parametrize("k", KS)
def test_increments_t_and_W(pkg, dev, k):
    s = solver(pkg, dev, k)
    for M in MS:
        t, dW = s.brownian(M, N, seed=SEED, increments=True)
        t2, W = s.brownian(M, N, seed=SEED)
        torch.cuda.synchronize()
        dW = dW.cpu().numpy()
        assert dW.shape == (M, N, k)
        ref = ph.increments(SEED, 0, 0, M, N, k, T)
        print(f"k={k} M={M}: max|dW err| = {np.abs(dW - ref).max():.3e}, max|ref| = {np.abs(ref).max():.3e}")
        np.testing.assert_allclose(dW, ref, rtol=2e-6, atol=2e-6)
        np.testing.assert_array_equal(t.cpu().numpy(), np.broadcast_to(ph.time_grid(N, T), (M, N + 1)))
        np.testing.assert_array_equal(t2.cpu().numpy(), t.cpu().numpy())
        np.testing.assert_array_equal(W.cpu().numpy(), ph.brownian_W(dW))


@pytest.mark.parametrize("k", KS)
def test_paths_are_the_chain_on_the_device_increments(pkg, dev, k):
    """X bit-equal to the numpy chain out of NaN-filled path buffers.  The
    sigma dW rows have no export: their S values are diag_step's other result,
    pinned through X; a NaN left in any of their columns -- the A column, which
    must be rewritten with 0, included -- makes the loss NaN (0 . NaN), and the
    loss of the zero network is sum g(A_N)^2 + sum g'(A_N)^2 exactly."""
    s = solver(pkg, dev, k)
    zero = torch.zeros(s.nparams, device=dev)
    for M in MS:
        dirty_path_buffer(s, dev, M)
        _, dW = s.brownian(M, N, seed=SEED, increments=True)
        X, loss, _ = paths(s, dev, zero, M, xi_dev(dev, k), SEED)
        Xr, sdw = ar.rollout(ar.xi_state(k), dW.cpu().numpy(), T, **ar.COEF)
        np.testing.assert_array_equal(X, Xr)
        assert np.all(sdw[:, :, 0] == 0)
        assert Xr[:, -1, 0].min() > 0.5 and np.ptp(Xr[:, -1, 0]) > 1e-3          # the average moved, path by path
        a = Xr[:, -1, 0].astype(np.float64) - 1.0
        want = np.sum(np.maximum(a, 0.0) ** 2) + np.sum((a > 0) * 1.0)
        np.testing.assert_allclose(loss, want, rtol=1e-5)


@pytest.mark.parametrize("k", [1, 17, 130])
def test_callers_grid_and_W(pkg, dev, k):
    """The caller's t / W [M, N+1, k]: a non-uniform grid per path, W of the
    device's own draws; the chain on the fp32 differences.  And the caller's
    grid alone (W = None): the device's increments on that grid."""
    s = solver(pkg, dev, k)
    zero, M = torch.zeros(s.nparams, device=dev), 7
    xi = xi_dev(dev, k, rows=M)
    _, W = s.brownian(M, N, seed=SEED)
    _, dW = s.brownian(M, N, seed=SEED, increments=True)
    torch.cuda.synchronize()
    rs = np.random.RandomState(k)
    tg = np.concatenate([np.zeros((M, 1)), np.cumsum(rs.uniform(0.5, 1.5, (M, N)), 1)], 1)
    tg = (tg / tg[:, -1:] * T).astype(np.float32)
    td = torch.from_numpy(tg).to(dev).contiguous()
    Xp, _, _ = paths(s, dev, zero, M, xi, SEED, t=td, W=W.contiguous())
    Wn = W.cpu().numpy()
    Xr, _ = ar.rollout(xi.cpu().numpy(), Wn[:, 1:] - Wn[:, :-1], T, tgrid=tg, **ar.COEF)
    np.testing.assert_array_equal(Xp, Xr)
    Xg, _, _ = paths(s, dev, zero, M, xi, SEED, t=td)
    Xr2, _ = ar.rollout(xi.cpu().numpy(), dW.cpu().numpy(), T, tgrid=tg, **ar.COEF)
    np.testing.assert_array_equal(Xg, Xr2)
    assert np.any(Xg != Xp)


@pytest.mark.parametrize("k", [3, 70, 130])
def test_shards_and_prefetch(pkg, dev, k):
    """An odd path0; three shards equal one device; a prefetched step, consumed
    at once or held back over a step of another batch, equals an in-step one
    bit for bit (paths, loss and gradient)."""
    s = solver(pkg, dev, k)
    zero, xi = torch.zeros(s.nparams, device=dev), xi_dev(dev, k)
    X24, _, _ = paths(s, dev, zero, 24, xi, SEED)
    parts = [paths(s, dev, zero, m, xi, SEED, path0=p0)[0] for p0, m in ((0, 7), (7, 9), (16, 8))]
    np.testing.assert_array_equal(np.concatenate(parts), X24)
    torch.manual_seed(k)
    params = (0.3 * torch.randn(s.nparams)).to(dev)
    ref = paths(s, dev, params, 24, xi, 5, grad=True)
    other = paths(s, dev, params, 24, xi, 6, grad=True)
    assert np.isfinite(ref[1]) and np.abs(ref[2]).max() > 0
    s.prefetch(24, N, xi, seed=5)
    got = paths(s, dev, params, 24, xi, 5, grad=True)
    s.prefetch(24, N, xi, seed=5)
    mid = paths(s, dev, params, 24, xi, 6, grad=True)
    late = paths(s, dev, params, 24, xi, 5, grad=True)
    for a, b in ((got, ref), (late, ref), (mid, other)):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1]
        np.testing.assert_array_equal(a[2], b[2])


# ------------------------------------------------------------------ 2. with a factor
@pytest.mark.parametrize("k", [3, 17, 130])
def test_a_factor_correlates_the_assets(pkg, dev, k):
    """The increments equal oracle.philox.increments(..., L) = L dz within
    tests/path_cases.py's corr_bound (the draws' error through L plus the fp32
    summation);
    X is bit-equal to the chain on the device's own increments (device grid
    and the caller's); L = I gives the uncorrelated bits; shards and a
    prefetched step as without a factor."""
    s = make_solver(pkg, dev, k)
    zero, xi = torch.zeros(s.nparams, device=dev), xi_dev(dev, k)
    plain = {M: paths(s, dev, zero, M, xi, SEED)[0] for M in MS}
    L = ar.equicorr_L(k, 0.3) if k < 100 else np.linalg.cholesky(
        0.5 * np.eye(k) + 0.5 * np.exp(-np.abs(np.subtract.outer(np.arange(k), np.arange(k))) / 7.0)).astype(np.float32)
    s.set_corr(np.eye(k, dtype=np.float32))
    for M in MS:
        np.testing.assert_array_equal(paths(s, dev, zero, M, xi, SEED)[0], plain[M])
    s.set_corr(L)
    for M in MS:
        dirty_path_buffer(s, dev, M)
        t, dW = s.brownian(M, N, seed=SEED, increments=True)
        _, W = s.brownian(M, N, seed=SEED)
        torch.cuda.synchronize()
        dW = dW.cpu().numpy()
        dz = ph.increments(SEED, 0, 0, M, N, k, T)
        ratio = float((np.abs(dW.astype(np.float64) - pc.corr_ref(L, dz)) / pc.corr_bound(L, dz)).max())
        print(f"k={k} M={M}: max |dW - L dz| / bound = {ratio:.4f}")
        assert ratio <= 1.0
        np.testing.assert_array_equal(W.cpu().numpy(), ph.brownian_W(dW))
        X, _, _ = paths(s, dev, zero, M, xi, SEED)
        Xr, _ = ar.rollout(ar.xi_state(k), dW, T, **ar.COEF)
        np.testing.assert_array_equal(X, Xr)
        assert np.any(X != plain[M])
    M = 7
    tg = np.broadcast_to((ph.time_grid(N, T).astype(np.float64) ** 1.5).astype(np.float32), (M, N + 1)).copy()
    _, dW = s.brownian(M, N, seed=SEED, increments=True)
    Xg, _, _ = paths(s, dev, zero, M, xi, SEED, t=torch.from_numpy(tg).to(dev))
    np.testing.assert_array_equal(Xg, ar.rollout(ar.xi_state(k), dW.cpu().numpy(), T, tgrid=tg, **ar.COEF)[0])
    X24, _, _ = paths(s, dev, zero, 24, xi, SEED)
    parts = [paths(s, dev, zero, m, xi, SEED, path0=p0)[0] for p0, m in ((0, 7), (7, 17))]
    np.testing.assert_array_equal(np.concatenate(parts), X24)
    s.prefetch(24, N, xi, seed=SEED)
    np.testing.assert_array_equal(paths(s, dev, zero, 24, xi, SEED)[0], X24)


# ------------------------------------------------------------------ 3. loss and gradient
_LOSS_REFS = {}


def loss_reference(case, dW):
    """The fp64 oracle on the device's own increments, once per network and batch
    (the cases of one network draw the same batch: the path kernels are the same)."""
    k, M = ar.LOSS_CASES[case][:2]
    key = (k, M, tuple(ar.loss_layers(case)))
    if key not in _LOSS_REFS:
        model, _ = ar.loss_model(case)
        prob = ar.AsianProblem(k, "call_mean", ar.LOSS_STRIKE)
        ref = ar.loss_and_grads(model, prob, ph.time_grid(N, T), dW, ar.xi_state(k))
        _LOSS_REFS[key] = (dW, dict(ref64=ref, tensors=dc.tensors(model)))
    np.testing.assert_array_equal(dW, _LOSS_REFS[key][0])
    return _LOSS_REFS[key][1]


@pytest.mark.parametrize("case", list(ar.LOSS_CASES))
def test_loss_and_gradient_match_the_fp64_oracle(pkg, dev, case):
    """Loss, Y, Z and every gradient tensor within tests/depth_cases.py's BOUNDS
    of the fp64 oracle, X within tests/test_gpu_heston2.py's rtol 1e-5 / atol
    1e-6 of it (and bit-equal to the numpy chain), unused gradient elements 0;
    the context runs the kernels the case names."""
    k, M, mode, act, _, env = ar.LOSS_CASES[case]
    layers = ar.loss_layers(case)
    _, flat = ar.loss_model(case)
    s = make_solver(pkg, dev, k, mode, layers, env, act, ar.spec(pkg, "call_mean", ar.LOSS_STRIKE))
    seed = ar.LOSS_SEED + k
    _, dW = s.brownian(M, N, seed=seed, increments=True)
    torch.cuda.synchronize()
    b = loss_reference(case, dW.cpu().numpy())
    params = torch.from_numpy(flat.astype(np.float32)).to(dev)
    D = k + 1
    nan = lambda n: torch.full((n,), float("nan"), device=dev)
    out = dict(loss=nan(1), X=nan(M * (N + 1) * D), Y=nan(M * (N + 1)), Z=nan(M * (N + 1) * D))
    grad = torch.full_like(params, float("nan"))
    s.profile(True)
    s.loss_grad(params, M, N, xi_dev(dev, k), seed=seed, grad=grad, **out)
    torch.cuda.synchronize()
    names = set(s.profile_read())
    s.profile(False)
    r = {n: v.cpu().numpy() for n, v in out.items()}
    r["X"], r["Z"] = r["X"].reshape(M, N + 1, D), r["Z"].reshape(M, N + 1, D)
    r["Y"], r["grad"] = r["Y"].reshape(M, N + 1, 1), grad.cpu().numpy()
    print(f"{case}: matrix_form {s.matrix_form}, ran {sorted(names)}")
    assert {"asian_chain", "asian_avg"} <= names
    fused = "fused_fwd_inputgrad" in names
    assert fused == case.startswith("fused"), sorted(names)
    if case.startswith("fused110"):
        assert (s.matrix_form & 1) == (1 if case.endswith("x3") else 0)
    if case == "wide_k130":
        assert "z_row_cotangent" in names, sorted(names)
    ref = b["ref64"]
    for key in ("loss", "X", "Y", "Z", "grad"):
        assert np.all(np.isfinite(r[key])), key
    e = dc.errors(r, ref, b["tensors"])
    print(f"{case}: error / bound: " + ", ".join(f"{n} {v:.3g}" if not isinstance(v, str) else f"({v})" for n, v in e.items()))
    np.testing.assert_allclose(r["X"], ref["X"], rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(r["X"], ar.rollout(ar.xi_state(k), dW.cpu().numpy(), T, **ar.COEF)[0])
    assert np.all(r["grad"][~ref["used"]] == 0)
    for key in ("loss", "Y", "Z", "grad", "tensor"):
        assert e[key] <= 1.0, f"{case}: {key} is {e[key]:.3g} of its bound ({e['tensor_name']})"
    assert np.abs(ref["Z"][:, :, 0]).max() > 1e-3                                  # u_A is there to be wrong


# ------------------------------------------------------------------ 4. PDE residual
def native_terms(s, dev, flat, t, X):
    R = X.shape[0]
    out = {key: torch.empty(R, device=dev) for key in jr.TERMS}
    s.pde_residual(torch.from_numpy(flat).to(dev), torch.from_numpy(t.ravel().astype(np.float32)).to(dev),
                   torch.from_numpy(X.astype(np.float32)).to(dev).contiguous(), **out)
    torch.cuda.synchronize()
    return {key: v.cpu().numpy().reshape(R, 1) for key, v in out.items()}


@pytest.mark.parametrize("k,corr", [(1, False), (3, False), (3, True), (70, False), (70, True)],
                         ids=["k1", "k3", "k3-factor", "k70", "k70-factor"])
def test_pde_residual_terms(pkg, dev, k, corr):
    """R = 12 random points against double autograd: u, u_t, drift and phi
    within 1e-4 of max|ref|, the diffusion within 2e-4, the residual within 2e-4
    of max(scale) (tests/test_gpu_jet.py).  T = 0.7, so the A drift mean S / T
    is not mean S; the drift of the DIAG problem on the same state differs by
    far more than the bound."""
    Tm = 0.7
    oracle, flat, t, X = ar.pde_setup(k)
    t = t * Tm
    sp = ar.spec(pkg, "smooth_call", sig_b=0.05)
    layers = [k + 2, 16, 16, 16, 16, 1]
    s = pkg.NativeSolver("Naisnet", layers, "Tanh", sp, Tm, dev)
    L = ar.equicorr_L(k, 0.4) if corr else None
    if corr:
        s.set_corr(L)
    prob = ar.AsianProblem(k, "smooth_call", 1.0, T=Tm, sig_b=0.05)
    want = ar.pde_terms(oracle, prob, t, X, L)
    got = native_terms(s, dev, flat, t, X)
    smax = float(np.abs(want["scale"]).max())
    for key in jr.TERMS:
        top = smax if key == "residual" else float(np.abs(want[key]).max())
        bound = 1e-4 if key in ("u", "u_t", "drift", "phi") else 2e-4
        err = float(np.abs(got[key] - want[key]).max())
        print(f"{key}: max|err| = {err:.3e} = {err / top:.3e} max|ref| (bound {bound:.0e})")
        assert top > 0 and np.all(np.isfinite(got[key]))
        np.testing.assert_allclose(got[key], want[key], rtol=0, atol=bound * top)
    diag = pkg.NativeSolver("Naisnet", layers, "Tanh", pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, sig_b=0.05, phi_r=0.05,
                                                                       g="smooth_call", strike=1.0, g_alpha=10.0,
                                                                       g_cols=1), Tm, dev)
    other = native_terms(diag, dev, flat, t, X)
    gap = float(np.abs(other["drift"] - got["drift"]).max())
    print(f"drift: max|DIAG - ASIAN| = {gap:.3e} = {gap / float(np.abs(want['drift']).max()):.3e} max|ref|")
    assert gap > 10 * 1e-4 * float(np.abs(want["drift"]).max())


# ------------------------------------------------------------------ 5. Monte-Carlo
def mc_device(pkg, dev, spec, t, X, n_steps, mc, seed, L=None, delta=False, offset=0):
    v, e, d = pkg.mc_value(spec, torch.from_numpy(np.asarray(t, np.float32)).to(dev),
                           torch.from_numpy(np.asarray(X, np.float32)).to(dev), T, n_steps, mc=mc, seed=seed, L=L,
                           delta=delta, offset=offset)
    torch.cuda.synchronize()
    return v.cpu().numpy()[:, 0], e.cpu().numpy()[:, 0], None if d is None else d.cpu().numpy()


def check_against(ref, v, e, d, kinked):
    """tests/test_gpu_mc.py's _check_against."""
    print("value", v, ref["value"], "stderr", e, ref["stderr"], "ambiguous", ref["ambiguous"])
    np.testing.assert_allclose(v, ref["value"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(e, ref["stderr"], rtol=RTOL, atol=ATOL)
    if d is None:
        return
    print("delta", d, ref["delta"])
    slack = ref["delta_slack"] if kinked else 0.0
    tol = ATOL + RTOL * np.abs(ref["delta"]) + slack
    assert np.all(np.abs(d - ref["delta"]) <= tol), (np.abs(d - ref["delta"]).max(), tol.min())


MC_RUNS = [(p, False) for p in ar.MC_PAYOFFS] + [("call_mean", True), ("smooth_put", True)]


@pytest.mark.parametrize("payoff,corr", MC_RUNS, ids=[p + ("-factor" if c else "") for p, c in MC_RUNS])
@pytest.mark.parametrize("shape", ar.MC_SHAPES, ids=["k8", "k3"])
def test_mc_same_draws(pkg, dev, shape, payoff, corr):
    """Value, standard error and pathwise delta [dA, dS_1..dS_k] == the
    restatement on the same draws (the point at t = T returns g(A_p), 0 and
    (g', 0, ..): its A sits at the strike, g' = +-1/2), with and without a
    factor; the kernel without the tangent computes the same value."""
    k, n_steps, mc = shape
    ref = ar.mc_case(pkg, payoff, shape, corr)
    # a sample within 2e-5 of the kink may sit on its other side on the device: it moves the value by at most
    # 2e-5 / mc (the delta has its own slack); A_T of 8 assets over half a year has a standard deviation of 0.014,
    # so a handful of the 4096 samples are that close
    assert ref["ambiguous"].max() * 2e-5 / mc <= ATOL / 10
    L = ar.equicorr_L(k) if corr else None
    sp = ar.spec(pkg, payoff)
    X = ar.mc_points(k)
    v, e, d = mc_device(pkg, dev, sp, ar.MC_T_POINTS, X, n_steps, mc, ar.MC_SEED, L=L, delta=True)
    check_against(ref, v, e, d, kinked=not payoff.startswith("smooth"))
    assert e[3] == 0 and np.all(d[3, 1:] == 0)                       # the point at t = T: (g', 0, .., 0)
    if not payoff.startswith("smooth"):
        assert abs(d[3, 0]) == 0.5                                   # A_p sits at the strike
    v2, e2, none = mc_device(pkg, dev, sp, ar.MC_T_POINTS, X, n_steps, mc, ar.MC_SEED, L=L)
    assert none is None
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(e2, e)


def test_mc_long_state(pkg, dev):
    """k > 256: a thread runs several assets in turn (and a second time for the
    delta); k = 300 is the smallest shape class that takes this path."""
    k, n_steps, mc = 300, 5, 96
    sp = ar.spec(pkg, "smooth_call")
    rs = np.random.RandomState(12)
    X = np.concatenate([[[0.0], [0.5], [1.0]], rs.uniform(0.8, 1.3, (3, k))], 1).astype(np.float32)
    t = np.array([0.0, 0.5, 1.0], np.float32)
    ref = ar.mc_value(sp, t, X, T, n_steps, mc, seed=4, offset=3, delta=True)
    v, e, d = mc_device(pkg, dev, sp, t, X, n_steps, mc, 4, delta=True, offset=3)
    check_against(ref, v, e, d, kinked=False)


def test_mc_point_does_not_depend_on_the_call(pkg, dev):
    """Bitwise repeatable; a point's result depends neither on P nor on its index."""
    k = 3
    sp, X, t = ar.spec(pkg), ar.mc_points(k), ar.MC_T_POINTS
    args = (6, 4096, ar.MC_SEED)
    a = mc_device(pkg, dev, sp, t, X, *args, delta=True)
    b = mc_device(pkg, dev, sp, t, X, *args, delta=True)
    one = mc_device(pkg, dev, sp, t[2:3], X[2:3], *args, delta=True)
    order = [0, 1, 3, 2, 4, 5, 6, 7, 8, 10, 9]
    X11, t11 = np.concatenate([X, X, X[2:3]])[order], np.concatenate([t, t, t[2:3]])[order]      # rows 3 and 9 <- X[2]
    big = mc_device(pkg, dev, sp, t11, X11, *args, delta=True)
    for u, w, o, g in zip(a, b, one, big):
        np.testing.assert_array_equal(u, w)
        np.testing.assert_array_equal(o[0], u[2])
        np.testing.assert_array_equal(g[3], u[2])
        np.testing.assert_array_equal(g[9], u[2])
    assert one[0][0] != a[0][0]


@pytest.mark.parametrize("corr", [False, True], ids=["plain", "factor"])
def test_mc_call_minus_put_is_the_discounted_forward(pkg, dev, corr):
    """On common draws call - put = e^{-phi_r tau} (mean A_T - K) to fp32
    rounding of the two values: mean A_T from the restatement on those draws."""
    shape = ar.MC_SHAPES[0]
    k, n_steps, mc = shape
    L = ar.equicorr_L(k) if corr else None
    X, t = ar.mc_points(k), ar.MC_T_POINTS
    call, _, _ = mc_device(pkg, dev, ar.spec(pkg, "call_mean"), t, X, n_steps, mc, ar.MC_SEED, L=L)
    put, _, _ = mc_device(pkg, dev, ar.spec(pkg, "put_mean"), t, X, n_steps, mc, ar.MC_SEED, L=L)
    ref = ar.mc_case(pkg, "call_mean", shape, corr)
    disc = np.exp(-float(np.float32(ar.R_RATE)) * (1.0 - t.astype(np.float64)))
    want = disc * (ref["mean_AT"] - 1.0)
    tol = 2.0 ** -23 * (np.abs(call) + np.abs(put)) + RTOL * np.abs(want) + ATOL
    print("call - put", call - put, "forward", want)
    assert np.all(np.abs((call.astype(np.float64) - put.astype(np.float64)) - want) <= tol)


def test_mc_delta_is_the_central_difference_on_common_draws(pkg, dev):
    """Smooth payoff: the pathwise delta of every column, A included, against the
    central difference of two bumped points evaluated in one call (h = 1/256,
    exact in fp32; a point at the money), within the truncation bound of
    tests/asian_reference.py (held on the CPU by tests/test_asian_cpu.py) plus
    the fp32 rounding of the two values, 2^-23 |value| / (2 h) each, and of the
    delta; the bound is below 1e-3 of the delta in every column (asserted)."""
    k, n_steps, mc, h = 3, 6, 4096, 1.0 / 256
    sp = ar.spec(pkg, "smooth_call")
    x = np.array([0.5, 1.0, 1.125, 0.875], np.float32)
    ref = ar.mc_value(sp, [0.5], x[None], T, n_steps, mc, seed=ar.MC_SEED, delta=True)
    pts = np.stack([x] + [x + s * h * np.eye(k + 1, dtype=np.float32)[d] for d in range(k + 1) for s in (1, -1)])
    v, _, d = mc_device(pkg, dev, sp, np.full(len(pts), 0.5, np.float32), pts, n_steps, mc, ar.MC_SEED, delta=True)
    tol = ar.central_difference_bound(ref["dA_max"][0], h) + 2.0 ** -23 * (abs(float(v[0])) / h + np.abs(d[0]))
    for c in range(k + 1):
        cd = (float(v[1 + 2 * c]) - float(v[2 + 2 * c])) / (2 * h)
        print(f"column {c}: pathwise {d[0, c]:.6f}, central difference {cd:.6f} (bound {tol[c]:.2e})")
        assert abs(cd - d[0, c]) <= tol[c] and tol[c] < 1e-3 * abs(d[0, c])


@pytest.mark.parametrize("k", ar.ARBITER["ks"])
def test_mc_arbiter(pkg, dev, k):
    """Strike 0, mu = 0.05, sigma = 0.4, N = 50, mc = 2^18, t in {0, 0.5}: the
    device value lies within 4 stderr of the exact expectation of the Euler
    scheme (tests/test_asian_cpu.py holds the restatement to the same bound on
    the same seed)."""
    c = ar.ARBITER
    sp = ar.spec(pkg, "call_mean", strike=0.0, mu_a=c["mu_a"], sig_a=c["sig_a"])
    X = np.stack([ar.arbiter_point(k)] * len(c["ts"]))
    v, e, _ = mc_device(pkg, dev, sp, np.array(c["ts"], np.float32), X, c["n_steps"], c["mc"], c["seed"])
    for p, t in enumerate(c["ts"]):
        want = ar.euler_expectation(X[p], t, T, c["n_steps"], float(np.float32(c["mu_a"])), float(np.float32(ar.R_RATE)))
        print(f"k={k} t={t}: device {v[p]:.6f} +- {e[p]:.2e}, exact {want:.6f}, |diff| {abs(v[p] - want):.2e} = "
              f"{abs(v[p] - want) / e[p]:.2f} stderr")
        assert e[p] > 0 and abs(v[p] - want) <= 4 * e[p]


# ------------------------------------------------------------------ 6. the problem classes
def test_device_steps_equal_train_steps_on_exported_increments(pkg, dev):
    """Three device_step iterations of AsianBasketCallOption with correlated
    assets (each prefetching the next): finite losses, one optimizer update per
    call.  A twin object runs the same three iterations through train_step on
    the exported (t, W) of the same seeds: parity mode differences W, the fp32
    cumulative sum, so its increments carry a rounding of 2^-24 |W| -- 1e-7 of
    an increment -- and the losses agree within tests/depth_cases.py's loss
    bound, 1e-4 relative, over all three steps."""
    M, k = 24, 5
    np.random.seed(3)
    torch.manual_seed(3)
    mk = lambda: pkg.AsianBasketCallOption(np.ones((1, k)), T, M, N, k, None, [k + 1] + 4 * [16] + [1], "NAIS-Net", "Sine",
                                           "restricted_random_correlation", device=dev)
    m = mk()
    assert m.native_coefficients and m.spec.average and m.solver.nb == k and m.state_dim == k + 1
    assert m.layers[0] == k + 2 and tuple(m.Xi.shape) == (1, k + 1) and float(m.Xi[0, 0]) == 0.0
    assert m._L is not None and m._L.shape == (k, k)
    m2 = mk()
    m2._L, m2.correlation_matrix = m._L, m.correlation_matrix
    m2.solver.set_corr(m._L)
    m2.params.copy_(m.params)
    opt, opt2 = m.new_optimizer_state("Adam", 1e-3), m2.new_optimizer_state("Adam", 1e-3)
    losses, losses2, moved = [], [], []
    for it, seed in enumerate((3, 4, 5)):
        before = m.params.clone()
        losses.append(float(m.device_step(opt, 1e-3, seed=seed, next_seed=seed + 1 if it < 2 else None)))
        moved.append(float((m.params - before).abs().max()))
        t, W = m2.solver.brownian(M, N, seed=seed)
        l2, _ = m2.train_step(t.unsqueeze(-1), W, opt2, learning_rate=1e-3)
        losses2.append(float(l2))
    torch.cuda.synchronize()
    print("device_step", losses, "train_step", losses2, "max |update|", moved)
    assert all(np.isfinite(losses)) and all(v > 0 for v in moved)
    assert m.optimizer_steps_taken(opt) == 3 and opt["calls"] == 3
    np.testing.assert_allclose(losses, losses2, rtol=dc.BOUNDS["loss"])


def test_python_surface(pkg, dev):
    M, k, R = 24, 3, 5
    np.random.seed(4)
    torch.manual_seed(4)
    for cls, g in ((pkg.AsianCallOption, "call_mean"), (pkg.AsianPutOption, "put_mean"),
                   (pkg.AsianBasketPutOption, "put_mean")):
        m = cls(np.ones((1, k)), T, M, N, k, None, [k + 1] + 4 * [16] + [1], "NAIS-Net", "Sine", device=dev)
        assert m.native_coefficients and m.spec.g == g and m.spec.g_cols == 1 and m.strike == 1.0
    sm = pkg.AsianCallOption(np.ones((1, k)), T, M, N, k, None, [k + 1] + 4 * [16] + [1], "NAIS-Net", "Sine",
                             payoff_type="continuous", device=dev)
    assert sm.spec.g == "smooth_call"
    m = pkg.AsianBasketCallOption(np.ones((1, k)), T, M, N, k, None, [k + 1] + 4 * [16] + [1], "NAIS-Net", "Sine", device=dev)
    t, W = m.fetch_minibatch()
    assert t.shape == (M, N + 1, 1) and W.shape == (M, N + 1, k)
    td, Wd = m.fetch_minibatch_device(seed=7)
    assert Wd.shape == (M, N + 1, k)
    loss, X, Y, y0 = m.loss_function(t, W, m.Xi)
    assert X.shape == (M, N + 1, k + 1) and Y.shape == (M, N + 1, 1) and np.isfinite(float(loss.detach()))
    Xn = X.cpu().numpy()
    Wn, tn = W.cpu().numpy(), t.cpu().numpy()[:, :, 0]
    Xr, _ = ar.rollout(ar.xi_state(k), Wn[:, 1:] - Wn[:, :-1], T, tgrid=tn, **ar.COEF)
    np.testing.assert_array_equal(Xn, Xr)
    graph = m.train_device(2, 1e-3, seed=1)
    assert np.all(np.isfinite(graph))
    m.N = N                                                            # (the "corr" schedule shortens N)
    out = m.train(1, 1e-3)
    assert len(out) == 4 and np.isfinite(out[1])
    m.N = N
    t, W = m.fetch_minibatch()
    Xp, Yp = m.predict(np.ones((1, k)), t, W)
    assert Xp.shape == (M, m.N + 1, k + 1) and bool((Xp[:, 0, 0] == 0).all())
    pts = np.concatenate([np.linspace(0.0, 0.6, R)[:, None], np.random.RandomState(1).uniform(0.8, 1.2, (R, k))], 1)
    tp = np.linspace(0.0, 0.6, R)
    u, du = m.net_u(tp, pts)
    assert u.shape == (R, 1) and du.shape == (R, k + 1)
    assert m.theta(tp, pts).shape == (R, 1)
    terms = m.pde_residual(tp, pts)
    assert set(terms) == set(jr.TERMS) and all(x.shape == (R, 1) and bool(torch.isfinite(x).all()) for x in terms.values())
    S = torch.tensor(pts, dtype=torch.float32, device=dev, requires_grad=True)
    with torch.enable_grad():
        _, Du = m.net_u(torch.tensor(tp), S)
        gamma = torch.autograd.grad(Du[:, 1:], S, grad_outputs=torch.ones_like(Du[:, 1:]))[0]
    assert gamma.shape == (R, k + 1)
    val, err, dl = m.mc_value(tp, pts, mc=2048, delta=True)
    assert val.shape == (R, 1) and err.shape == (R, 1) and dl.shape == (R, k + 1)
    val0, _, _ = m.mc_value(np.zeros(2), np.ones((2, k)), mc=2048)            # [S_1..S_k]: A = 0 is prepended
    assert val0.shape == (2, 1) and float(val0[0]) == float(val0[1]) > 0

    class Other(pkg.AsianCallOption):
        def mu_tf(self, t, X, Y=None, Z=None):
            return 0.1 * X

    with pytest.raises(NotImplementedError, match="running-average"):
        Other(np.ones((1, k)), T, M, N, k, None, [k + 1] + 4 * [16] + [1], "NAIS-Net", "Sine", device=dev)
