"""The geometric-average Asian problem on the device (problem kind 8,
ProblemSpec(average="geometric")): rollout_asian_chain_kernel and the geometric
instance of rollout_asian_avg_kernel in every role (increments, paths, the
caller's grid and W, shards, prefetch, a factor), the loss and gradient on every
network form, the PDE residual, the Monte-Carlo comparator against its
restatement, against the closed form and against the arithmetic problem (the
geometric price is its lower bound path by path), the closed forms
DBSDE_EXACT_GEO_ASIAN / _PUT and the problem classes.  Needs an MI355X.

Every expectation is computed on the CPU from oracle/philox.py,
oracle/fbsnn_ref.py and tests/geo_asian_reference.py (held to references of its
own by tests/test_geo_asian_cpu.py).

Shapes: tests/test_gpu_asian.py's -- k in {1, 3, 17, 70, 130}, M in {24, 7},
N = 6.  Bounds: increments and the S columns as there (bit-equal to the numpy
chain); the G column within (4 N + 2) 2^-24 max(1, |a|) G of the chain on the
device's own S (the device's fp64 log / exp may differ from the host's by one
fp32 ulp at a near-tie: each of the N steps then moves a = log G by at most 4
roundings of a term <= 1, the exp adds 2; the number of entries that differ at
all is printed, 0 expected); loss / Y / Z / gradient tests/depth_cases.py's
BOUNDS with X at rtol 1e-5 / atol 1e-6; PDE terms tests/test_gpu_jet.py's 1e-4 /
2e-4 of max|ref|; Monte-Carlo tests/test_gpu_mc.py's RTOL, ATOL = 2e-5, 2e-6 and
kink slack; closed forms tests/test_gpu_put.py's 2^-23 relative."""
import os

import numpy as np
import pytest
import torch

import asian_reference as ar
import depth_cases as dc
import geo_asian_reference as gr
import jet_reference as jr
import path_cases as pc
from conftest import load_pkg
from oracle import philox as ph

pytestmark = pytest.mark.gpu
T, N = gr.T, gr.N
KS = list(gr.KS)
MS = gr.MS
SEED = 4
RTOL, ATOL = 2e-5, 2e-6
F32_EPS = 2.0 ** -23
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
        s = pkg.NativeSolver(mode, layers, act, spec or gr.spec(pkg), T, dev)
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
    xi = np.repeat(gr.xi_state(k), rows, 0)
    if rows > 1:                                                     # per-path states: G_0 and the prices differ
        xi = xi * np.linspace(0.8, 1.2, rows)[:, None]
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
    (tests/test_gpu_asian.py's recipe)."""
    D, R = s.D, M * (N + 1)
    par = torch.zeros(s.nparams, device=dev)
    nan = lambda n: torch.full((n,), float("nan"), device=dev)
    s.loss_grad(par, M, N, nan(D), seed=77, loss=torch.empty(1, device=dev))
    s.net_u(par, nan(R), nan(R * D), torch.empty(R, device=dev), torch.empty(R * D, device=dev))
    s.net_u_vjp(par, torch.zeros(R, device=dev), torch.ones(R * D, device=dev), torch.zeros(R, device=dev), nan(R * D),
                torch.empty(s.nparams, device=dev))
    torch.cuda.synchronize()


def check_paths(X, xi, dW, what, tgrid=None):
    """S columns bit-equal to the numpy chain; the G column within the documented
    bound of the chain on those S (the count of differing entries is printed)."""
    Xr, sdw, a = gr.rollout(xi, dW, T, tgrid=tgrid, with_log=True, **gr.COEF)
    np.testing.assert_array_equal(X[:, :, 1:], Xr[:, :, 1:])
    np.testing.assert_array_equal(X[:, 0, 0], Xr[:, 0, 0])                       # G_0 as given
    assert np.all(sdw[:, :, 0] == 0)
    G, Gr = X[:, :, 0], Xr[:, :, 0]
    assert np.all(np.isfinite(G))
    bound = gr.g_column_bound(a, Gr, dW.shape[1])
    err = np.abs(G.astype(np.float64) - Gr.astype(np.float64))
    print(f"{what}: {int((G != Gr).sum())} of {G.size} G entries differ from the chain; max err / bound = "
          f"{(err / bound).max():.3f}")
    assert np.all(err <= bound)
    return Xr


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
    """Out of NaN-filled path buffers.  A NaN left in any sigma dW column -- the
    G column, which must be rewritten with 0, included -- makes the loss NaN,
    and the loss of the zero network is sum g(G_N)^2 + sum g'(G_N)^2 exactly."""
    s = solver(pkg, dev, k)
    zero = torch.zeros(s.nparams, device=dev)
    for M in MS:
        dirty_path_buffer(s, dev, M)
        _, dW = s.brownian(M, N, seed=SEED, increments=True)
        X, loss, _ = paths(s, dev, zero, M, xi_dev(dev, k), SEED)
        Xr = check_paths(X, gr.xi_state(k), dW.cpu().numpy(), f"k={k} M={M}")
        assert np.all(X[:, 0, 0] == 1.0) and np.ptp(Xr[:, -1, 0]) > 1e-3          # the average moved, path by path
        a = X[:, -1, 0].astype(np.float64) - 1.0
        assert np.abs(a).min() > 1e-6
        want = np.sum(np.maximum(a, 0.0) ** 2) + np.sum((a > 0) * 1.0)
        np.testing.assert_allclose(loss, want, rtol=1e-5)


@pytest.mark.parametrize("k", [1, 17, 130])
def test_callers_grid_and_W(pkg, dev, k):
    """The caller's t / W [M, N+1, k]: a non-uniform grid per path, per-path
    G_0 != 1, W of the device's own draws; and the caller's grid alone."""
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
    check_paths(Xp, xi.cpu().numpy(), Wn[:, 1:] - Wn[:, :-1], f"k={k} caller's t and W", tgrid=tg)
    Xg, _, _ = paths(s, dev, zero, M, xi, SEED, t=td)
    check_paths(Xg, xi.cpu().numpy(), dW.cpu().numpy(), f"k={k} caller's t", tgrid=tg)
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
    """The increments equal L dz within tests/path_cases.py's corr_bound; the
    paths are the chain on the device's own increments (device grid and the
    caller's); L = I gives the uncorrelated bits; shards and a prefetched step
    as without a factor."""
    s = make_solver(pkg, dev, k)
    zero, xi = torch.zeros(s.nparams, device=dev), xi_dev(dev, k)
    plain = {M: paths(s, dev, zero, M, xi, SEED)[0] for M in MS}
    L = gr.equicorr_L(k, 0.3) if k < 100 else np.linalg.cholesky(
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
        check_paths(X, gr.xi_state(k), dW, f"k={k} M={M} factor")
        assert np.any(X != plain[M])
    M = 7
    tg = np.broadcast_to((ph.time_grid(N, T).astype(np.float64) ** 1.5).astype(np.float32), (M, N + 1)).copy()
    _, dW = s.brownian(M, N, seed=SEED, increments=True)
    Xg, _, _ = paths(s, dev, zero, M, xi, SEED, t=torch.from_numpy(tg).to(dev))
    check_paths(Xg, gr.xi_state(k), dW.cpu().numpy(), f"k={k} factor, caller's t", tgrid=tg)
    X24, _, _ = paths(s, dev, zero, 24, xi, SEED)
    parts = [paths(s, dev, zero, m, xi, SEED, path0=p0)[0] for p0, m in ((0, 7), (7, 17))]
    np.testing.assert_array_equal(np.concatenate(parts), X24)
    s.prefetch(24, N, xi, seed=SEED)
    np.testing.assert_array_equal(paths(s, dev, zero, 24, xi, SEED)[0], X24)


# ------------------------------------------------------------------ 3. loss and gradient
_LOSS_REFS = {}


def loss_reference(case, dW):
    """The fp64 oracle on the device's own increments, once per network and batch."""
    k, M = gr.LOSS_CASES[case][:2]
    key = (k, M, tuple(gr.loss_layers(case)))
    if key not in _LOSS_REFS:
        model, _ = gr.loss_model(case)
        prob = gr.GeoAsianProblem(k, "call_mean", gr.LOSS_STRIKE)
        ref = gr.loss_and_grads(model, prob, ph.time_grid(N, T), dW, gr.xi_state(k))
        _LOSS_REFS[key] = (dW, dict(ref64=ref, tensors=dc.tensors(model)))
    np.testing.assert_array_equal(dW, _LOSS_REFS[key][0])
    return _LOSS_REFS[key][1]


@pytest.mark.parametrize("case", list(gr.LOSS_CASES))
def test_loss_and_gradient_match_the_fp64_oracle(pkg, dev, case):
    """Loss, Y, Z and every gradient tensor within tests/depth_cases.py's BOUNDS
    of the fp64 oracle, X within rtol 1e-5 / atol 1e-6 of it (and the chain's),
    unused gradient elements 0; the context runs the kernels the case names."""
    k, M, mode, act, _, env = gr.LOSS_CASES[case]
    layers = gr.loss_layers(case)
    _, flat = gr.loss_model(case)
    s = make_solver(pkg, dev, k, mode, layers, env, act, gr.spec(pkg, "call_mean", gr.LOSS_STRIKE))
    seed = gr.LOSS_SEED + k
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
    assert {"asian_chain", "geo_asian_avg"} <= names and "asian_avg" not in names
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
    check_paths(r["X"], gr.xi_state(k), dW.cpu().numpy(), case)
    assert np.all(r["grad"][~ref["used"]] == 0)
    for key in ("loss", "Y", "Z", "grad", "tensor"):
        assert e[key] <= 1.0, f"{case}: {key} is {e[key]:.3g} of its bound ({e['tensor_name']})"
    assert np.abs(ref["Z"][:, :, 0]).max() > 1e-3                                  # u_G is there to be wrong


# ------------------------------------------------------------------ 4. PDE residual
def native_terms(s, dev, flat, t, X):
    R = X.shape[0]
    out = {key: torch.empty(R, device=dev) for key in jr.TERMS}
    s.pde_residual(torch.from_numpy(flat).to(dev), torch.from_numpy(t.ravel().astype(np.float32)).to(dev),
                   torch.from_numpy(X.astype(np.float32)).to(dev).contiguous(), **out)
    torch.cuda.synchronize()
    return {key: v.cpu().numpy().reshape(R, 1) for key, v in out.items()}


@pytest.mark.parametrize("k,corr", [(1, False), (1, True), (3, False), (3, True), (70, False), (70, True)],
                         ids=["k1", "k1-factor", "k3", "k3-factor", "k70", "k70-factor"])
def test_pde_residual_terms(pkg, dev, k, corr):
    """R = 12 random points against double autograd: u, u_t, drift and phi
    within 1e-4 of max|ref|, the diffusion within 2e-4, the residual within 2e-4
    of max(scale) (tests/test_gpu_jet.py).  T = 0.7; the drift of the arithmetic
    problem on the same state differs by far more than the bound."""
    Tm = 0.7
    oracle, flat, t, X = gr.pde_setup(k)
    t = t * Tm
    sp = gr.spec(pkg, "smooth_call")
    layers = [k + 2, 16, 16, 16, 16, 1]
    s = pkg.NativeSolver("Naisnet", layers, "Tanh", sp, Tm, dev)
    L = gr.equicorr_L(k, 0.4) if corr else None
    if corr:
        s.set_corr(L)
    prob = gr.GeoAsianProblem(k, "smooth_call", 1.0, T=Tm)
    want = gr.pde_terms(oracle, prob, t, X, L)
    got = native_terms(s, dev, flat, t, X)
    smax = float(np.abs(want["scale"]).max())
    for key in jr.TERMS:
        top = smax if key == "residual" else float(np.abs(want[key]).max())
        bound = 1e-4 if key in ("u", "u_t", "drift", "phi") else 2e-4
        err = float(np.abs(got[key] - want[key]).max())
        print(f"{key}: max|err| = {err:.3e} = {err / top:.3e} max|ref| (bound {bound:.0e})")
        assert top > 0 and np.all(np.isfinite(got[key]))
        np.testing.assert_allclose(got[key], want[key], rtol=0, atol=bound * top)
    arith = pkg.NativeSolver("Naisnet", layers, "Tanh", ar.spec(pkg, "smooth_call"), Tm, dev)
    other = native_terms(arith, dev, flat, t, X)
    gap = float(np.abs(other["drift"] - got["drift"]).max())
    print(f"drift: max|ASIAN - GEO_ASIAN| = {gap:.3e} = {gap / float(np.abs(want['drift']).max()):.3e} max|ref|")
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


MC_RUNS = [(p, c) for c in (False, True) for p in gr.MC_PAYOFFS]


@pytest.mark.parametrize("payoff,corr", MC_RUNS, ids=[p + ("-factor" if c else "") for p, c in MC_RUNS])
@pytest.mark.parametrize("shape", gr.MC_SHAPES, ids=["k8", "k3"])
def test_mc_same_draws(pkg, dev, shape, payoff, corr):
    """Value, standard error and pathwise delta [dG, dS_1..dS_k] == the
    restatement on the same draws (the point at t = T returns g(G_p), 0 and
    (g', 0, ..): its G sits at the strike, g' = +-1/2), with and without a
    factor; the kernel without the tangent computes the same value."""
    k, n_steps, mc = shape
    ref = gr.mc_case(pkg, payoff, shape, corr)
    # a sample within 2e-5 of the kink may sit on its other side on the device: it moves the value by at most
    # 2e-5 / mc (the delta has its own slack)
    assert ref["ambiguous"].max() * 2e-5 / mc <= ATOL / 10
    L = gr.equicorr_L(k) if corr else None
    sp = gr.spec(pkg, payoff)
    X = gr.mc_points(k)
    v, e, d = mc_device(pkg, dev, sp, gr.MC_T_POINTS, X, n_steps, mc, gr.MC_SEED, L=L, delta=True)
    check_against(ref, v, e, d, kinked=not payoff.startswith("smooth"))
    assert e[3] == 0 and np.all(d[3, 1:] == 0)                       # the point at t = T: (g', 0, .., 0)
    if not payoff.startswith("smooth"):
        assert abs(d[3, 0]) == 0.5                                   # G_p sits at the strike
    v2, e2, none = mc_device(pkg, dev, sp, gr.MC_T_POINTS, X, n_steps, mc, gr.MC_SEED, L=L)
    assert none is None
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(e2, e)


def test_mc_long_state(pkg, dev):
    """k > 256: a thread runs several assets in turn (and a second time for the
    delta); k = 300 is the smallest shape class that takes this path."""
    k, n_steps, mc = 300, 5, 96
    sp = gr.spec(pkg, "smooth_call")
    rs = np.random.RandomState(12)
    X = np.concatenate([[[1.0], [0.98], [1.01]], rs.uniform(0.8, 1.3, (3, k))], 1).astype(np.float32)
    t = np.array([0.0, 0.5, 1.0], np.float32)
    ref = gr.mc_value(sp, t, X, T, n_steps, mc, seed=4, offset=3, delta=True)
    v, e, d = mc_device(pkg, dev, sp, t, X, n_steps, mc, 4, delta=True, offset=3)
    check_against(ref, v, e, d, kinked=False)


def test_mc_point_does_not_depend_on_the_call(pkg, dev):
    """Bitwise repeatable; a point's result depends neither on P nor on its index."""
    k = 3
    sp, X, t = gr.spec(pkg), gr.mc_points(k), gr.MC_T_POINTS
    args = (6, 4096, gr.MC_SEED)
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


def exact_device(pkg, dev, kind, t, X, Tm, params):
    p, d = pkg.exact(kind, torch.from_numpy(np.asarray(t, np.float32)).to(dev),
                     torch.from_numpy(np.asarray(X, np.float32)).to(dev), Tm, params)
    torch.cuda.synchronize()
    return p.cpu().numpy(), d.cpu().numpy()


@pytest.mark.parametrize("k,t,G", gr.ARBITER["points"], ids=[f"k{k}-t{t}" for k, t, _ in gr.ARBITER["points"]])
def test_mc_arbiter(pkg, dev, k, t, G):
    """Strike 1, sigma = 0.4, mu = r = 0.05, n_steps = 400, mc = 2^16: the device
    value lies within 4 stderr of exact("geo_asian") (tests/test_geo_asian_cpu.py
    holds the restatement to 3 stderr on the same seed)."""
    c = gr.ARBITER
    sp = gr.spec(pkg, "call_mean", strike=c["strike"], mu_a=c["mu_a"], sig_a=c["sig_a"])
    x = gr.arbiter_point(k, G)[None]
    L = gr.arbiter_L(k)
    v, e, _ = mc_device(pkg, dev, sp, [t], x, c["steps"][-1], c["mc"], c["seed"], L=L)
    cbar, vbar = gr.factor_moments(L, k)
    r32 = lambda v: float(np.float32(v))                                  # the comparator's coefficients are fp32
    want, _ = exact_device(pkg, dev, "geo_asian", [t], x, T,
                           (r32(c["mu_a"]), r32(gr.R_RATE), r32(c["sig_a"]), c["strike"], cbar, vbar))
    want = float(want[0, 0])
    assert abs(want - gr.arbiter_exact(k, t, G)) <= F32_EPS * want
    print(f"k={k} t={t}: device {v[0]:.6f} +- {e[0]:.2e}, closed form {want:.6f}, |diff| {abs(v[0] - want):.2e} = "
          f"{abs(v[0] - want) / e[0]:.2f} stderr")
    assert e[0] > 0 and abs(v[0] - want) <= 4 * e[0]


@pytest.mark.parametrize("k,corr", [(1, False), (8, False), (8, True)], ids=["k1", "k8", "k8-factor"])
def test_geometric_value_bounds_the_arithmetic_value(pkg, dev, k, corr):
    """t = 0, G = 1, A = 0, the same seed and factor: the left-point weights
    dt_n / T sum to 1, so G_T <= A_T sample by sample (the geometric mean of the
    S_{i,n} under those weights against their arithmetic mean): the geometric
    call is at most the arithmetic call, the geometric put at least the
    arithmetic put, up to 2^-22 |value|."""
    n_steps, mc = 6, 4096
    S = np.random.RandomState(11).uniform(0.8, 1.3, (3, k)).astype(np.float32)
    t = np.zeros(3, np.float32)
    Xg, Xa = np.concatenate([np.ones((3, 1), np.float32), S], 1), np.concatenate([np.zeros((3, 1), np.float32), S], 1)
    L = gr.equicorr_L(k) if corr else None
    for payoff, sign in (("call_mean", 1.0), ("put_mean", -1.0)):
        vg, _, _ = mc_device(pkg, dev, gr.spec(pkg, payoff), t, Xg, n_steps, mc, gr.MC_SEED, L=L)
        va, _, _ = mc_device(pkg, dev, ar.spec(pkg, payoff), t, Xa, n_steps, mc, gr.MC_SEED, L=L)
        print(f"k={k} {payoff}: geometric {vg}, arithmetic {va}")
        assert np.all(sign * (vg.astype(np.float64) - va.astype(np.float64)) <= 2.0 ** -22 * np.abs(vg))
        assert np.all(vg > 0) and np.any(vg != va)                  # (an arithmetic put far out of the money is exactly 0)


# ------------------------------------------------------------------ 6. the closed forms
def fp32_close(got, want, what):
    """tests/test_gpu_put.py's rule: got is the fp32 rounding of an fp64 value
    equal to want up to fp64 rounding of the same formula."""
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max err / (2^-23 |ref|) = {(err / (F32_EPS * np.abs(want) + 1e-45)).max():.3f}")
    assert np.all(err <= F32_EPS * np.abs(want) + 1.5e-45), what


@pytest.mark.parametrize("k,corr", [(1, False), (3, False), (3, True)], ids=["k1", "k3", "k3-factor"])
def test_closed_forms_on_the_device(pkg, dev, k, corr):
    """64 points, tau from 0 to 2 (tau = 0 at, in and out of the money first),
    then a deep out-of-the-money point; prices and every delta column against
    the fp64 numpy formula at 2^-23 relative; device call - put against the
    forward under tests/test_gpu_put.py's parity bound."""
    Tm = 2.0
    rs = np.random.RandomState(40 + k)
    G = rs.uniform(0.7, 1.4, 64).astype(np.float32)
    S = rs.uniform(0.5, 2.0, (64, k)).astype(np.float32)
    tau = rs.uniform(0.02, 2.0, 64).astype(np.float32)
    G[:3], tau[:3] = [1.0, 1.25, 0.75], 0.0
    tau[3] = 2.0
    X = np.concatenate([G[:, None], S], 1)
    deep = np.full((1, k + 1), 0.7, np.float32)       # a call far out of the money (1 / deep: a put), d2 = -4.6 .. -8
    X, tau = np.concatenate([X, deep, 1.0 / deep]), np.append(tau, np.float32([1.0, 1.0]))
    t = (np.float32(Tm) - tau).astype(np.float32)
    L = gr.equicorr_L(k, 0.3) if corr else None
    cbar, vbar = gr.factor_moments(L, k)
    params = (0.03, 0.05, 0.4, 1.0, cbar, vbar)
    res = {}
    for kind, put in (("geo_asian", False), ("geo_asian_put", True)):
        want_p, want_d = gr.closed_form(X.astype(np.float64), t, Tm, *params, put=put)
        p, d = exact_device(pkg, dev, kind, t, X, Tm, params)
        assert p.shape == (66, 1) and d.shape == (66, k + 1)
        fp32_close(p[:, 0], want_p, kind + " price")
        fp32_close(d, want_d, kind + " delta")
        res[kind] = p[:, 0]
        sgn = -1.0 if put else 1.0
        np.testing.assert_array_equal(p[:3, 0], [0.0, 0.0 if put else 0.25, 0.25 if put else 0.0])
        np.testing.assert_array_equal(d[:3, 0], [sgn * 0.5, 0.0 if put else 1.0, -1.0 if put else 0.0])
        assert np.all(d[:3, 1:] == 0)
        far = 64 if not put else 65
        print(f"{kind} deep out of the money: device {p[far, 0]:.6e}, fp64 {want_p[far]:.6e}")
        assert 2.0 ** -126 < p[far, 0] < 1e-4
    Mm, V, tau64 = gr.closed_form_terms(X.astype(np.float64), t, Tm, *params)
    fwd = np.where(tau64 > 0, np.exp(-params[1] * tau64) * (np.exp(Mm + 0.5 * V) - params[3]), X[:, 0].astype(np.float64) - 1.0)
    c, p = res["geo_asian"].astype(np.float64), res["geo_asian_put"].astype(np.float64)
    gap = np.abs(c - p - fwd)
    bound = 2.0 ** -24 * (np.abs(c) + np.abs(p)) + 2.0 ** -24 * np.abs(fwd)
    print(f"parity: max gap / bound = {(gap / np.maximum(bound, 1e-300)).max():.3f}")
    assert np.all(gap <= bound)


# ------------------------------------------------------------------ 7. the problem classes
def test_device_steps_equal_train_steps_on_exported_increments(pkg, dev):
    """tests/test_gpu_asian.py's check on GeometricAsianBasketCallOption with
    correlated assets: three device_step iterations (each prefetching the next)
    against train_step on the exported (t, W) of the same seeds, losses within
    tests/depth_cases.py's loss bound."""
    M, k = 24, 5
    np.random.seed(3)
    torch.manual_seed(3)
    mk = lambda: pkg.GeometricAsianBasketCallOption(np.ones((1, k)), T, M, N, k, None, [k + 1] + 4 * [16] + [1], "NAIS-Net",
                                                    "Sine", "restricted_random_correlation", device=dev)
    m = mk()
    assert m.native_coefficients and m.spec.average == "geometric" and m.solver.nb == k and m.state_dim == k + 1
    assert m.layers[0] == k + 2 and tuple(m.Xi.shape) == (1, k + 1) and float(m.Xi[0, 0]) == 1.0
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
    lay = [k + 1] + 4 * [16] + [1]
    pts = np.concatenate([np.linspace(1.0, 1.05, R)[:, None], np.random.RandomState(1).uniform(0.8, 1.2, (R, k))], 1)
    tp = np.linspace(0.0, 0.6, R)
    for cls, g, corr in ((pkg.GeometricAsianCallOption, "call_mean", "no_correlation"),
                         (pkg.GeometricAsianPutOption, "put_mean", "no_correlation"),
                         (pkg.GeometricAsianBasketCallOption, "call_mean", "restricted_random_correlation"),
                         (pkg.GeometricAsianBasketPutOption, "put_mean", "no_correlation")):
        m = cls(np.ones((1, k)), T, M, N, k, None, lay, "NAIS-Net", "Sine", corr, device=dev)
        assert m.native_coefficients and m.spec.g == g and m.spec.g_cols == 1 and m.strike == 1.0
        assert m.spec.average == "geometric" and float(m.Xi[0, 0]) == 1.0 and m.state_dim == k + 1
        graph = m.train_device(2, 1e-3, seed=1)
        assert np.all(np.isfinite(graph))
        m.N = N                                                            # (the "corr" schedule shortens N)
        t, W = m.fetch_minibatch()
        assert W.shape == (M, N + 1, k)
        Xp, Yp = m.predict(np.ones((1, k)), t, W)
        assert Xp.shape == (M, N + 1, k + 1) and bool((Xp[:, 0, 0] == 1).all()) and bool((Xp[:, :, 0] > 0).all())
        Wn, tn = W.cpu().numpy(), t.cpu().numpy()[:, :, 0]
        check_paths(Xp.cpu().numpy(), gr.xi_state(k), Wn[:, 1:] - Wn[:, :-1], cls.__name__, tgrid=tn)
        terms = m.pde_residual(tp, pts)
        assert set(terms) == set(jr.TERMS) and all(x.shape == (R, 1) and bool(torch.isfinite(x).all()) for x in terms.values())
        val, err, dl = m.mc_value(tp, pts, mc=2048, delta=True)
        assert val.shape == (R, 1) and err.shape == (R, 1) and dl.shape == (R, k + 1)
        assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(dl).all())
        val0, _, _ = m.mc_value(np.zeros(2), np.ones((2, k)), mc=2048)            # [S_1..S_k]: G = 1 is prepended
        assert val0.shape == (2, 1) and float(val0[0]) == float(val0[1]) > 0
        # closed_form() is exact() with this object's strike, T and factor
        price, delta = m.closed_form(pts[:, 0], pts[:, 1:], tp)
        cbar, vbar = gr.factor_moments(m._L, k)
        kind = "geo_asian_put" if cls.option_type == "put" else "geo_asian"
        p2, d2 = pkg.exact(kind, torch.as_tensor(tp, dtype=torch.float32).to(dev),
                           torch.as_tensor(pts, dtype=torch.float32).to(dev), T, (0.05, 0.05, 0.20, 1.0, cbar, vbar))
        assert price.shape == (R, 1) and delta.shape == (R, k + 1)
        assert torch.equal(price, p2) and torch.equal(delta, d2)
        want, _ = gr.closed_form(pts.astype(np.float32).astype(np.float64), tp.astype(np.float32), T, 0.05, 0.05, 0.20, 1.0,
                                 cbar, vbar, put=cls.option_type == "put")
        fp32_close(price.cpu().numpy()[:, 0], want, cls.__name__ + ".closed_form")
        if corr != "no_correlation":
            assert abs(vbar - 1.0 / k) > 1e-3                                # the factor is felt
    sm = pkg.GeometricAsianCallOption(np.ones((1, k)), T, M, N, k, None, lay, "NAIS-Net", "Sine", payoff_type="continuous",
                                      device=dev)
    assert sm.spec.g == "smooth_call"
    with pytest.raises(ValueError, match="discontinuous"):
        sm.closed_form(pts[:, 0], pts[:, 1:], tp)
    for bad in (np.array([[1.0, -0.5, 1.0]]), np.array([[0.0, 1.0, 1.0, 1.0]])):       # S_2 <= 0; G = 0
        with pytest.raises(ValueError, match="positive|> 0"):
            pkg.GeometricAsianCallOption(bad, T, M, N, k, None, lay, "NAIS-Net", "Sine", device=dev)
    with pytest.raises(ValueError, match="positive|> 0"):
        sm.mc_value(np.zeros(1), np.array([[1.0, 1.0, 0.0]]), mc=64)

    class Other(pkg.GeometricAsianCallOption):
        def mu_tf(self, t, X, Y=None, Z=None):
            return 0.1 * X

    with pytest.raises(NotImplementedError, match="running-average"):
        Other(np.ones((1, k)), T, M, N, k, None, lay, "NAIS-Net", "Sine", device=dev)
