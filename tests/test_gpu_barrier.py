"""The knock-out problem on the device (problem kind 11, ProblemSpec(barrier=B)):
rollout_barrier_stop_kernel behind every rollout form (in-step, prefetched, the
caller's grid and W, shards, a factor, Dp > 128), the loss and gradient on the
stopped paths, the PDE residual, the Monte-Carlo comparator, the closed forms
and the problem classes.  Needs an MI355X.

Every expectation is computed on the CPU from oracle/philox.py,
oracle/fbsnn_ref.py and tests/barrier_reference.py (held to references of its
own by tests/test_barrier_cpu.py, which also asserts what each case shows:
knocked fractions between 20 % and 80 %, paths with tau = 0, tau = N and none,
margins to the barrier).

Bounds: paths bit-equal to the numpy stopped chain on the device's own
increments; loss / Y / Z / gradient tests/depth_cases.py's BOUNDS against the
fp64 oracle that stops where the float32 chain stops; PDE terms bit-equal to
kind DIAG's; Monte-Carlo tests/test_gpu_asian.py::test_mc_same_draws's RTOL,
ATOL = 2e-5, 2e-6; closed forms 2^-23 relative, the fp32 rounding of an fp64
value (tests/test_gpu_american.py holds the tree kernel to the same)."""
import os

import numpy as np
import pytest
import torch

import barrier_reference as br
import depth_cases as dc
import jet_reference as jr
import mc_reference as mr
from conftest import load_pkg
from oracle import philox as ph

pytestmark = pytest.mark.gpu
T = br.T
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


def make_solver(pkg, dev, k, spec, mode="Naisnet", layers=None, env=None, act="Sine"):
    """A context of the kind (env holds while it is created, every other path switch unset)."""
    layers = layers or [k + 1, 16, 16, 16, 16, 1]
    old = {n: os.environ.pop(n, None) for n in ENV_KEYS}
    os.environ.update(env or {})
    try:
        s = pkg.NativeSolver(mode, layers, act, spec, T, dev)
    finally:
        for n, v in old.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v
    assert s.D == k and s.nb == k
    return s


def case_spec(pkg, c, phi_c=0.0):
    return br.spec(pkg, c["payoff"], strike=c["strike"], barrier=c["barrier"], cols=c["cols"], phi_c=phi_c, **c["coef"])


def to_dev(a, dev):
    return torch.as_tensor(np.asarray(a, np.float32)).to(dev).contiguous()


def paths(s, dev, params, M, N, xi, seed, path0=0, grad=False, t=None, W=None):
    """(X [M, N+1, D], loss, grad or None) of a loss_grad into NaN-filled outputs."""
    X = torch.full((M * (N + 1) * s.D,), float("nan"), device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    g = torch.full_like(params, float("nan")) if grad else None
    s.loss_grad(params, M, N, xi, seed=seed, path0=path0, loss=loss, X=X, grad=g, t=t, W=W)
    torch.cuda.synchronize()
    return X.cpu().numpy().reshape(M, N + 1, s.D), float(loss), (g.cpu().numpy() if grad else None)


def dirty_path_buffer(s, dev, M, N):
    """NaN into the rows the next rollout of this shape writes
    (tests/test_gpu_asian.py's recipe): the state columns of xin and sdw."""
    D, R = s.D, M * (N + 1)
    par = torch.zeros(s.nparams, device=dev)
    nan = lambda n: torch.full((n,), float("nan"), device=dev)
    s.loss_grad(par, M, N, nan(D), seed=77, loss=torch.empty(1, device=dev))
    s.net_u(par, nan(R), nan(R * D), torch.empty(R, device=dev), torch.empty(R * D, device=dev))
    s.net_u_vjp(par, torch.zeros(R, device=dev), torch.ones(R * D, device=dev), torch.zeros(R, device=dev), nan(R * D),
                torch.empty(s.nparams, device=dev))
    torch.cuda.synchronize()


def zero_net_loss(c, X):
    """The loss of the zero network on stopped rows: sum g(X_N)^2 + sum |dg(X_N)|^2
    over the payoff columns -- finite only if no NaN is left in any sdw column
    (0 . NaN), and 0 on every knocked path."""
    prob = br.BarrierProblem(c["k"], c["payoff"], c["strike"], c["cols"])
    XN = torch.as_tensor(X[:, -1].astype(np.float64)).requires_grad_(True)
    g = prob.g(XN)
    dg = torch.autograd.grad(g.sum(), XN)[0]
    return float((g.detach() ** 2).sum() + (dg[:, :prob.cols] ** 2).sum())


# ------------------------------------------------------------------ 1. rows
@pytest.mark.parametrize("name", list(br.ROW_CASES))
def test_rows_are_the_stopped_chain_on_the_device_increments(pkg, dev, name):
    """X bit-equal to the numpy stopped chain on the device's own increments,
    out of NaN-filled path buffers and NaN-filled outputs; the stopping rows are
    the CPU reference's (its margins hold); the zero network's loss is the
    terminal terms of the live paths alone, so every sdw column was rewritten."""
    c = br.row_case(name)
    k, M, N = c["k"], c["M"], c["N"]
    s = make_solver(pkg, dev, k, case_spec(pkg, c))
    zero, xi = torch.zeros(s.nparams, device=dev), to_dev(c["xi"], dev)
    dirty_path_buffer(s, dev, M, N)
    _, dW = s.brownian(M, N, seed=c["seed"], increments=True)
    X, loss, _ = paths(s, dev, zero, M, N, xi, c["seed"])
    r = br.rollout(c["xi"], dW.cpu().numpy(), T, c["payoff"], c["barrier"], c["cols"], **c["coef"])
    np.testing.assert_array_equal(X, r["X"])
    ref = br.rollout(c["xi"], ph.increments(c["seed"], 0, 0, M, N, k, T), T, c["payoff"], c["barrier"], c["cols"], **c["coef"])
    np.testing.assert_array_equal(r["tau"], ref["tau"])
    cov = br.coverage(r["tau"], N)
    print(name, cov)
    assert cov["first"] and cov["last"] and cov["never"] and np.any(r["X"] != r["X0"])
    np.testing.assert_allclose(loss, zero_net_loss(c, r["X"]), rtol=1e-5)


# ------------------------------------------------------------------ 2. routes
@pytest.mark.parametrize("name", ["k3_put_mean", "k130_call_mean"])
def test_callers_grid_and_W(pkg, dev, name):
    """The caller's non-uniform grid per path with W of the device's own draws
    (fetch_minibatch followed by loss_function goes through the same stop pass),
    and the caller's grid alone."""
    c = br.row_case(name)
    k, M, N = c["k"], c["M"], c["N"]
    s = make_solver(pkg, dev, k, case_spec(pkg, c))
    zero, xi = torch.zeros(s.nparams, device=dev), to_dev(c["xi"], dev)
    _, W = s.brownian(M, N, seed=c["seed"])
    _, dW = s.brownian(M, N, seed=c["seed"], increments=True)
    torch.cuda.synchronize()
    rs = np.random.RandomState(k)
    tg = np.concatenate([np.zeros((M, 1)), np.cumsum(rs.uniform(0.5, 1.5, (M, N)), 1)], 1)
    tg = (tg / tg[:, -1:] * T).astype(np.float32)
    td = torch.from_numpy(tg).to(dev).contiguous()
    Xp, _, _ = paths(s, dev, zero, M, N, xi, c["seed"], t=td, W=W.contiguous())
    Wn = W.cpu().numpy()
    r = br.rollout(c["xi"], Wn[:, 1:] - Wn[:, :-1], T, c["payoff"], c["barrier"], c["cols"], tgrid=tg, **c["coef"])
    np.testing.assert_array_equal(Xp, r["X"])
    assert np.any(r["X"] != r["X0"]) and np.any(r["tau"] > N)
    Xg, _, _ = paths(s, dev, zero, M, N, xi, c["seed"], t=td)
    r2 = br.rollout(c["xi"], dW.cpu().numpy(), T, c["payoff"], c["barrier"], c["cols"], tgrid=tg, **c["coef"])
    np.testing.assert_array_equal(Xg, r2["X"])


@pytest.mark.parametrize("name", ["k3_put_mean", "k17_put_sum", "k130_put_mean"])
def test_shards_and_prefetch(pkg, dev, name):
    """An odd path0; three shards equal one device; a prefetched step, consumed
    at once or held back over a step of another batch, equals an in-step one bit
    for bit (paths, loss and gradient)."""
    c = br.row_case(name)
    k, M, N = c["k"], c["M"], c["N"]
    s = make_solver(pkg, dev, k, case_spec(pkg, c))
    zero = torch.zeros(s.nparams, device=dev)
    xi1 = to_dev(c["xi"][M // 2 - 2:M // 2 - 1], dev)                   # one shared state close to the barrier
    Xall, _, _ = paths(s, dev, zero, M, N, xi1, c["seed"])
    cuts = ((0, 7), (7, 25), (32, M - 32))
    parts = [paths(s, dev, zero, m, N, xi1, c["seed"], path0=p0)[0] for p0, m in cuts]
    np.testing.assert_array_equal(np.concatenate(parts), Xall)
    xi = to_dev(c["xi"], dev)
    torch.manual_seed(k)
    params = (0.3 * torch.randn(s.nparams)).to(dev)
    ref = paths(s, dev, params, M, N, xi, 5, grad=True)
    other = paths(s, dev, params, M, N, xi, 6, grad=True)
    assert np.isfinite(ref[1]) and np.abs(ref[2]).max() > 0
    unstopped = ph.rollout(c["xi"], s.brownian(M, N, seed=5, increments=True)[1].cpu().numpy(), T, **c["coef"])
    assert np.any(ref[0] != unstopped)
    s.prefetch(M, N, xi, seed=5)
    got = paths(s, dev, params, M, N, xi, 5, grad=True)
    s.prefetch(M, N, xi, seed=5)
    mid = paths(s, dev, params, M, N, xi, 6, grad=True)
    late = paths(s, dev, params, M, N, xi, 5, grad=True)
    for a, b in ((got, ref), (late, ref), (mid, other)):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1]
        np.testing.assert_array_equal(a[2], b[2])


@pytest.mark.parametrize("name", ["k3_put_mean", "k17_put_sum", "k130_put_mean"])
def test_with_a_factor(pkg, dev, name):
    """L = I gives the uncorrelated bits; with a factor X is the stopped chain on
    the device's own (correlated) increments, in-step and prefetched."""
    c = br.row_case(name)
    k, M, N = c["k"], c["M"], c["N"]
    s = make_solver(pkg, dev, k, case_spec(pkg, c))
    zero, xi = torch.zeros(s.nparams, device=dev), to_dev(c["xi"], dev)
    plain = paths(s, dev, zero, M, N, xi, c["seed"])[0]
    s.set_corr(np.eye(k, dtype=np.float32))
    np.testing.assert_array_equal(paths(s, dev, zero, M, N, xi, c["seed"])[0], plain)
    s.set_corr(br.ar.equicorr_L(k, 0.3))
    dirty_path_buffer(s, dev, M, N)
    _, dW = s.brownian(M, N, seed=c["seed"], increments=True)
    X, loss, _ = paths(s, dev, zero, M, N, xi, c["seed"])
    r = br.rollout(c["xi"], dW.cpu().numpy(), T, c["payoff"], c["barrier"], c["cols"], **c["coef"])
    np.testing.assert_array_equal(X, r["X"])
    assert np.any(X != plain) and np.any(r["X"] != r["X0"]) and np.any(r["tau"] > N)
    np.testing.assert_allclose(loss, zero_net_loss(c, r["X"]), rtol=1e-5)
    s.prefetch(M, N, xi, seed=c["seed"])
    np.testing.assert_array_equal(paths(s, dev, zero, M, N, xi, c["seed"])[0], X)


# ------------------------------------------------------------------ 3. loss and gradient
@pytest.mark.parametrize("name", list(br.LOSS_CASES))
def test_loss_and_gradient_match_the_fp64_oracle(pkg, dev, name):
    """Loss, Y, Z and every gradient tensor within tests/depth_cases.py's BOUNDS
    of the fp64 oracle on the device's own increments, stopped where the float32
    chain stops; X bit-equal to that chain; the context runs the kernels the
    case names, the stop pass among them.  tests/test_barrier_cpu.py shows that
    the unstopped loss is more than ten loss bounds away."""
    c = br.loss_case(name)
    k, M, N = c["k"], c["M"], c["N"]
    model, flat = br.loss_model(name)
    s = make_solver(pkg, dev, k, case_spec(pkg, c, c["phi_c"]), c["mode"], c["layers"], c["env"], c["act"])
    _, dW = s.brownian(M, N, seed=c["seed"], increments=True)
    torch.cuda.synchronize()
    dW = dW.cpu().numpy()
    r = br.rollout(c["xi"], dW, T, c["payoff"], c["barrier"], c["cols"], **c["coef"])
    ref = br.loss_and_grads(model, br.loss_problem(name), ph.time_grid(N, T), dW, c["xi"], r["tau"])
    cov = br.coverage(r["tau"], N)
    assert cov["first"] and cov["last"] and cov["never"] and 0.2 <= cov["knocked"] <= 0.8, cov
    params = torch.from_numpy(flat.astype(np.float32)).to(dev)
    nan = lambda n: torch.full((n,), float("nan"), device=dev)
    out = dict(loss=nan(1), X=nan(M * (N + 1) * k), Y=nan(M * (N + 1)), Z=nan(M * (N + 1) * k))
    grad = torch.full_like(params, float("nan"))
    s.profile(True)
    s.loss_grad(params, M, N, to_dev(c["xi"], dev), seed=c["seed"], grad=grad, **out)
    torch.cuda.synchronize()
    names = set(s.profile_read())
    s.profile(False)
    got = {n: v.cpu().numpy() for n, v in out.items()}
    got["X"], got["Z"] = got["X"].reshape(M, N + 1, k), got["Z"].reshape(M, N + 1, k)
    got["Y"], got["grad"] = got["Y"].reshape(M, N + 1, 1), grad.cpu().numpy()
    print(f"{name}: ran {sorted(names)}")
    assert "barrier_stop" in names
    assert ("fused_fwd_inputgrad" in names) == name.startswith("fused"), sorted(names)
    for key in ("loss", "X", "Y", "Z", "grad"):
        assert np.all(np.isfinite(got[key])), key
    e = dc.errors(got, ref, dc.tensors(model))
    print(f"{name}: error / bound: " + ", ".join(f"{n} {v:.3g}" if not isinstance(v, str) else f"({v})" for n, v in e.items()))
    np.testing.assert_array_equal(got["X"], r["X"])
    assert np.all(got["grad"][~ref["used"]] == 0)
    for key in ("loss", "Y", "Z", "grad", "tensor"):
        assert e[key] <= 1.0, f"{name}: {key} is {e[key]:.3g} of its bound ({e['tensor_name']})"


# ------------------------------------------------------------------ 4. PDE residual
def test_pde_residual_is_diags_on_the_live_side(pkg, dev):
    """12 live-side points: every term equals kind DIAG's bit for bit (the
    generators of the stopped and the unstopped process agree there), with and
    without a factor."""
    k, R = 3, 12
    sp = br.spec(pkg, "call_mean", strike=1.0, barrier=0.9, phi_c=1.0, sig_b=0.05)
    plain = pkg.ProblemSpec(**{**{f: getattr(sp, f) for f in sp.__dataclass_fields__}, "barrier": 0.0})
    layers = [k + 1, 16, 16, 16, 16, 1]
    a, b = pkg.NativeSolver("Naisnet", layers, "Tanh", sp, T, dev), pkg.NativeSolver("Naisnet", layers, "Tanh", plain, T, dev)
    torch.manual_seed(5)
    params = (0.3 * torch.randn(a.nparams)).to(dev)
    rs = np.random.RandomState(3)
    t, X = to_dev(rs.uniform(0.0, 0.9, R), dev), to_dev(rs.uniform(0.92, 1.4, (R, k)), dev)
    for L in (None, br.ar.equicorr_L(k, 0.4)):
        got = []
        for s in (a, b):
            s.set_corr(L)
            out = {key: torch.full((R,), float("nan"), device=dev) for key in jr.TERMS}
            s.pde_residual(params, t, X, **out)
            torch.cuda.synchronize()
            got.append({key: v.cpu().numpy() for key, v in out.items()})
        for key in jr.TERMS:
            assert np.all(np.isfinite(got[0][key])) and np.abs(got[0][key]).max() > 0, key
            np.testing.assert_array_equal(got[0][key], got[1][key])


# ------------------------------------------------------------------ 5. Monte-Carlo
def mc_device(pkg, dev, spec, t, X, n_steps, mc, seed, L=None, offset=0):
    v, e, d = pkg.mc_value(spec, to_dev(t, dev), to_dev(X, dev), T, n_steps, mc=mc, seed=seed, L=L, offset=offset)
    torch.cuda.synchronize()
    assert d is None
    return v.cpu().numpy()[:, 0], e.cpu().numpy()[:, 0]


@pytest.mark.parametrize("name", list(br.MC_CASES))
def test_mc_same_draws(pkg, dev, name):
    """Value and standard error == the restatement on the same draws, k in {1, 3,
    8, 100}, with and without a factor.  Every alive flag is the restatement's:
    tests/test_barrier_cpu.py shows each sample's deciding statistics more than
    ten normal errors from the barrier, and one flipped flag of an in-the-money
    sample would move the value by g / mc, far above the tolerance.  The point at
    t = T beyond the barrier returns 0 and 0, the live one g(x) and 0.  Bitwise
    repeatable."""
    c, ref = br.mc_setup(pkg, name), br.mc_case(pkg, name)
    v, e = mc_device(pkg, dev, c["spec"], c["t"], c["X"], c["n_steps"], c["mc"], c["seed"], L=c["L"])
    print(name, "value", v, ref["value"], "stderr", e, ref["stderr"], "alive", ref["alive"].mean(1))
    np.testing.assert_allclose(v, ref["value"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(e, ref["stderr"], rtol=RTOL, atol=ATOL)
    assert v[4] == 0 and e[4] == 0 and e[3] == 0 and v[3] > 0
    v2, e2 = mc_device(pkg, dev, c["spec"], c["t"], c["X"], c["n_steps"], c["mc"], c["seed"], L=c["L"])
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(e2, e)


@pytest.mark.parametrize("name", ["k3_put_mean", "k8_call_mean-factor"])
def test_mc_point_does_not_depend_on_the_call(pkg, dev, name):
    """A point's result depends neither on P nor on its index."""
    c = br.mc_setup(pkg, name)
    X, t = c["X"], c["t"]
    args = (c["n_steps"], c["mc"], c["seed"])
    a = mc_device(pkg, dev, c["spec"], t, X, *args, L=c["L"])
    one = mc_device(pkg, dev, c["spec"], t[2:3], X[2:3], *args, L=c["L"])
    order = [0, 1, 3, 2, 4, 5, 6, 7, 8, 10, 9]
    X11, t11 = np.concatenate([X, X, X[2:3]])[order], np.concatenate([t, t, t[2:3]])[order]      # rows 3 and 9 <- X[2]
    big = mc_device(pkg, dev, c["spec"], t11, X11, *args, L=c["L"])
    for u, o, g in zip(a, one, big):
        np.testing.assert_array_equal(o[0], u[2])
        np.testing.assert_array_equal(g[3], u[2])
        np.testing.assert_array_equal(g[9], u[2])
    assert one[0][0] != a[0][0]


@pytest.mark.parametrize("name", ["k1_call", "k8_call_mean", "k8_call_mean-factor", "k100_put_sum"])
def test_mc_bounds_and_limits(pkg, dev, name):
    """With the barrier out of reach (B = 1e-30 for a call, 1e30 for a put) the
    value is within one fp32 ulp of kind DIAG's on the same draws (the payoff sum
    runs in another order, in fp64); the knocked-out value is <= the vanilla one
    at every point."""
    c = br.mc_setup(pkg, name)
    sp = c["spec"]
    fields = {f: getattr(sp, f) for f in sp.__dataclass_fields__}
    args = (c["t"], c["X"], c["n_steps"], c["mc"], c["seed"])
    far = pkg.ProblemSpec(**{**fields, "barrier": 1e30 if sp.g in br.PUTS else 1e-30})
    plain = pkg.ProblemSpec(**{**fields, "barrier": 0.0})
    v, e = mc_device(pkg, dev, sp, *args, L=c["L"])
    vf, ef = mc_device(pkg, dev, far, *args, L=c["L"])
    vd, ed = mc_device(pkg, dev, plain, *args, L=c["L"])
    ulp = np.spacing(np.abs(vd).astype(np.float32))
    print(name, "barrier", v, "far", vf, "diag", vd)
    assert np.all(np.abs(vf[:4] - vd[:4]) <= ulp[:4]) and np.all(np.abs(ef[:4] - ed[:4]) <= np.spacing(np.abs(ed[:4]).astype(np.float32)))
    assert np.all(v <= vd)
    if sp.g not in br.PUTS:                     # (a knocked put path of three steps need not come back into the money)
        assert np.any(v[:3] < vd[:3])


def test_mc_refusals(pkg, dev):
    sp = br.spec(pkg, "call_mean", strike=1.0, barrier=0.9)
    t = torch.zeros(1, device=dev)
    with pytest.raises(ValueError, match="bump and reprice"):
        pkg.mc_value(sp, t, torch.ones(1, 3, device=dev), T, 4, mc=16, delta=True)
    with pytest.raises(ValueError, match="128"):
        pkg.mc_value(sp, t, torch.ones(1, 129, device=dev), T, 4, mc=16)
    v, e, _ = pkg.mc_value(sp, t, torch.ones(1, 128, device=dev), T, 4, mc=64)
    torch.cuda.synchronize()
    assert np.isfinite(float(v)) and float(e) >= 0


@pytest.mark.parametrize("side", ["call", "put"])
def test_mc_arbiter(pkg, dev, side):
    """k = 1, N = 2: the scheme's expectation is exact in one dimension
    (barrier_reference.arbiter, held on the CPU to the issue's figures 0.131094
    and 0.034490 and to a Monte Carlo of its own); the device value at mc = 2^18
    lies within 4 of its own standard errors."""
    a = br.ARBITER
    B, want = a[side]["B"], a[side]["value"]
    sp = br.spec(pkg, f"{side}_sum", strike=a["K"], barrier=B, phi_c=1.0, mu_a=a["b"] - a["r"], sig_a=a["sig"])
    assert abs(float(mr.mu_eff(sp)) - a["b"]) < 1e-7
    v, e = mc_device(pkg, dev, sp, [0.0], [[a["x"]]], a["n_steps"], a["mc"], a["seed"])
    exact = br.arbiter(side == "put", B)
    print(f"{side}: device {v[0]:.6f} +- {e[0]:.2e}, exact {exact:.6f} (issue {want}), |diff| {abs(v[0] - exact) / e[0]:.2f} stderr")
    assert abs(exact - want) < 5e-7
    assert e[0] > 0 and abs(v[0] - want) <= 4 * e[0]


# ------------------------------------------------------------------ 6. closed forms
@pytest.mark.parametrize("kind,B", [("barrier_call", 0.9), ("barrier_put", 1.1)])
@pytest.mark.parametrize("n_mon", [0.0, 50.0])
def test_closed_forms_on_the_device(pkg, dev, kind, B, n_mon):
    """64 points x 2 coordinates, tau from 0 to 2, S on both sides of the barrier
    and at least 1 % from it on the live side: price and delta against the fp64
    numpy restatement at 2^-23 relative (the bound tests/test_gpu_american.py
    holds the tree kernel to: the fp32 rounding of an fp64 value), 0 beyond the
    barrier, the payoff at tau = 0; two calls are bitwise equal."""
    put = kind == "barrier_put"
    r, sig, K, b = 0.05, 0.2, 1.0, 0.10
    rs = np.random.RandomState(8)
    S = rs.uniform(0.95, 1.6, (64, 2)) if not put else rs.uniform(0.5, 1.05, (64, 2))
    S[::8, 1] = 0.8 if not put else 1.2                                   # beyond the barrier
    S = S.astype(np.float32)
    t = np.concatenate([[2.0, 2.0], rs.uniform(0.0, 1.95, 62)]).astype(np.float32)
    tau = 2.0 - t.astype(np.float64)
    p = (r, sig, K, b, B, n_mon)
    price, delta = pkg.exact(kind, to_dev(t, dev), to_dev(S, dev), 2.0, p)
    p2, d2 = pkg.exact(kind, to_dev(t, dev), to_dev(S, dev), 2.0, p)
    torch.cuda.synchronize()
    assert price.shape == (64, 2) == delta.shape and torch.equal(price, p2) and torch.equal(delta, d2)
    wp, wd = br.closed_form(S.astype(np.float64), tau[:, None], r, sig, K, b, B, n_mon, put)
    for what, got, want in (("price", price, wp), ("delta", delta, wd)):
        got = got.cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        print(f"{kind} n_mon {n_mon} {what}: max err / (2^-23 |ref|) = {(err / (F32_EPS * np.abs(want) + 1e-45)).max():.3f}")
        assert np.all(err <= F32_EPS * np.abs(want) + 1.5e-45), what
    assert np.all(price.cpu().numpy()[::8, 1] == 0) and np.all(delta.cpu().numpy()[::8, 1] == 0)
    assert np.abs(wp).max() > 0.1


# ------------------------------------------------------------------ 7. the problem classes
def test_python_surface(pkg, dev, tmp_path):
    M, N, k = 24, 6, 5
    np.random.seed(3)
    torch.manual_seed(3)
    lay = [k + 1] + 4 * [16] + [1]
    m = pkg.BarrierBasketCallOption(np.ones((1, k)), T, M, N, k, None, lay, "NAIS-Net", "Sine", "restricted_random_correlation",
                                    device=dev, barrier=0.97)
    assert m.native_coefficients and m.spec.barrier == 0.97 and m.spec.g == "call_mean" and m.strike == 1.0
    assert m._L is not None and m.solver.nb == k and m.spec.to_c().kind == 11
    opt = m.new_optimizer_state("Adam", 1e-3)
    losses = [float(m.device_step(opt, 1e-3, seed=s, next_seed=s + 1 if s < 5 else None)) for s in (3, 4, 5)]
    torch.cuda.synchronize()
    print("device_step", losses)
    assert all(np.isfinite(losses)) and m.optimizer_steps_taken(opt) == 3
    m.N = N
    t, W = m.fetch_minibatch()
    loss, X, Y, y0 = m.loss_function(t, W, m.Xi)
    Wn, tn = W.cpu().numpy(), t.cpu().numpy()[:, :, 0]
    r = br.rollout(np.ones((1, k)), Wn[:, 1:] - Wn[:, :-1], T, "call_mean", 0.97, tgrid=tn, **br.COEF)
    np.testing.assert_array_equal(X.cpu().numpy(), r["X"])
    assert np.isfinite(float(loss.detach())) and np.any(r["tau"] <= N) and np.any(r["tau"] > N)
    pts, tp = np.random.RandomState(1).uniform(0.99, 1.1, (4, k)), np.linspace(0.0, 0.6, 4)
    val, err, none = m.mc_value(tp, pts, mc=2048)
    twin = m.european()
    assert type(twin) is type(m) and twin.barrier == 0.0 and twin.spec.to_c().kind == 0
    np.testing.assert_array_equal(twin._L, m._L)
    up, _, _ = twin.mc_value(tp, pts, mc=2048)
    torch.cuda.synchronize()
    assert none is None and val.shape == (4, 1) and bool((val <= up).all()) and bool((val < up).any()) and bool((val > 0).all())
    with pytest.raises(ValueError, match="bump and reprice"):
        m.mc_value(tp, pts, mc=64, delta=True)
    assert not hasattr(m, "mc_greeks")
    with pytest.raises(ValueError, match="one asset"):
        m.closed_form(tp, pts)
    f = str(tmp_path / "barrier.pt")
    m.save_model(f)
    m2 = pkg.BarrierBasketCallOption(np.ones((1, k)), T, M, N, k, None, lay, "NAIS-Net", "Sine", device=dev, barrier=0.97)
    m2.load_model(f)
    for a, b in zip(m.model.state_dict().values(), m2.model.state_dict().values()):
        assert torch.equal(a.cpu(), b.cpu())

    # one asset: the closed form, discrete and continuous monitoring, against the restatement
    for cls, B, put in ((pkg.BarrierCallOption, 0.9, False), (pkg.BarrierPutOption, 1.1, True),
                        (pkg.BarrierBasketCallOption, 0.9, False), (pkg.BarrierBasketPutOption, 1.1, True)):
        o = cls(np.ones((1, 1)), T, M, 50, 1, None, [2] + 4 * [16] + [1], "NAIS-Net", "Sine", device=dev, barrier=B)
        assert o.native_coefficients and o.strike == 1.0 and o.spec.q3 is False
        S, tt = np.array([0.95, 1.0, 1.05, 1.0], np.float32), np.array([0.0, 0.0, 0.5, 1.0], np.float32)
        sp = o.spec
        bb = sp.mu_a + sp.phi_r * sp.phi_c
        tau = 1.0 - tt.astype(np.float64)
        for mon, nm in (("discrete", 50), ("continuous", 0)):
            pr, dl = o.closed_form(tt, S, monitoring=mon)
            # n_mon = N tau / T: the same spacing T / N at every point
            want = [br.closed_form(float(S[i]), tau[i], sp.phi_r, sp.sig_a, 1.0, bb, B, nm * tau[i], put) for i in range(4)]
            np.testing.assert_allclose(pr.cpu().numpy()[:, 0], [float(w[0]) for w in want], rtol=2 * F32_EPS, atol=1e-45)
            np.testing.assert_allclose(dl.cpu().numpy()[:, 0], [float(w[1]) for w in want], rtol=2 * F32_EPS, atol=1e-45)
        with pytest.raises(ValueError, match="monitoring"):
            o.closed_form(tt, S, monitoring="daily")

    class Other(pkg.BarrierCallOption):
        def sigma_tf(self, t, X, Y):
            return 0.5 * torch.diag_embed(X)

    with pytest.raises(NotImplementedError, match="knock-out"):
        Other(np.ones((1, k)), T, M, N, k, None, lay, "NAIS-Net", "Sine", device=dev, barrier=0.9 * k)
    with pytest.raises(ValueError, match="strike"):
        pkg.BarrierCallOption(np.ones((1, k)), T, M, N, k, None, lay, "NAIS-Net", "Sine", device=dev, barrier=1.1 * k)
