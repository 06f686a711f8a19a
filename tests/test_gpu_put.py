"""The put payoffs on the device: terminal conditions "put_sum", "put_mean",
"smooth_put" at every place of the engine that evaluates the terminal
condition, the tie gradient, Heston kinds 1 and 2, the Monte-Carlo comparator,
the closed forms "bs_put", "basket_avg_put", "basket_mean_put", "heston_put",
and the problem classes.  Needs an MI355X.

Every expectation is computed on the CPU: oracle/fbsnn_ref.py with the put
payoffs as duck-typed problems, and the restatements of tests/put_reference.py
(held to references of their own by tests/test_put_cpu.py, which also checks
the conditions on these tests' inputs).

Bounds: loss / Y / Z / gradient tests/depth_cases.py's BOUNDS (the call
cases' bounds: only signs differ); Heston tests/test_gpu_heston2.py's check;
Monte-Carlo tests/test_gpu_mc.py's RTOL, ATOL = 2e-5, 2e-6 and kink slack;
closed forms the fp32 rounding of an fp64 value, 2^-23 relative.

Measured on an MI355X when these tests were written, the largest fraction of
its bound over the 24 site x payoff cases: loss 0.0014, Y 0.0089, Z 0.0078,
gradient 0.0060, worst tensor 0.0121; the tie Z-term within 3.7e-5 absolute
(3e-3 of its tolerance); closed forms at most 0.63 of 2^-23 relative; the Heston
put 0.149449 +- 3.4e-4 by Monte-Carlo against 0.149650 (bound 1.8e-3)."""
import os

import numpy as np
import pytest
import torch

import depth_cases as dc
import heston2_reference as h2
import put_reference as pr
from conftest import load_pkg
from oracle import fbsnn_ref as fr
from oracle import philox as ph

pytestmark = pytest.mark.gpu

ENV_KEYS = ("DBSDE_FUSED", "DBSDE_TNW", "DBSDE_X3", "DBSDE_TNW_X3", "DBSDE_CS", "DBSDE_CHUNKS", "DBSDE_W256",
            "DBSDE_TNW_ORDER")
RTOL, ATOL = 2e-5, 2e-6
F32_EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def with_env(env, make):
    """make() while env holds and every other path switch of the engine is unset."""
    old = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env or {})
    try:
        return make()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def site_solver(pkg, dev, site, spec):
    c = pr.SITES[site]
    return with_env(c["env"], lambda: pkg.NativeSolver(c["mode"], c["layers"], c["act"], spec, pr.T, dev))


def loss_grad(s, dev, b, D, grad=True):
    """One parity-mode loss_grad on the bundle's t, W, Xi into NaN-filled outputs."""
    M, N = b["M"], b["N"]
    params = torch.from_numpy(b["params"]).to(dev)
    nan = lambda n: torch.full((n,), float("nan"), device=dev)
    out = dict(loss=nan(1), X=nan(M * (N + 1) * D), Y=nan(M * (N + 1)), Z=nan(M * (N + 1) * D))
    g = torch.full_like(params, float("nan")) if grad else None
    s.loss_grad(params, M, N, torch.from_numpy(b["Xi"]).to(dev).contiguous(),
                t=torch.from_numpy(b["t"]).to(dev).reshape(M, N + 1).contiguous(),
                W=torch.from_numpy(b["W"]).to(dev).contiguous(), grad=g, **out)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    r["X"], r["Z"], r["Y"] = r["X"].reshape(M, N + 1, D), r["Z"].reshape(M, N + 1, D), r["Y"].reshape(M, N + 1, 1)
    if grad:
        r["grad"] = g.cpu().numpy()
    return r


def ran(s, dev, b, D):
    """Names of what a profiled repeat launched."""
    s.profile(True)
    s.profile_reset()
    loss_grad(s, dev, b, D)
    names = set(s.profile_read())
    s.profile(False)
    return names


def check_site(s, site, names):
    """The context runs the site's kernels: fused phases or the per-layer
    chain with its EPI_COTAN epilogue / the wide row kernel; the split-bf16 or
    the fp32-input form of the fused phases."""
    c = pr.SITES[site]
    assert ("fused_fwd_inputgrad" in names) == c["fused"], sorted(names)
    if site == "chain110":
        assert "gemm_z_cotangent" in names, sorted(names)
    if site == "wide130":
        assert "z_row_cotangent" in names, sorted(names)
    if c["fused"] and c["layers"][1] != 16:
        assert (s.matrix_form & 1) == (0 if site.endswith("_fp32") else 1), (site, s.matrix_form)


# ------------------------------------------------------------------ 1. loss and gradients at every cotangent site
@pytest.mark.parametrize("site,payoff", pr.RUNS, ids=[f"{s}-{p}" for s, p in pr.RUNS])
def test_loss_and_gradients_match_the_fp64_oracle(pkg, dev, site, payoff):
    """M = 20, N = 3 (80 rows), parity-mode W, strike 1.0625 (x D for the sum):
    rows on both sides of the kink.  tests/depth_cases.py's check: X bit-equal
    to the fp32 oracle, loss / Y / Z / gradient (global and per tensor) within
    BOUNDS of the fp64 oracle, unused gradient elements exactly 0."""
    b = pr.reference(site, payoff)
    D = pr.site_dim(site)
    s = site_solver(pkg, dev, site, pr.spec_for(pkg, pr.site_base(site, payoff), payoff, D))
    r = loss_grad(s, dev, b, D)
    names = ran(s, dev, b, D)
    print(f"{site} {payoff}: matrix_form {s.matrix_form}, ran {sorted(names)}")
    dc.check(r, b, f"{site} {payoff}")
    check_site(s, site, names)
    fwd = loss_grad(s, dev, b, D, grad=False)              # the forward-only loss kernel (cotan_kernel / chain)
    assert abs(float(fwd["loss"][0]) - b["ref64"]["loss"]) <= dc.BOUNDS["loss"] * abs(b["ref64"]["loss"])


# ------------------------------------------------------------------ 2. the tie
@pytest.mark.parametrize("site,payoff", [(s, p) for s in pr.TIE_SITES for p in pr.TIE_PAYOFFS])
def test_tie_rows_take_half_the_gradient(pkg, dev, site, payoff):
    """Three paths with W = 0 and Xi = ones, 1.25 ones, 0.75 ones at K = 1 (K = D
    for the sum): X_N = Xi, the rows sit at, out of and in the money.  The
    whole step against the fp64 oracle (torch.maximum's 1/2 : 1/2 split) with
    BOUNDS -- a split of 0 or 1 moves the worst tensor's gradient by more than
    10 bounds (tests/test_put_cpu.py) -- and the terminal Z-term by itself:
    the device's loss minus every other term, recomputed in fp64 from the
    device's own Y and Z, equals sum |Z_N - dg|^2 with dg = -1/2, 0, -1 (over
    G for the mean) within pr.TIE_ZTERM_RTOL of the loss."""
    b = pr.tie_reference(site, payoff)
    D = pr.site_dim(site)
    s = site_solver(pkg, dev, site, pr.spec_for(pkg, "bsb", payoff, D, level=1.0))
    r = loss_grad(s, dev, b, D)
    names = ran(s, dev, b, D)
    dc.check(r, b, f"tie {site} {payoff}")
    check_site(s, site, names)
    np.testing.assert_array_equal(r["X"][:, -1, :], b["Xi"])
    # every term but the terminal Z-term, from the device's Y and Z ("bsb": phi = 0.05 (Y - X.Z), dW = 0)
    X, Y, Z, t = (np.asarray(v, np.float64) for v in (r["X"], r["Y"][..., 0], r["Z"], b["t"]))
    rest = 0.0
    for n in range(b["N"]):
        phi = 0.05 * (Y[:, n] - np.sum(X[:, n] * Z[:, n], 1))
        rest += np.sum((Y[:, n + 1] - (Y[:, n] + phi * (t[:, n + 1] - t[:, n]))) ** 2)
    a = pr.moneyness(b, payoff, 1.0)
    rest += np.sum((Y[:, -1] - np.maximum(a, 0.0)) ** 2)
    cols = 1.0 if payoff == "put_sum" else float(D)
    dg = np.array([-0.5, 0.0, -1.0]) / cols
    want = np.sum((Z[:, -1, :] - dg[:, None]) ** 2)
    got = float(r["loss"][0]) - rest
    tol = pr.TIE_ZTERM_RTOL * abs(float(r["loss"][0]))
    print(f"tie {site} {payoff}: Z-term {got:.6e}, with the 1/2 split {want:.6e}, |diff| {abs(got - want):.2e}, tol {tol:.2e}")
    assert abs(got - want) <= tol


# ------------------------------------------------------------------ 3. Heston kinds 1 and 2
def heston_check(r, ref):
    """tests/test_gpu_heston2.py's check."""
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


@pytest.mark.parametrize("payoff_type", ["discontinuous", "continuous"])
@pytest.mark.parametrize("kind", ["heston", "heston2"])
def test_heston_put_loss_and_gradient_match_oracle(pkg, dev, kind, payoff_type):
    """k = 3, M = 7, N = 6 on the device's own batch: kind 1 against
    oracle.fbsnn_ref.heston_loss_function on the exported (t, W), kind 2
    against its two-factor restatement on the exported increments, both with
    the put g over the k asset columns and the u clamp."""
    k, M, N = pr.HESTON_K, pr.HESTON_M, h2.N
    layers, model, flat = h2.loss_model(k)
    spec = pr.heston_spec(pkg, kind, payoff_type)
    s = with_env({}, lambda: pkg.NativeSolver("Naisnet", layers, "Sine", spec, h2.T, dev))
    seed = pr.HESTON_SEED + k
    h = pr.PutHeston(k=k, payoff=payoff_type, **h2.HESTON)
    if kind == "heston":
        t, W = s.brownian(M, N, seed=seed)
        torch.cuda.synchronize()
        ref = fr.heston_loss_and_grads(model, h, t.cpu()[..., None], W.cpu(), np.ones((1, k)), M)
    else:
        _, dW = s.brownian(M, N, seed=seed, increments=True)
        torch.cuda.synchronize()
        ref = pr.heston2_loss_and_grads(model, h, ph.time_grid(N, h2.T), dW.cpu().numpy(), h2.xi_state(k))
    a = 1.0 - np.asarray(ref["X"], np.float64)[:, -1, :k].mean(1)
    print(f"{kind} {payoff_type}: K - mean S_N = {a}")
    assert 0 < (a > 0).sum() < M                      # rows on both sides of the kink
    params = torch.from_numpy(flat.astype(np.float32)).to(dev)
    out = dict(loss=torch.empty(1, device=dev), X=torch.empty(M * (N + 1) * 2 * k, device=dev),
               Y=torch.empty(M * (N + 1), device=dev), Z=torch.empty(M * (N + 1) * 2 * k, device=dev))
    grad = torch.empty_like(params)
    xi = torch.as_tensor(h2.xi_state(k), dtype=torch.float32).to(dev).contiguous()
    s.loss_grad(params, M, N, xi, seed=seed, grad=grad, **out)
    torch.cuda.synchronize()
    r = {n: v.cpu().numpy() for n, v in out.items()}
    r["X"], r["Z"] = r["X"].reshape(M, N + 1, 2 * k), r["Z"].reshape(M, N + 1, 2 * k)
    r["Y"], r["grad"] = r["Y"].reshape(M, N + 1, 1), grad.cpu().numpy()
    assert float(np.abs(ref["Y"][:, -1]).max()) > 0   # (not clamped away)
    heston_check(r, ref)


# ------------------------------------------------------------------ 4. Monte-Carlo comparator
def mc_device(pkg, dev, spec, t, X, n_steps, mc, seed, L=None, delta=False):
    v, e, d = pkg.mc_value(spec, torch.from_numpy(np.asarray(t, np.float32)).to(dev),
                           torch.from_numpy(np.asarray(X, np.float32)).to(dev), pr.T, n_steps, mc=mc, seed=seed, L=L,
                           delta=delta)
    torch.cuda.synchronize()
    return v.cpu().numpy()[:, 0], e.cpu().numpy()[:, 0], None if d is None else d.cpu().numpy()


@pytest.mark.parametrize("shape", pr.MC_SHAPES, ids=[f"D{d}_N{n}_mc{m}" for d, n, m in pr.MC_SHAPES])
@pytest.mark.parametrize("name", pr.MC_DIAG)
def test_mc_same_draws_diag(pkg, dev, name, shape):
    """Value, standard error and pathwise delta == the restatement on the same
    draws (tests/test_gpu_mc.py's test_same_draws_diag for the puts), with and
    without L; point 3 has tau = 0: the payoff and its -1 / -1/2 / 0 gradient.
    A sample within 2e-5 of the kink may sit on its other side on the device:
    the delta lies within the restatement's +- (their |dg J| sum) / mc."""
    D, n_steps, mc = shape
    spec, L = pr.mc_diag_spec(pkg, name, D)
    ref = pr.mc_diag_case(pkg, name, shape)
    assert ref["ambiguous"].max() <= 4
    X = pr.mc_points(D)
    v, e, d = mc_device(pkg, dev, spec, pr.MC_T_POINTS, X, n_steps, mc, pr.MC_SEED, L=L, delta=True)
    print("value", v, ref["value"], "stderr", e, ref["stderr"], "ambiguous", ref["ambiguous"])
    np.testing.assert_allclose(v, ref["value"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(e, ref["stderr"], rtol=RTOL, atol=ATOL)
    slack = ref["delta_slack"] if name != "smooth_put" else 0.0
    tol = ATOL + RTOL * np.abs(ref["delta"]) + slack
    print("delta", d, ref["delta"])
    assert np.all(np.abs(d - ref["delta"]) <= tol), (np.abs(d - ref["delta"]).max(), tol.min())
    g, dg, _ = pr.payoff(spec, X[3:4])
    assert v[3] == np.float32(g[0]) and e[3] == 0 and np.all(d[3] == dg[0].astype(np.float32))
    v2, e2, none = mc_device(pkg, dev, spec, pr.MC_T_POINTS, X, n_steps, mc, pr.MC_SEED, L=L)
    assert none is None
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(e2, e)


def test_mc_maturity_point_at_the_kink(pkg, dev):
    """tau <= 0 at, out of and in the money: the payoff and -1/2, 0, -1 (over G
    for the mean), 0 past g_cols."""
    X = np.array([[1.5, 0.5, 7.0], [1.5, 1.0, 7.0], [0.5, 1.0, 7.0]], np.float32)
    t = np.array([1.0, 1.0, 2.0], np.float32)
    for g, K, n in (("put_sum", 2.0, 1.0), ("put_mean", 1.0, 2.0)):
        spec = pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, g=g, strike=K, g_cols=2)
        v, e, d = mc_device(pkg, dev, spec, t, X, 4, 8, 0, delta=True)
        np.testing.assert_array_equal(v, np.array([0.0, 0.0, 0.5 if g == "put_sum" else 0.25], np.float32))
        np.testing.assert_array_equal(e, 0.0)
        want = np.array([[-0.5, -0.5, 0.0], [0.0, 0.0, 0.0], [-1.0, -1.0, 0.0]]) / n
        np.testing.assert_array_equal(d, want.astype(np.float32))


@pytest.mark.parametrize("kind,g", pr.MC_HESTON, ids=[f"{k}-{g}" for k, g in pr.MC_HESTON])
def test_mc_same_draws_heston(pkg, dev, kind, g):
    """Heston kinds 1, 2 and kind 1 with correlated assets (k = 3): value and
    standard error on the same draws; the delta refusal stays."""
    spec, L = pr.mc_heston_spec(pkg, kind, g)
    ref = pr.mc_heston_case(pkg, kind, g)
    assert ref["ambiguous"].max() <= 4
    X = h2.mc_points(pr.MC_HESTON_K)
    v, e, _ = mc_device(pkg, dev, spec, pr.MC_T_POINTS, X, h2.MC_STEPS, h2.MC_SAMPLES, pr.MC_SEED, L=L)
    print("value", v, ref["value"], "stderr", e, ref["stderr"])
    np.testing.assert_allclose(v, ref["value"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(e, ref["stderr"], rtol=RTOL, atol=ATOL)
    with pytest.raises(ValueError, match="Heston"):
        mc_device(pkg, dev, spec, pr.MC_T_POINTS, X, h2.MC_STEPS, h2.MC_SAMPLES, pr.MC_SEED, L=L, delta=True)


@pytest.mark.parametrize("name", ["put_mean", "put_sum"])
def test_mc_put_call_parity_on_the_device(pkg, dev, name):
    """One seed, the call and the put of the same problem: call - put ==
    e^{-phi_r tau} (mean_k s(X_T) - K), s the mean (sum) over the columns, from
    the restatement's terminal states, within the comparator tolerance applied
    to each of the two terms."""
    D, n_steps, mc = pr.MC_SHAPES[0]
    put, L = pr.mc_diag_spec(pkg, name, D)
    call, _ = pr.mc_diag_spec(pkg, name, D, call=True)
    ref = pr.mc_diag_case(pkg, name, pr.MC_SHAPES[0])
    X = pr.mc_points(D)
    vp, _, _ = mc_device(pkg, dev, put, pr.MC_T_POINTS, X, n_steps, mc, pr.MC_SEED)
    vc, _, _ = mc_device(pkg, dev, call, pr.MC_T_POINTS, X, n_steps, mc, pr.MC_SEED)
    tau = np.float32(pr.T) - pr.MC_T_POINTS
    want = np.exp(-float(np.float32(put.phi_r)) * tau.astype(np.float64)) * (ref["mean_XT"] - float(np.float32(put.strike)))
    diff = vc.astype(np.float64) - vp.astype(np.float64)
    tol = (ATOL + RTOL * np.abs(vc)) + (ATOL + RTOL * np.abs(vp))
    print("call", vc, "put", vp, "call - put", diff, "forward", want, "tol", tol)
    live = [0, 1, 2, 4]                               # (point 3 is at maturity: one of the two payoffs is 0)
    assert np.all(vp[live] > 0) and np.all(vc[live] > 0)
    assert np.all(np.abs(diff - want) <= tol), np.abs(diff - want) / tol


# ------------------------------------------------------------------ 5. closed forms
def exact_device(pkg, dev, kind, t, X, Tm, params):
    p, d = pkg.exact(kind, torch.from_numpy(t).to(dev), torch.from_numpy(X).to(dev), Tm, params)
    torch.cuda.synchronize()
    return p.cpu().numpy(), d.cpu().numpy()


def fp32_close(got, want, what):
    """got is the fp32 rounding of an fp64 value equal to want up to fp64
    rounding of the same formula: 2^-23 relative, and one denormal step."""
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max err / (2^-23 |ref|) = {(err / (F32_EPS * np.abs(want) + 1e-45)).max():.3f}")
    assert np.all(err <= F32_EPS * np.abs(want) + 1.5e-45), what


@pytest.mark.parametrize("kind", ["bs_put", "basket_avg_put", "basket_mean_put"])
def test_black_scholes_puts_on_the_device(pkg, dev, kind):
    """64 points over tests/test_gpu_heston2.py's domain (D = 3 columns, S in
    [0.5, 2], tau in [0, 2]; tau = 0 at, out of and in the money first), then
    the deep out-of-the-money point S / K = 2, tau = 0.05 in every column: about
    1e-15 against a call of 1, held to 2^-23 relative like every other point.
    Device parity with the call kind: |C - P - (S' - K e^{-r tau})| <=
    2^-24 (|C| + |P|) + 2^-24 |S' - K e^{-r tau}|."""
    S, _, tau = pr.closed_form_points()
    rs = np.random.RandomState(22)
    X = np.stack([S, rs.uniform(0.5, 2.0, 64).astype(np.float32), rs.uniform(0.5, 2.0, 64).astype(np.float32)], 1)
    X[:3, 1:] = X[:3, :1]                               # the maturity rows: every column on the same side
    X, tau = np.concatenate([X, np.full((1, 3), pr.DEEP_OTM["S"], np.float32)]), np.append(tau, np.float32(pr.DEEP_OTM["tau"]))
    Tm = 2.0
    t = (np.float32(Tm) - tau).astype(np.float32)
    tau64 = Tm - t.astype(np.float64)                  # what the kernel sees
    # basket_avg prices with sigma / sqrt(D): sigma sqrt(D) keeps its deep point the same normal fp32 number
    params = (pr.BS["r"], pr.BS["sig"] * (np.sqrt(3.0) if kind == "basket_avg_put" else 1.0), pr.BS["K"])
    want_p, want_d = pr.exact_put(kind, X.astype(np.float64), tau64, *params)
    p, d = exact_device(pkg, dev, kind, t, X, Tm, params)
    ncol = 3 if kind == "bs_put" else 1
    assert p.shape == (65, ncol) and d.shape == (65, ncol)
    fp32_close(p, want_p, f"{kind} price")
    fp32_close(d, want_d, f"{kind} delta")
    np.testing.assert_array_equal(p[:3, 0], [0.0, 0.0, 0.5])
    np.testing.assert_array_equal(d[:3, 0], [0.0, -0.5, -1.0])
    print(f"deep out of the money: device {p[64, 0]:.6e}, fp64 {want_p[64, 0]:.6e}")
    assert 2.0 ** -126 < p[64, 0] < 1e-13 and abs(float(p[64, 0]) - want_p[64, 0]) <= F32_EPS * want_p[64, 0]
    c, cd = exact_device(pkg, dev, {"bs_put": "bs_call", "basket_avg_put": "basket_avg", "basket_mean_put": "basket_mean"}[kind],
                         t, X, Tm, params)
    Sx = X.astype(np.float64) if kind == "bs_put" else X.astype(np.float64).mean(1, keepdims=True)
    fwd = Sx - params[2] * np.exp(-params[0] * np.maximum(tau64, 0.0))[:, None]
    gap = np.abs(c.astype(np.float64) - p.astype(np.float64) - fwd)
    bound = 2.0 ** -24 * (np.abs(c) + np.abs(p)) + 2.0 ** -24 * np.abs(fwd)
    print(f"{kind} parity: max gap / bound = {(gap / np.maximum(bound, 1e-300)).max():.3f}")
    assert np.all(gap <= bound)


@pytest.mark.parametrize("rho", [0.8, -0.7])
def test_heston_put_on_the_device(pkg, dev, rho):
    """tests/test_gpu_heston2.py's 64 points: the put against the restatement on
    the kernel's nodes (2^-23 relative: fp32 roundings of the same fp64
    arithmetic, the quadrature sum's order aside: + 1e-12 absolute), bitwise
    repeatable, and parity with the device's call, whose quadrature terms
    cancel in C - P."""
    S, v, tau = pr.closed_form_points()
    Tm = 2.0
    t = (np.float32(Tm) - tau).astype(np.float32)
    tau64 = Tm - t.astype(np.float64)
    want_p, want_d = pr.heston_put(S.astype(np.float64), v.astype(np.float64), tau64, rho=rho)
    X = np.stack([S, v], 1)
    params = (h2.R_RATE, 1.0, 2.0, 0.2, 0.3, rho)
    p, d = exact_device(pkg, dev, "heston_put", t, X, Tm, params)
    p2, d2 = exact_device(pkg, dev, "heston_put", t, X, Tm, params)
    c, cd = exact_device(pkg, dev, "heston", t, X, Tm, params)
    assert p.shape == (64, 1) and d.shape == (64, 1)
    p, d, c, cd = p[:, 0], d[:, 0], c[:, 0], cd[:, 0]
    ep, ed = np.abs(p - want_p), np.abs(d - want_d)
    print(f"rho={rho}: max|price err| = {ep.max():.3e}, max|delta err| = {ed.max():.3e}")
    assert np.all(ep <= F32_EPS * np.abs(want_p) + 1e-12) and np.all(ed <= F32_EPS * np.abs(want_d) + 1e-12)
    np.testing.assert_array_equal(p[:3], [0.0, 0.0, 0.5])
    np.testing.assert_array_equal(d[:3], [0.0, -0.5, -1.0])
    np.testing.assert_array_equal(p2[:, 0], p)
    np.testing.assert_array_equal(d2[:, 0], d)
    fwd = S.astype(np.float64) - np.exp(-h2.R_RATE * np.maximum(tau64, 0.0))
    gap = np.abs(c.astype(np.float64) - p.astype(np.float64) - fwd)
    bound = 2.0 ** -24 * (np.abs(c) + np.abs(p)) + 2.0 ** -24 * np.abs(fwd)
    print(f"parity: max gap / bound = {(gap / np.maximum(bound, 1e-300)).max():.3f}; delta parity max gap {np.abs(cd - d - 1).max():.2e}")
    assert np.all(gap <= bound)
    assert np.all(np.abs(cd.astype(np.float64) - d.astype(np.float64) - 1.0) <= 2.0 ** -23)


def test_mc_ties_to_the_heston_put(pkg, dev):
    """DESIGN 3.8's case, k = 1, (S, v, t) = (1, 0.2, 0), 100 steps, mc = 2^18:
    |mc - closed form| <= 4 stderr + 2 b + |(1 + r dt)^N - e^{rT}|, b the call's
    Euler bias bound (tests/heston2_reference.py).  P = C - e^{-rT}(S_T - K)
    path by path, so the put's bias is the call's up to the bias of E[S_T],
    which for this scheme's drift is S ((1 + r dt)^N - e^{rT})."""
    c = h2.EULER_TIE
    spec = h2.spec(pkg, 1, "put_mean")
    v, e, _ = mc_device(pkg, dev, spec, [c["t"]], [[c["S"], c["v"]]], c["n_steps"], c["mc"], 9)
    price, delta = pkg.exact("heston_put", torch.tensor([c["t"]], device=dev),
                             torch.tensor([[c["S"], c["v"]]], device=dev), h2.T, (h2.R_RATE, 1.0, 2.0, 0.2, 0.3, 0.8))
    torch.cuda.synchronize()
    cf = float(price[0, 0])
    drift = abs((1.0 + h2.R_RATE * h2.T / c["n_steps"]) ** c["n_steps"] - np.exp(h2.R_RATE * h2.T))
    bound = 4 * float(e[0]) + 2 * h2.EULER_BIAS_100 + drift
    print(f"mc {v[0]:.6f} +- {e[0]:.2e}, closed form {cf:.6f}, |diff| {abs(v[0] - cf):.2e}, bound {bound:.2e} "
          f"(drift term {drift:.2e})")
    assert -1 < float(delta[0, 0]) < 0 and cf > 0
    assert abs(v[0] - cf) <= bound


# ------------------------------------------------------------------ 6. the Python surface
def test_put_objects_train(pkg, dev):
    D, M, N = 8, 16, 6
    layers = [D + 1] + 4 * [16] + [1]
    for cls, g, strike in ((pkg.BasketPutOption, "put_mean", 1.0), (pkg.PutOption, "put_sum", 1.0 * D)):
        np.random.seed(3)
        torch.manual_seed(3)
        m = cls(np.ones((1, D)), 1.0, M, N, D, 1.0, layers, "Naisnet", "Tanh", device=dev)
        assert m.native_coefficients and m.generic_reason is None
        assert m.spec.g == g and m.strike == strike
        before = m.params.clone()
        out = m.train(3, 1e-3)
        torch.cuda.synchronize()
        graph, min_loss = out[0], out[1]
        assert np.isfinite(min_loss) and min_loss > 0
        print(cls.__name__, "losses", np.asarray(m.training_loss))
        assert len(m.training_loss) >= 1 and np.all(np.isfinite(np.asarray(m.training_loss, np.float64)))
        assert np.all(np.isfinite(np.asarray(graph, np.float64)))
        assert float((m.params - before).abs().max()) > 0
        val, err, dlt = m.mc_value(np.zeros(2, np.float32), np.ones((2, D), np.float32), mc=1024, delta=True)
        assert val.shape == (2, 1) and bool((val > 0).all()) and bool((dlt <= 0).all())


def test_closed_form_of_a_put_object(pkg, dev):
    np.random.seed(3)
    m = pkg.HestonTwoFactorFBSNN(np.ones((1, 1)), h2.T, 8, h2.N, 1, None, [2] + 4 * [16] + [1], "Naisnet", "Sine",
                                 device=dev, option_type="put")
    assert m.native_coefficients and m.spec.kind == "heston2" and m.spec.g == "put_mean"
    R = 5
    Sp, vp, tp = np.linspace(0.8, 1.2, R).astype(np.float32), np.full(R, 0.2, np.float32), np.linspace(0.0, 0.8, R).astype(np.float32)
    price, delta = m.closed_form(Sp, vp, tp)
    want_p, want_d = pkg.exact("heston_put", torch.from_numpy(tp).to(dev), torch.from_numpy(np.stack([Sp, vp], 1)).to(dev),
                               h2.T, (0.05, m.strike, m.kappa, m.theta, m.sigma, m.rho))
    torch.cuda.synchronize()
    assert torch.equal(price, want_p) and torch.equal(delta, want_d)
    assert bool(((delta > -1) & (delta < 0)).all()) and bool((price > 0).all())
    val, err, none = m.mc_value(tp, np.stack([Sp, vp], 1), mc=2048)
    assert float((price - val).abs().max()) < 0.05
    call = pkg.HestonTwoFactorFBSNN(np.ones((1, 1)), h2.T, 8, h2.N, 1, None, [2] + 4 * [16] + [1], "Naisnet", "Sine",
                                    device=dev)
    cp, cd = call.closed_form(Sp, vp, tp)
    assert call.option_type == "call" and call.spec.g == "call_mean" and bool((cd > 0).all())
    opt = m.new_optimizer_state("Adam", 1e-3)
    assert np.isfinite(float(m.device_step(opt, 1e-3, seed=3)))
