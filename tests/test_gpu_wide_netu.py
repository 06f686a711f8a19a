"""The net_u family at state dimensions above 126: dbsde_net_u (column-tiled Z
GEMM), dbsde_net_u_vjp, dbsde_net_u_xvjp (netu_xbar_wide_kernel: output blocks
in passes of 8), dbsde_net_u_jet and dbsde_pde_residual (more than 64 KB of
dynamic LDS at Dp = 1024), against the oracle's autograd (oracle/fbsnn_ref.py,
tests/jet_reference.py; torch CPU) on the same weights and points.

Bounds: tests/test_gpu_netu_vjp.py (u, Du abs 1e-4 max(1, |ref|max); parameter
gradient 2e-4 max|ref|), tests/test_gpu_netu_xgrad.py (xbar 2e-4 max|ref|) and
tests/test_gpu_jet.py (d1 1e-4, d2 2e-4 max|ref|; every PDE term 2e-4
max|term|, the residual 2e-4 max(scale)).  Needs a GPU."""
import numpy as np
import pytest
import torch

import jet_reference as jr
from conftest import load_pkg
from oracle import fbsnn_ref as ref

pytestmark = pytest.mark.gpu
T = 1.0
R = 37
CASES = {
    "fc64_d200": ("FC", 200, 64, "Tanh"),
    "nais48_d1022": ("NAIS-Net", 1022, 48, "Sine"),
}


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def check(got, want, tol, what, scale=None):
    scale = float(np.abs(want).max()) if scale is None else scale
    err = float(np.abs(got - want).max())
    print(f"{what}: max|err| = {err:.3e} = {err / scale if scale else float('nan'):.3e} max|ref| (bound {tol:.0e})")
    assert scale > 0 and np.all(np.isfinite(got))
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale)


_B = {}


def bundle(pkg, dev, case):
    """Solver, weights, points, cotangents and the oracle's results of one
    case, built once and shared by the tests below (none of them changes it)."""
    if case not in _B:
        mode, D, width, act = CASES[case]
        layers = [D + 1] + 4 * [width] + [1]
        torch.manual_seed(D)
        oracle = ref.build_model(mode, layers, act)
        params = ref.flat_params(oracle)
        rs = np.random.RandomState(1)
        t = rs.uniform(0.0, 1.0, (R, 1)).astype(np.float32)
        X = (1.0 + 0.3 * rs.normal(size=(R, D))).astype(np.float32)
        gu = rs.normal(size=(R, 1)).astype(np.float32)
        gdu = rs.normal(size=(R, D)).astype(np.float32)
        Xr = torch.from_numpy(X).requires_grad_(True)
        ur, dur = ref.net_u(oracle, torch.from_numpy(t), Xr)
        full = (torch.from_numpy(gu) * ur).sum() + (torch.from_numpy(gdu) * dur).sum()
        xb = torch.autograd.grad(full, Xr, retain_graph=True)[0].numpy()
        oracle.zero_grad(set_to_none=True)
        full.backward()
        g_ref, used = ref.flat_grads(oracle)
        spec = pkg.ProblemSpec(sig_a=0.4, phi_r=0.05, phi_c=1.0, g="sumsq")
        s = pkg.NativeSolver(mode, layers, act, spec, T, dev)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        _B[case] = dict(s=s, oracle=oracle, D=D, t=t, X=X, params=d(params), td=d(t.reshape(-1)), Xd=d(X),
                        gud=d(gu.reshape(-1)), gdud=d(gdu), u=ur.detach().numpy(), du=dur.detach().numpy(), xb=xb,
                        g_ref=g_ref, used=used)
    return _B[case]


@pytest.mark.parametrize("case", list(CASES))
def test_net_u_matches_oracle(pkg, dev, case):
    b = bundle(pkg, dev, case)
    u, du = torch.empty(R, device=dev), torch.empty(R, b["D"], device=dev)
    b["s"].net_u(b["params"], b["td"], b["Xd"], u, du)
    torch.cuda.synchronize()
    check(u.cpu().numpy().reshape(R, 1), b["u"], 1e-4, f"u {case}", scale=max(1.0, float(np.abs(b["u"]).max())))
    check(du.cpu().numpy(), b["du"], 1e-4, f"Du {case}", scale=max(1.0, float(np.abs(b["du"]).max())))


@pytest.mark.parametrize("case", list(CASES))
def test_vjp_and_xvjp_match_oracle_autograd(pkg, dev, case):
    b = bundle(pkg, dev, case)
    s, used = b["s"], b["used"]
    args = (b["params"], b["td"], b["Xd"], b["gud"], b["gdud"])
    scale = float(np.abs(b["g_ref"][used]).max())

    def grads_ok(g, what):
        g = g.cpu().numpy()
        check(g[used], b["g_ref"][used], 2e-4, what, scale=scale)
        assert np.all(g[~used] == 0.0)

    g = torch.full_like(b["params"], float("nan"))
    s.net_u_vjp(*args, g)
    torch.cuda.synchronize()
    grads_ok(g, f"vjp grad {case}")
    # xbar alone, grad alone, both
    x1 = torch.full((R, b["D"]), float("nan"), device=dev)
    s.net_u_xvjp(*args, xbar=x1)
    g2 = torch.full_like(b["params"], float("nan"))
    s.net_u_xvjp(*args, grad=g2)
    g3, x3 = torch.full_like(b["params"], float("nan")), torch.full((R, b["D"]), float("nan"), device=dev)
    s.net_u_xvjp(*args, grad=g3, xbar=x3)
    torch.cuda.synchronize()
    check(x1.cpu().numpy(), b["xb"], 2e-4, f"xbar alone {case}")
    check(x3.cpu().numpy(), b["xb"], 2e-4, f"xbar with grad {case}")
    grads_ok(g2, f"xvjp grad alone {case}")
    grads_ok(g3, f"xvjp grad with xbar {case}")
    torch.testing.assert_close(g2, g, rtol=0, atol=0)
    torch.testing.assert_close(g3, g, rtol=0, atol=0)
    torch.testing.assert_close(x3, x1, rtol=0, atol=0)      # fixed summation order: bitwise repeatable


@pytest.mark.parametrize("case", list(CASES))
def test_jets_match_oracle(pkg, dev, case):
    """nd = 3 random directions and e_t."""
    b = bundle(pkg, dev, case)
    D = b["D"]
    V = np.random.RandomState(2).normal(size=(R, 4, D + 1)).astype(np.float32)
    V[:, 3, :] = 0.0
    V[:, 3, 0] = 1.0
    r1, r2 = jr.jets(b["oracle"], b["t"], b["X"], V)
    d1, d2 = (torch.full((R, 4), float("nan"), device=dev) for _ in range(2))
    b["s"].net_u_jet(b["params"], b["td"], b["Xd"], torch.from_numpy(V).to(dev), d1=d1, d2=d2)
    torch.cuda.synchronize()
    check(d1.cpu().numpy(), r1, 1e-4, f"d1 {case}")
    check(d2.cpu().numpy(), r2, 2e-4, f"d2 {case}")


# ------------------------------------------------------------------ pde_residual at D = 200
def check_terms(got, want, what):
    """Every term within 2e-4 max|term|; the residual within 2e-4 max(scale)."""
    smax = float(np.abs(want["scale"]).max())
    for k in jr.TERMS:
        g = got[k].cpu().numpy().reshape(-1, 1)
        top = smax if k == "residual" else float(np.abs(want[k]).max())
        if top == 0:   # a term the problem does not have (mu = 0): exactly zero
            assert np.all(g == 0), k
        else:
            check(g, want[k], 2e-4, f"{what} {k}", scale=top)


def native_terms(s, dev, params, t, X):
    P = X.shape[0]
    out = {k: torch.full((P,), float("nan"), device=dev) for k in jr.TERMS}
    s.pde_residual(torch.from_numpy(params).to(dev), torch.from_numpy(t.reshape(-1)).to(dev), torch.from_numpy(X).to(dev),
                   **out)
    torch.cuda.synchronize()
    return out


def points8(D):
    rs = np.random.RandomState(1)
    return rs.uniform(0.0, 1.0, (8, 1)).astype(np.float32), (1.0 + 0.3 * rs.normal(size=(8, D))).astype(np.float32)


@pytest.mark.parametrize("corr", [False, True], ids=["diagonal", "correlated"])
def test_pde_residual_wide(pkg, dev, corr):
    """201 directions per point (e_t and the 200 diffusion columns)."""
    D = 200
    layers = [D + 1] + 4 * [48] + [1]
    torch.manual_seed(11)
    oracle = ref.build_model("NAIS-Net", layers, "Sine")
    params = ref.flat_params(oracle)
    spec = pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=0.0, g="call_mean", strike=1.0)
    s = pkg.NativeSolver("NAIS-Net", layers, "Sine", spec, T, dev)
    L = None
    if corr:
        rs = np.random.RandomState(D)
        A = rs.normal(size=(D, D))
        C = A @ A.T + D * np.eye(D)
        d = np.sqrt(np.diag(C))
        L = np.linalg.cholesky(C / np.outer(d, d)).astype(np.float32)
        s.set_corr(L)
    t, X = points8(D)
    want = jr.pde_terms(oracle, ref.make_problem("basket", D), t, X, L=L)
    check_terms(native_terms(s, dev, params, t, X), want, "basket200" + ("_corr" if corr else ""))


def test_heston_pde_residual_wide(pkg, dev):
    """k = 100 (state 200).  The output bias is moved so that half of the
    points clamp (tests/test_gpu_jet.py heston_setup); every raw output stays
    more than 1e-4 from zero, so the reference alone decides every mask."""
    k = 100
    layers = [1 + 2 * k] + 4 * [16] + [1]
    torch.manual_seed(42)
    oracle = ref.build_heston_model("Naisnet", [2] + layers[1:], "Tanh", k)
    rs = np.random.RandomState(5)
    t = rs.uniform(0.0, 1.0, (8, 1)).astype(np.float32)
    X = np.concatenate([1.0 + 0.3 * rs.normal(size=(8, k)), 0.2 + 0.05 * rs.uniform(size=(8, k))], 1).astype(np.float32)
    flat = ref.flat_params(oracle).astype(np.float32)
    z = torch.cat([torch.from_numpy(t), torch.from_numpy(X)], 1)
    with torch.no_grad():
        flat[-1] -= np.float32(np.median(oracle(z).numpy().ravel()))
        ref.set_flat_params(oracle, flat)
        raw = oracle(z).numpy().ravel()
    clamped = raw < 0
    assert 2 <= int(clamped.sum()) <= 6 and float(np.abs(raw).min()) > 1e-4, raw
    spec = pkg.ProblemSpec(kind="heston", mu_a=0.05, phi_r=0.05, g="call_mean", strike=1.0, g_alpha=10.0, g_cols=k,
                           u_clamp=True, q3=False, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8)
    s = pkg.NativeSolver("Naisnet", layers, "Tanh", spec, T, dev)
    want = jr.heston_pde_terms(oracle, t, X, k, 2.0, 0.2, 0.3, 0.8)
    got = native_terms(s, dev, flat, t, X)
    check_terms(got, want, "heston k=100")
    for key in jr.TERMS:
        assert np.all(got[key].cpu().numpy()[clamped] == 0), key
