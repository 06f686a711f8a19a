"""Forward jets of the network (dbsde_net_u_jet: first and second directional
derivatives in z = (t, x), csrc/jet.hip), theta and the PDE residual
(dbsde_pde_residual, FBSNN.theta / FBSNN.pde_residual), against the oracle's
double autograd on the same weights, points and directions
(tests/jet_reference.py, torch CPU).

Tolerances: 1e-4 max|ref| for first derivatives (Du-like quantities), 2e-4
max|ref| for second-order ones and for every PDE term (as
tests/test_gpu_netu_xgrad.py uses them; the oracle's own fp32-vs-fp64
difference on these networks is <= 3.4e-6 max|ref|); the residual is read
against max(scale).  Needs a GPU."""
import os

import numpy as np
import pytest
import torch

import jet_reference as jr
from conftest import load_pkg
from oracle import fbsnn_ref as ref

pytestmark = pytest.mark.gpu

# the network forms of tests/test_gpu_netu_xgrad.py (form: the
# solver.matrix_form bit the case must run on; None: not pinned)
CASES = {
    "nais110_x3": ("NAIS-Net", [101] + 4 * [110] + [1], "Sine", 1),
    "naisnet16": ("Naisnet", [6] + 4 * [16] + [1], "Tanh", None),
    "fc256_chain": ("FC", [21] + 4 * [256] + [1], "Sine", 4),
    "fc256_fused_d100": ("FC", [101] + 4 * [256] + [1], "Sine", 1),
    "fc256_fused_d1": ("FC", [2] + 4 * [256] + [1], "Sine", 1),
    "resnet16": ("Resnet", [9] + 4 * [16] + [1], "Tanh", None),
}
FP32_ENV = {"DBSDE_X3": "0", "DBSDE_TNW_X3": "0"}


def shapes(case):
    """(R, nd): a tile holding a partial point, several points, padding rows."""
    D = CASES[case][1][0] - 1
    s = [(5, 3), (7, D + 1), (70, 4)]
    return s + [(20, 101)] if case == "nais110_x3" else s


RUNS = [(c, R, nd) for c in CASES for R, nd in shapes(c)]
RUN_IDS = [f"{c}-R{R}-nd{nd}" for c, R, nd in RUNS]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def make_model(pkg, dev, case, env=None, pin=True):
    """The case's model; env: variables set while its context is created."""
    mode, layers, act, form = CASES[case]
    D = layers[0] - 1
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        torch.manual_seed(0)
        m = pkg.BlackScholesBarenblatt(np.ones((1, D)), 1.0, 8, 5, D, layers, mode, act, device=dev)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if env and pin:
        assert m.solver.matrix_form & 1 == 0, f"expected the fp32-input fused form, got {m.solver.matrix_form}"
    elif form is not None:
        assert m.solver.matrix_form & form, f"expected matrix_form bit {form}, got {m.solver.matrix_form}"
    return m


def points(R, D):
    rs = np.random.RandomState(1)
    t = rs.uniform(0.0, 1.0, (R, 1)).astype(np.float32)
    X = (1.0 + 0.3 * rs.normal(size=(R, D))).astype(np.float32)
    return t, X


def directions(R, nd, D):
    """Random normal directions, the t component included."""
    return np.random.RandomState(2).normal(size=(R, nd, D + 1)).astype(np.float32)


_MODELS, _REFS = {}, {}


def model_of(pkg, dev, case):
    """The case's model and the oracle on its weights, built once."""
    if case not in _MODELS:
        m = make_model(pkg, dev, case)
        oracle = ref.build_model(*CASES[case][:3])
        ref.set_flat_params(oracle, m.params.cpu().numpy())
        _MODELS[case] = (m, oracle)
    return _MODELS[case]


def bundle(pkg, dev, case, R, nd):
    """Inputs and the oracle's jets of one (case, R, nd), computed once and
    shared by the tests below (none of them changes it)."""
    key = (case, R, nd)
    if key not in _REFS:
        m, oracle = model_of(pkg, dev, case)
        D = CASES[case][1][0] - 1
        t, X = points(R, D)
        V = directions(R, nd, D)
        d1, d2 = jr.jets(oracle, t, X, V)
        _REFS[key] = dict(m=m, oracle=oracle, t=t, X=X, V=V, d1=d1, d2=d2)
    return _REFS[key]


def native_jets(m, dev, t, X, V, want=("d1", "d2")):
    R, nd = V.shape[0], V.shape[1]
    out = {k: torch.full((R, nd), float("nan"), device=dev) for k in want}
    m.solver.net_u_jet(m.params, torch.from_numpy(t).to(dev).reshape(-1), torch.from_numpy(X).to(dev),
                       torch.from_numpy(np.ascontiguousarray(V)).to(dev), **out)
    torch.cuda.synchronize()
    return tuple(out[k].cpu().numpy() for k in want)


def check(got, want, tol, what, scale=None):
    scale = float(np.abs(want).max()) if scale is None else scale
    err = float(np.abs(got - want).max())
    print(f"{what}: max|err| = {err:.3e} = {err / scale if scale else float('nan'):.3e} max|ref| (bound {tol:.0e})")
    assert scale > 0 and np.all(np.isfinite(got))
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale)


# ------------------------------------------------------------------ 1. jets against the oracle
@pytest.mark.parametrize("case,R,nd", RUNS, ids=RUN_IDS)
def test_jets_match_oracle(pkg, dev, case, R, nd):
    b = bundle(pkg, dev, case, R, nd)
    d1, d2 = native_jets(b["m"], dev, b["t"], b["X"], b["V"])
    check(d1, b["d1"], 1e-4, f"d1 {case} R={R} nd={nd}")
    check(d2, b["d2"], 2e-4, f"d2 {case} R={R} nd={nd}")


# ------------------------------------------------------------------ 2. consistency with the existing API
@pytest.mark.parametrize("case", list(CASES))
def test_unit_directions_match_net_u_and_xvjp(pkg, dev, case):
    """Direction e_d: d1 = Du[:, d], d2 = the d-th component of H e_d, which
    net_u_xvjp(ubar = 0, zbar = e_d) returns."""
    m, _ = model_of(pkg, dev, case)
    D = CASES[case][1][0] - 1
    R = 7
    t, X = points(R, D)
    ds = sorted({0, D // 2, D - 1})
    V = np.zeros((R, len(ds), D + 1), np.float32)
    for j, d in enumerate(ds):
        V[:, j, 1 + d] = 1.0
    d1, d2 = native_jets(m, dev, t, X, V)
    td, Xd = torch.from_numpy(t).to(dev).reshape(-1), torch.from_numpy(X).to(dev)
    u, du = torch.empty(R, device=dev), torch.empty((R, D), device=dev)
    m.solver.net_u(m.params, td, Xd, u, du)
    du = du.cpu().numpy()
    check(d1, du[:, ds], 1e-4, f"d1(e_d) vs Du {case}", scale=float(np.abs(du).max()))
    hd = np.empty((R, len(ds)), np.float32)
    scale = 0.0
    for j, d in enumerate(ds):
        zbar = torch.zeros((R, D), device=dev)
        zbar[:, d] = 1.0
        xbar = torch.empty((R, D), device=dev)
        m.solver.net_u_xvjp(m.params, td, Xd, torch.zeros(R, device=dev), zbar, xbar=xbar)
        xb = xbar.cpu().numpy()
        hd[:, j] = xb[:, d]
        scale = max(scale, float(np.abs(xb).max()))
    check(d2, hd, 2e-4, f"d2(e_d) vs xvjp {case}", scale=scale)


@pytest.mark.parametrize("case", list(CASES))
def test_theta_matches_oracle_autograd(pkg, dev, case):
    m, oracle = model_of(pkg, dev, case)
    D = CASES[case][1][0] - 1
    t, X = points(70, D)
    got = m.theta(t, X)
    assert got.shape == (70, 1)
    check(got.cpu().numpy(), jr.theta(oracle, t, X), 1e-4, f"theta {case}")


# ------------------------------------------------------------------ 3. structure
@pytest.mark.parametrize("case", ["nais110_x3", "naisnet16", "fc256_chain"])
def test_structure(pkg, dev, case):
    b = bundle(pkg, dev, case, 70, 4)
    m, t, X, V = b["m"], b["t"], b["X"], b["V"]
    d1, d2 = native_jets(m, dev, t, X, V)
    # V = 0: exact zeros
    z1, z2 = native_jets(m, dev, t, X, np.zeros_like(V))
    assert np.all(z1 == 0) and np.all(z2 == 0)
    # bitwise repeatable
    r1, r2 = native_jets(m, dev, t, X, V)
    assert np.array_equal(r1, d1) and np.array_equal(r2, d2)
    # a subset of the points, evaluated alone
    sub = np.array([3, 17, 18, 40, 69])
    s1, s2 = native_jets(m, dev, t[sub], X[sub], V[sub])
    np.testing.assert_allclose(s1, d1[sub], rtol=0, atol=1e-6 * float(np.abs(d1).max()))
    np.testing.assert_allclose(s2, d2[sub], rtol=0, atol=1e-6 * float(np.abs(d2).max()))
    # each output alone
    (o1,) = native_jets(m, dev, t, X, V, want=("d1",))
    (o2,) = native_jets(m, dev, t, X, V, want=("d2",))
    assert np.array_equal(o1, d1) and np.array_equal(o2, d2)


def test_rows_cross_the_launch_cap(pkg, dev):
    """DBSDE_JET_CAP=64 (read at context creation): 280 jet rows in five
    launches, the boundaries inside points; the same values as one launch."""
    b = bundle(pkg, dev, "naisnet16", 70, 4)
    m = make_model(pkg, dev, "naisnet16", {"DBSDE_JET_CAP": "64"}, pin=False)
    assert torch.equal(m.params, b["m"].params)
    d1, d2 = native_jets(m, dev, b["t"], b["X"], b["V"])
    check(d1, b["d1"], 1e-4, "d1 capped")
    check(d2, b["d2"], 2e-4, "d2 capped")
    f1, f2 = native_jets(b["m"], dev, b["t"], b["X"], b["V"])
    assert np.array_equal(d1, f1) and np.array_equal(d2, f2)


# ------------------------------------------------------------------ 4. fp32-input contexts
@pytest.mark.parametrize("case", ["nais110_x3", "naisnet16"])
def test_jets_behind_the_fp32_input_phase_kernels(pkg, dev, case):
    """A context created under DBSDE_X3=0 DBSDE_TNW_X3=0 runs the same jet kernels."""
    m = make_model(pkg, dev, case, FP32_ENV)
    for R, nd in shapes(case):
        b = bundle(pkg, dev, case, R, nd)
        assert torch.equal(m.params, b["m"].params)
        d1, d2 = native_jets(m, dev, b["t"], b["X"], b["V"])
        check(d1, b["d1"], 1e-4, f"d1 fp32 form {case} R={R} nd={nd}")
        check(d2, b["d2"], 2e-4, f"d2 fp32 form {case} R={R} nd={nd}")


# ------------------------------------------------------------------ 5. ReLU
def test_relu_second_derivative_is_exactly_zero(pkg, dev):
    layers, R, D = [9, 16, 16, 16, 16, 1], 32, 8
    torch.manual_seed(3)
    oracle = ref.build_model("FC", layers, "ReLU")
    m = pkg.BlackScholesBarenblatt(np.ones((1, D)), 1.0, 8, 5, D, layers, "FC", "ReLU", device=dev)
    m.params.copy_(torch.from_numpy(ref.flat_params(oracle).astype(np.float32)).to(dev))
    t, X = points(R, D)
    # no hidden unit of any row sits at the kink: the oracle alone decides every branch
    with torch.no_grad():
        h, low = torch.cat((torch.from_numpy(t), torch.from_numpy(X)), 1), np.inf
        for mod in list(oracle)[:-1]:
            h = mod(h)
            if isinstance(mod, torch.nn.Linear):
                low = min(low, float(h.abs().min()))
    print(f"min|pre-activation| = {low:.3e}")
    assert low > 1e-4, low
    V = directions(R, 4, D)
    r1, r2 = jr.jets(oracle, t, X, V)
    assert np.all(r2 == 0)
    d1, d2 = native_jets(m, dev, t, X, V)
    assert np.all(d2 == 0)
    check(d1, r1, 1e-4, "d1 relu")


# ------------------------------------------------------------------ 6. Heston clamp
HESTON_SEED = 42


def heston_setup(pkg, dev, k=1, seed=HESTON_SEED):
    """The set-up of tests/test_gpu_netu_xgrad.py's heston_setup (k = 1,
    R = 48): the output bias is moved to the median raw output, so about half
    of the rows clamp; the weights are drawn on the CPU so that the seed alone
    fixes them, and every raw output stays more than 1e-4 away from zero."""
    layers, act, R = [2] + 4 * [16] + [1], "Tanh", 48
    torch.manual_seed(seed)
    oracle = ref.build_heston_model("Naisnet", layers, act, k)
    m = pkg.HestonFBSNN(np.ones((1, k)), 1.0, 8, 5, k, None, layers, "Naisnet", act, device=dev)
    rs = np.random.RandomState(5)
    t = rs.uniform(0.0, 1.0, (R, 1)).astype(np.float32)
    X = np.concatenate([1.0 + 0.3 * rs.normal(size=(R, k)), 0.2 + 0.05 * rs.uniform(size=(R, k))], 1).astype(np.float32)
    flat = ref.flat_params(oracle).astype(np.float32)
    with torch.no_grad():
        raw = oracle(torch.cat([torch.from_numpy(t), torch.from_numpy(X)], 1)).numpy().ravel()
    assert list(m.model.state_dict())[-1].endswith("bias")
    flat[-1] -= np.float32(np.median(raw))
    ref.set_flat_params(oracle, flat)
    m.params.copy_(torch.from_numpy(flat).to(dev))
    with torch.no_grad():
        raw = oracle(torch.cat([torch.from_numpy(t), torch.from_numpy(X)], 1)).numpy().ravel()
    clamped = raw < 0
    assert 0.25 * R < int(clamped.sum()) < 0.75 * R, int(clamped.sum())
    assert float(np.abs(raw).min()) > 1e-4, float(np.abs(raw).min())   # the reference alone decides every mask
    return m, oracle, t, X, clamped, rs


def test_heston_jets_through_the_clamp(pkg, dev):
    m, oracle, t, X, clamped, rs = heston_setup(pkg, dev)
    R, D = X.shape
    V = rs.normal(size=(R, 3, D + 1)).astype(np.float32)
    r1, r2 = jr.jets(oracle, t, X, V, clamp=True)
    assert np.all(r1[clamped] == 0) and np.all(r2[clamped] == 0)
    d1, d2 = native_jets(m, dev, t, X, V)
    assert np.all(d1[clamped] == 0) and np.all(d2[clamped] == 0)
    check(d1[~clamped], r1[~clamped], 1e-4, "heston d1")
    check(d2[~clamped], r2[~clamped], 2e-4, "heston d2")
    # (HestonFBSNN.theta is the reference's model parameter: the method is u_t there)
    th = m.u_t(t, X).cpu().numpy()
    assert np.all(th[clamped] == 0)
    check(th, jr.theta(oracle, t, X, clamp=True), 1e-4, "heston theta")


# ------------------------------------------------------------------ 7. pde_residual per problem
def check_terms(got, want, what):
    """Every term within 2e-4 max|term|; the residual within 2e-4 max(scale)."""
    assert set(got) == set(jr.TERMS)
    smax = float(np.abs(want["scale"]).max())
    for k in jr.TERMS:
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        assert g.shape == want[k].shape, (k, g.shape)
        top = smax if k == "residual" else float(np.abs(want[k]).max())
        if top == 0:   # a term the problem does not have (mu = 0): exactly zero
            print(f"{what} {k}: identically zero")
            assert np.all(g == 0), k
        else:
            check(g, want[k], 2e-4, f"{what} {k}", scale=top)


def _problem_model(pkg, dev, name):
    """(model, oracle model, oracle problem, L, R) of one native problem."""
    torch.manual_seed(0)
    np.random.seed(0)
    if name == "bsb":
        D, mode, layers, act, R = 100, "NAIS-Net", [101] + 4 * [110] + [1], "Sine", 20
        m = pkg.BlackScholesBarenblatt(np.ones((1, D)), 1.0, 8, 5, D, layers, mode, act, device=dev)
    elif name == "basket":
        D, mode, layers, act, R = 8, "Naisnet", [9] + 4 * [16] + [1], "Tanh", 20
        m = pkg.BasketCallOption(np.ones((1, D)), 1.0, 8, 5, D, 1.0, layers, mode, act,
                                 correlation_type="random_correlation", device=dev)
        assert m._L is not None and np.abs(np.tril(m._L, -1)).max() > 0
    elif name == "hjb":
        D, mode, layers, act, R = 20, "FC", [21] + 4 * [256] + [1], "Sine", 40
        m = pkg.HamiltonJacobiBellman(np.ones((1, D)), 1.0, 8, 5, D, layers, mode, act, device=dev)
    else:
        D, mode, layers, act, R = 1, "Naisnet", [2] + 4 * [16] + [1], "Tanh", 20
        m = pkg.CallOption1D(np.ones((1, D)), 1.0, 8, 5, D, 1.0, layers, mode, act, device=dev)
    assert m.native_coefficients
    oracle = ref.build_model(mode, layers, act)
    ref.set_flat_params(oracle, m.params.cpu().numpy())
    return m, oracle, ref.make_problem(name, D), m._L, R, D


@pytest.mark.parametrize("name", ["bsb", "basket", "hjb", "call1d"])
def test_pde_residual_matches_reference(pkg, dev, name):
    m, oracle, problem, L, R, D = _problem_model(pkg, dev, name)
    t, X = points(R, D)
    want = jr.pde_terms(oracle, problem, t, X, L=L)
    got = m.pde_residual(t, X)
    torch.cuda.synchronize()
    check_terms(got, want, name)


@pytest.mark.parametrize("k", [1, 2])
def test_heston_pde_residual_matches_reference(pkg, dev, k):
    m, oracle, t, X, clamped, _ = heston_setup(pkg, dev, k)
    want = jr.heston_pde_terms(oracle, t, X, k, m.kappa, m.theta, m.sigma, m.rho)
    got = m.pde_residual(t, X)
    torch.cuda.synchronize()
    check_terms(got, want, f"heston k={k}")
    for key in jr.TERMS:
        assert np.all(got[key].cpu().numpy()[clamped] == 0), key


# ------------------------------------------------------------------ 8. plugin problems
def test_plugin_problem_returns_the_native_terms(pkg, dev):
    """sigma = 0.3 Black-Scholes-Barenblatt defined the reference's way (no
    problem_spec: its own coefficient methods run) against the native context
    of the same problem (sig_a = 0.3) on the same weights."""
    D, R = 8, 20
    layers = [D + 1, 16, 16, 16, 16, 1]

    class Plugin(pkg.FBSNN):
        def phi_tf(self, t, X, Y, Z):
            return 0.05 * (Y - torch.sum(X * Z, dim=1, keepdim=True))

        def g_tf(self, X):
            return torch.sum(X ** 2, 1, keepdim=True)

        def sigma_tf(self, t, X, Y):
            return 0.3 * torch.diag_embed(X)

    class Native(pkg.BlackScholesBarenblatt):
        def problem_spec(self):
            return pkg.ProblemSpec(sig_a=0.3, phi_r=0.05, phi_c=1.0, g="sumsq")

        def sigma_tf(self, t, X, Y):
            return 0.3 * torch.diag_embed(X)

    torch.manual_seed(0)
    p = Plugin(np.ones((1, D)), 1.0, 8, 5, D, None, layers, "Naisnet", "Sine", device=dev)
    n = Native(np.ones((1, D)), 1.0, 8, 5, D, layers, "Naisnet", "Sine", device=dev)
    assert not p.native_coefficients and n.native_coefficients
    n.params.copy_(p.params)
    t, X = points(R, D)
    want = {k: v.cpu().numpy() for k, v in n.pde_residual(t, X).items()}
    got = p.pde_residual(t, X)
    torch.cuda.synchronize()
    assert float(np.abs(want["diffusion"]).max()) > 0
    check_terms(got, want, "plugin")


# ------------------------------------------------------------------ prefetch state
def test_a_prefetched_rollout_survives_jet_calls(pkg, dev):
    """dbsde_prefetch, then net_u_jet and pde_residual, then the step that
    consumes the batch: bit-identical X, loss and gradient to a step that
    rolls out itself (as with dbsde_net_u in between)."""
    D, M, N = 8, 64, 10
    spec = pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, g="call_mean", strike=1.0)
    s = pkg.NativeSolver("Naisnet", [D + 1, 16, 16, 16, 16, 1], "Tanh", spec, 1.0, dev)
    rs = np.random.RandomState(3)
    params = torch.from_numpy(rs.normal(scale=0.3, size=s.nparams).astype(np.float32)).to(dev)
    Xi = torch.ones(D, device=dev)

    def step(seed):
        X = torch.empty(M * (N + 1) * D, device=dev)
        grad, loss = torch.empty_like(params), torch.empty(1, device=dev)
        s.loss_grad(params, M, N, Xi, seed=seed, grad=grad, loss=loss, X=X)
        torch.cuda.synchronize()
        return X.cpu().numpy(), float(loss), grad.cpu().numpy()

    want = step(5)
    t, X = points(20, D)
    td, Xd = torch.from_numpy(t).to(dev).reshape(-1), torch.from_numpy(X).to(dev)
    V = torch.from_numpy(directions(20, 3, D)).to(dev)
    d2 = torch.empty((20, 3), device=dev)
    res = torch.empty(20, device=dev)
    s.net_u_jet(params, td, Xd, V, d2=d2)
    s.pde_residual(params, td, Xd, residual=res)
    torch.cuda.synchronize()
    first = (d2.cpu().numpy(), res.cpu().numpy())
    s.prefetch(M, N, Xi, seed=5)
    s.net_u_jet(params, td, Xd, V, d2=d2)
    s.pde_residual(params, td, Xd, residual=res)
    got = step(5)
    np.testing.assert_array_equal(got[0], want[0])
    assert got[1] == want[1]
    np.testing.assert_array_equal(got[2], want[2])
    assert np.array_equal(d2.cpu().numpy(), first[0]) and np.array_equal(res.cpu().numpy(), first[1])
    assert np.all(np.isfinite(first[0])) and np.all(np.isfinite(first[1]))
