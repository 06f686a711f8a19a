"""FBSNN.net_u differentiated in the points X (the reference's own callers do:
StabilityCheck's torch.autograd.functional.jacobian(net_u, S),
with_corr_high_dimension_pde.py:856-877, and HestonFBSNN.calculate_greeks'
gamma = autograd.grad(delta, S), heston_dnnpde.py:685-699).

The native backward is dbsde_net_u_xvjp: for cotangents (gu, gdu) on (u, Du)

    xbar_r = d/dX_r [gu_r u_r + gdu_r . Du_r] = gu_r Du_r + H_r gdu_r,

the reverse cotangents alpha_j of the loss_grad backward contracted with the
input-facing weights by one split-bf16 kernel (csrc/xbar.hip) behind every
network form.  Checked against the oracle's autograd (oracle/fbsnn_ref.py
net_u / heston_net_u, torch CPU) on the same weights, points and cotangents.

Tolerances: 2e-4 max|ref| for gradients (the oracle's own
fp32-vs-fp64 difference on these cases is <= 3.4e-6 max), 1e-4 max for Du-like
quantities (the Jacobian of u is Du).  Needs a GPU."""
import os

import numpy as np
import pytest
import torch

from conftest import load_pkg
from oracle import fbsnn_ref as ref

pytestmark = pytest.mark.gpu

# form: the solver.matrix_form bit the case must run on (1 = the fused
# split-bf16 phase kernels, 4 = the split-bf16 per-layer chain; None: not pinned)
CASES = {
    "nais110_x3": ("NAIS-Net", [101] + 4 * [110] + [1], "Sine", 1),
    "naisnet16": ("Naisnet", [6] + 4 * [16] + [1], "Tanh", None),
    "fc256_chain": ("FC", [21] + 4 * [256] + [1], "Sine", 4),
    "fc256_fused_d100": ("FC", [101] + 4 * [256] + [1], "Sine", 1),
    "fc256_fused_d1": ("FC", [2] + 4 * [256] + [1], "Sine", 1),
    "resnet16": ("Resnet", [9] + 4 * [16] + [1], "Tanh", None),
}
RUNS = [(c, 70) for c in CASES] + [("nais110_x3", 96)]
RUN_IDS = [f"{c}-R{r}" for c, r in RUNS]
FP32_ENV = {"DBSDE_X3": "0", "DBSDE_TNW_X3": "0"}


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def make_model(pkg, dev, case, env=None):
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
    if env:
        assert m.solver.matrix_form & 1 == 0, f"expected the fp32-input fused form, got {m.solver.matrix_form}"
    elif form is not None:
        assert m.solver.matrix_form & form, f"expected matrix_form bit {form}, got {m.solver.matrix_form}"
    return m


def points(R, D):
    rs = np.random.RandomState(1)
    t = rs.uniform(0.0, 1.0, (R, 1)).astype(np.float32)
    X = (1.0 + 0.3 * rs.normal(size=(R, D))).astype(np.float32)
    gu = rs.normal(size=(R, 1)).astype(np.float32)
    gdu = rs.normal(size=(R, D)).astype(np.float32)
    return t, X, gu, gdu


def oracle_xbar(net_u, oracle, t, X, gu, gdu):
    """(d/dX [gu u + gdu . Du], d/dX [gdu . Du]) by the oracle's autograd."""
    Xr = torch.from_numpy(X).requires_grad_(True)
    ur, dur = net_u(oracle, torch.from_numpy(t), Xr)
    hz = (torch.from_numpy(gdu) * dur).sum()
    full = (torch.from_numpy(gu) * ur).sum() + hz
    xb = torch.autograd.grad(full, Xr, retain_graph=True)[0].numpy()
    xh = torch.autograd.grad(hz, Xr)[0].numpy()
    return xb, xh, ur.detach().numpy(), dur.detach().numpy()


_BUNDLES = {}


def bundle(pkg, dev, case, R):
    """Model, inputs and the oracle's references of one (case, R), built once
    and shared by the tests below (none of them changes it)."""
    key = (case, R)
    if key not in _BUNDLES:
        m = _BUNDLES[(case, None)] if (case, None) in _BUNDLES else make_model(pkg, dev, case)
        _BUNDLES[(case, None)] = m
        D = CASES[case][1][0] - 1
        oracle = ref.build_model(*CASES[case][:3])
        ref.set_flat_params(oracle, m.params.cpu().numpy())
        t, X, gu, gdu = points(R, D)
        xb, xh, _, _ = oracle_xbar(ref.net_u, oracle, t, X, gu, gdu)
        _BUNDLES[key] = dict(m=m, oracle=oracle, t=t, X=X, gu=gu, gdu=gdu, xb=xb, xh=xh)
    return _BUNDLES[key]


def native_xbar(m, dev, t, X, gu, gdu):
    """X.grad of one backward of (gu u).sum() + (gdu Du).sum(); gu None: the
    second term alone."""
    Xg = torch.from_numpy(X).to(dev).requires_grad_(True)
    u, du = m.net_u(t, Xg)
    assert u.requires_grad and du.requires_grad
    loss = (torch.from_numpy(gdu).to(dev) * du).sum()
    if gu is not None:
        loss = loss + (torch.from_numpy(gu).to(dev) * u).sum()
    loss.backward()
    assert Xg.grad is not None and Xg.grad.shape == Xg.shape
    return Xg.grad.cpu().numpy()


def flat_param_grad(m):
    named = dict(m.model.named_parameters())
    return torch.cat([(named[n].grad if named[n].grad is not None else torch.zeros_like(named[n])).reshape(-1)
                      for n in m.model.state_dict()])


def check(got, want, tol, what):
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print(f"{what}: max|err| = {err:.3e} = {err / scale:.3e} max|ref| (bound {tol:.0e})")
    assert scale > 0 and np.all(np.isfinite(got))
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale)


@pytest.mark.parametrize("case,R", RUNS, ids=RUN_IDS)
def test_xbar_matches_reference_autograd(pkg, dev, case, R):
    b = bundle(pkg, dev, case, R)
    b["m"].model.zero_grad(set_to_none=True)
    got = native_xbar(b["m"], dev, b["t"], b["X"], b["gu"], b["gdu"])
    check(got, b["xb"], 2e-4, f"xbar {case} R={R}")


@pytest.mark.parametrize("case,R", RUNS, ids=RUN_IDS)
def test_hessian_vector_product_alone(pkg, dev, case, R):
    """gu = 0: xbar = H gdu, the term an implementation that returned gu Du
    alone would miss entirely."""
    b = bundle(pkg, dev, case, R)
    b["m"].model.zero_grad(set_to_none=True)
    got = native_xbar(b["m"], dev, b["t"], b["X"], None, b["gdu"])
    check(got, b["xh"], 2e-4, f"H zbar {case} R={R}")


@pytest.mark.parametrize("case,R", RUNS, ids=RUN_IDS)
def test_parameter_gradients_do_not_move(pkg, dev, case, R):
    """The same backward's parameter gradients equal, bit for bit, those of the
    call whose X does not require grad, and those equal solver.net_u_vjp."""
    b = bundle(pkg, dev, case, R)
    m = b["m"]
    m.model.zero_grad(set_to_none=True)
    native_xbar(m, dev, b["t"], b["X"], b["gu"], b["gdu"])
    g_with = flat_param_grad(m).clone()
    m.model.zero_grad(set_to_none=True)
    u, du = m.net_u(b["t"], b["X"])
    ((torch.from_numpy(b["gu"]).to(dev) * u).sum() + (torch.from_numpy(b["gdu"]).to(dev) * du).sum()).backward()
    g_without = flat_param_grad(m).clone()
    m.model.zero_grad(set_to_none=True)
    assert float(g_without.abs().max()) > 0
    torch.testing.assert_close(g_with, g_without, rtol=0, atol=0)
    g = torch.empty_like(m.params)
    m.solver.net_u_vjp(m.params, torch.from_numpy(b["t"]).to(dev).reshape(-1), torch.from_numpy(b["X"]).to(dev),
                       torch.from_numpy(b["gu"]).to(dev).reshape(-1), torch.from_numpy(b["gdu"]).to(dev), g)
    torch.cuda.synchronize()
    used = m.solver.used_mask.to(dev)
    torch.testing.assert_close(g_without[used], g[used], rtol=0, atol=0)
    # and the input cotangent is repeatable bit for bit (fixed summation order)
    x1 = native_xbar(m, dev, b["t"], b["X"], b["gu"], b["gdu"])
    x2 = native_xbar(m, dev, b["t"], b["X"], b["gu"], b["gdu"])
    m.model.zero_grad(set_to_none=True)
    assert np.array_equal(x1, x2)


@pytest.mark.parametrize("case,R", RUNS, ids=RUN_IDS)
def test_only_xbar(pkg, dev, case, R):
    """No parameter requires grad: X.grad still matches, no parameter gets one."""
    b = bundle(pkg, dev, case, R)
    m = b["m"]
    m.model.zero_grad(set_to_none=True)
    prm = [p for _, p in m.model.named_parameters()]
    for p in prm:
        p.requires_grad_(False)
    try:
        got = native_xbar(m, dev, b["t"], b["X"], b["gu"], b["gdu"])
        assert all(p.grad is None for p in prm)
    finally:
        for p in prm:
            p.requires_grad_(True)
    check(got, b["xb"], 2e-4, f"xbar alone {case} R={R}")


@pytest.mark.parametrize("case", ["nais110_x3", "naisnet16"])
def test_xbar_behind_the_fp32_input_phase_kernels(pkg, dev, case):
    """A context created under DBSDE_X3=0 DBSDE_TNW_X3=0 (phase kernels in the
    fp32-input MFMA form) runs the same input-cotangent kernel."""
    b = bundle(pkg, dev, case, 70)
    m = make_model(pkg, dev, case, FP32_ENV)
    assert torch.equal(m.params, b["m"].params)
    check(native_xbar(m, dev, b["t"], b["X"], b["gu"], b["gdu"]), b["xb"], 2e-4, f"xbar fp32 form {case}")
    check(native_xbar(m, dev, b["t"], b["X"], None, b["gdu"]), b["xh"], 2e-4, f"H zbar fp32 form {case}")


@pytest.mark.parametrize("mode,layers,act,R", [("Naisnet", [9] + 4 * [16] + [1], "Tanh", 6),
                                               ("NAIS-Net", [101] + 4 * [110] + [1], "Sine", 4)],
                         ids=["naisnet16_d8", "nais110"])
def test_reference_jacobian_call(pkg, dev, mode, layers, act, R):
    """StabilityCheck.calculate_jacobian / calculate_spectral_radius
    (with_corr_high_dimension_pde.py:856-877, 965-985), the call as written."""
    D = layers[0] - 1
    torch.manual_seed(0)
    m = pkg.BlackScholesBarenblatt(np.ones((1, D)), 1.0, 8, 5, D, layers, mode, act, device=dev)
    oracle = ref.build_model(mode, layers, act)
    ref.set_flat_params(oracle, m.params.cpu().numpy())
    t, X, _, _ = points(R, D)
    S = torch.from_numpy(X).to(dev)
    tt = torch.from_numpy(t).to(dev)
    J = torch.autograd.functional.jacobian(lambda s: m.net_u(tt, s)[0], S).cpu()
    to = torch.from_numpy(t)
    Jr = torch.autograd.functional.jacobian(lambda s: ref.net_u(oracle, to, s)[0], torch.from_numpy(X))
    assert J.shape == Jr.shape == (R, 1, R, D)
    check(J.numpy(), Jr.numpy(), 1e-4, f"jacobian {mode}")
    for r in range(R):
        for q in range(R):
            if r != q:
                assert torch.all(J[r, 0, q] == 0), (r, q)
        assert float(J[r, 0, r].abs().max()) > 0, r
    s_nat = float(torch.linalg.svdvals(J.reshape(R, -1)).max())
    s_ref = float(torch.linalg.svdvals(Jr.reshape(R, -1)).max())
    print(f"spectral norm {s_nat:.7g} vs oracle {s_ref:.7g}")
    np.testing.assert_allclose(s_nat, s_ref, rtol=1e-4)


HESTON_SEED = 42


def heston_setup(pkg, dev):
    """The set-up of test_heston_net_u_backward_through_the_clamp
    (tests/test_gpu_round4.py) at k = 1, R = 48: the output bias is moved to
    the median raw output, so about half of the rows clamp.  The weights are
    drawn on the CPU (the oracle's initialiser) so that the seed alone fixes
    them; HESTON_SEED keeps every raw output more than 1e-4 away from zero."""
    k, layers, act, R = 1, [2] + 4 * [16] + [1], "Tanh", 48
    torch.manual_seed(HESTON_SEED)
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


def test_heston_greeks_k1(pkg, dev):
    """heston_dnnpde.py:685-699 against the oracle's heston_net_u and its
    double autograd, through the u clamp."""
    m, oracle, t, X, clamped, _ = heston_setup(pkg, dev)
    Y, delta, gamma = m.calculate_greeks(X[:, 0], X[:, 1], t[:, 0])
    R = X.shape[0]
    assert Y.shape == (R, 1) and delta.shape == (R, 1) and gamma.shape == (R,)
    Xr = torch.from_numpy(X).requires_grad_(True)
    ur, dur = ref.heston_net_u(oracle, torch.from_numpy(t), Xr)
    gr = torch.autograd.grad(dur[:, :1], Xr, torch.ones_like(dur[:, :1]))[0][:, 0].numpy()
    ur, dur = ur.detach().numpy(), dur.detach().numpy()
    assert np.array_equal(ur.ravel() == 0, clamped)
    np.testing.assert_allclose(Y, ur, rtol=0, atol=1e-4 * max(1.0, float(np.abs(ur).max())))
    np.testing.assert_allclose(delta, dur[:, :1], rtol=0, atol=1e-4 * max(1.0, float(np.abs(dur[:, :1]).max())))
    check(gamma, gr, 2e-4, "gamma")
    assert np.all(gamma[clamped] == 0.0)
    assert np.all(gr[clamped] == 0.0) and float(np.abs(gamma[~clamped]).max()) > 0


def test_heston_xbar_through_the_clamp(pkg, dev):
    m, oracle, t, X, clamped, rs = heston_setup(pkg, dev)
    R, D = X.shape
    gu = rs.normal(size=(R, 1)).astype(np.float32)
    gdu = rs.normal(size=(R, D)).astype(np.float32)
    xb, xh, _, _ = oracle_xbar(ref.heston_net_u, oracle, t, X, gu, gdu)
    got = native_xbar(m, dev, t, X, gu, gdu)
    check(got, xb, 2e-4, "heston xbar")
    assert np.all(got[clamped] == 0.0)
    check(native_xbar(m, dev, t, X, None, gdu), xh, 2e-4, "heston H zbar")


def test_third_order_raises(pkg, dev):
    """A derivative of xbar itself is out of scope: it raises, never zeros."""
    b = bundle(pkg, dev, "naisnet16", 70)
    Xg = torch.from_numpy(b["X"]).to(dev).requires_grad_(True)
    u, du = b["m"].net_u(b["t"], Xg)
    xb = torch.autograd.grad(du.sum(), Xg, create_graph=True)[0]
    with pytest.raises(RuntimeError):
        torch.autograd.grad(xb.sum(), Xg)
