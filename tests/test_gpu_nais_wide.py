"""NAIS-Net and Naisnet at hidden widths 128 < L <= 1024: the matrix-core
projection kernels (csrc/projw.hip: R_j = W_j^T W_j over a triangle of tiles,
one reduced norm and one reduced <Abar_j, R_j> per block, the adjoint
W_j S_j) and the per-layer chain's x-stack paths at Wp > 128.  Needs an MI355X.

Every expectation is computed here, on the CPU, from oracle/fbsnn_ref.py and
tests/jet_reference.py.  Bounds are tests/test_gpu_parity.py's: X bit-exact,
loss rel 1e-4, Y / Z abs 1e-4 max(1, |ref|max), gradient abs 2e-4 max|ref grad|,
unused parameters exactly 0 -- and, for every projected (L x L hidden) weight
block, gradient abs 2e-4 max|ref grad of that block|: those blocks' gradients
are 10-60 times smaller than the global maximum, so the global bound alone
would pass a wrong norm-derivative term.  The oracle's own fp32-vs-fp64
difference at these cases is at most 4 % of any bound (loss 1.3e-7 rel, Y / Z
7.9e-7, global gradient 1.3e-6, per block 8.1e-6).

The scales applied to the hidden weight matrices make both projection
branches (|W^T W|_F above / below 0.98) occur, per block; each case asserts
that no norm sits near the branch.  ReLU is left out (kink flips between
summation orders)."""
import numpy as np
import pytest
import torch

import jet_reference as jr
from conftest import load_pkg
from oracle import fbsnn_ref as fr

pytestmark = pytest.mark.gpu
T = 1.0


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def spec_for(pkg, problem):
    S = pkg.ProblemSpec
    return {
        "bsb": S(sig_a=0.4, phi_r=0.05, phi_c=1.0, g="sumsq"),
        "bspde_test": S(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=1.0, g="sumsq"),
        "basket": S(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=0.0, g="call_mean", strike=1.0),
    }[problem]


# case: mode, activation, problem, D, L, depth, M, N, scale per hidden block (None: unscaled)
CASES = {
    "a": ("NAIS-Net", "Sine", "bsb", 8, 144, 4, 20, 3, None),
    "b": ("NAIS-Net", "Sine", "bsb", 8, 144, 4, 20, 3, [1.0, 0.2, 1.0]),
    "c": ("NAIS-Net", "Sine", "bsb", 8, 129, 4, 20, 3, None),
    "d": ("Naisnet", "Tanh", "bspde_test", 20, 272, 4, 20, 3, [0.15, 1.0, 0.15]),
    "e": ("NAIS-Net", "Sine", "basket", 200, 528, 3, 20, 2, None),
    "f": ("NAIS-Net", "Sine", "bsb", 30, 1024, 3, 16, 2, [1.0, 0.1]),
}


def layers_of(case):
    _, _, _, D, L, depth, _, _, _ = CASES[case]
    return [D + 1] + depth * [L] + [1]


def hidden_blocks(model, L):
    """(offset, name) of every projected L x L weight in the flat vector."""
    out, off = [], 0
    for name, p in model.state_dict().items():
        if name.endswith(".weight") and "input" not in name and tuple(p.shape) == (L, L):
            out.append((off, name))
        off += p.numel()
    return out


def build(case):
    """The case's oracle model: torch.manual_seed(D + L), build_model, then the
    scales; asserts each block's |W^T W|_F is on the expected side of 0.98."""
    mode, act, _, D, L, depth, _, _, scales = CASES[case]
    torch.manual_seed(D + L)
    model = fr.build_model(mode, layers_of(case), act)
    blocks = hidden_blocks(model, L)
    assert len(blocks) == depth - 1
    sd = model.state_dict()
    with torch.no_grad():
        for k, (_, name) in enumerate(blocks):
            s = 1.0 if scales is None else scales[k]
            sd[name].mul_(s)
            w = sd[name].double()
            nrm = float(torch.norm(w.t() @ w))
            print(f"case {case} block {k}: |W^T W|_F = {nrm:.4g}")
            assert (nrm < 0.9) if s < 1.0 else (nrm > 1.1), (case, k, nrm)
    return model, blocks


_REFS = {}


def reference(case):
    """Weights, batch and the oracle's results of one case, computed once and
    shared by the tests below (none of them changes it)."""
    if case not in _REFS:
        mode, act, problem, D, L, depth, M, N, _ = CASES[case]
        model, blocks = build(case)
        params = fr.flat_params(model)
        t, W = fr.fetch_minibatch(M, N, D, T, rng=np.random.RandomState(7))
        Xi = np.ones((1, D))
        ref = fr.loss_and_grads(model, fr.make_problem(problem, D), t, W, torch.as_tensor(Xi, dtype=torch.float32), M, D)
        _REFS[case] = dict(model=model, blocks=blocks, params=params, t=t.squeeze(-1).numpy(), W=W.numpy(), Xi=Xi,
                           ref=ref)
    return _REFS[case]


def solver(pkg, dev, case):
    mode, act, problem = CASES[case][:3]
    return pkg.NativeSolver(mode, layers_of(case), act, spec_for(pkg, problem), T, dev)


def native(s, params, M, N, D, Xi, t, W, dev, want_grad=True):
    out = dict(loss=torch.empty(1, device=dev), X=torch.empty(M * (N + 1) * D, device=dev),
               Y=torch.empty(M * (N + 1), device=dev), Z=torch.empty(M * (N + 1) * D, device=dev))
    grad = torch.full_like(params, float("nan")) if want_grad else None
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


def run_case(pkg, dev, case, want_grad=True):
    _, _, _, D, _, _, M, N, _ = CASES[case]
    b = reference(case)
    return native(solver(pkg, dev, case), torch.from_numpy(b["params"]).to(dev), M, N, D, b["Xi"], b["t"], b["W"], dev,
                  want_grad)


def check(r, ref, blocks=(), L=0, heston=False):
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
        for k, (off, _) in enumerate(blocks):
            g, gr = r["grad"][off:off + L * L], ref["grad"][off:off + L * L]
            top = float(np.abs(gr).max())
            print(f"block {k}: max|err| = {np.abs(g - gr).max():.3e}, max|ref| = {top:.3e}")
            assert top > 0
            np.testing.assert_allclose(g, gr, rtol=0, atol=2e-4 * top)


# ------------------------------------------------------------------ 1. limits
@pytest.mark.parametrize("mode", ["NAIS-Net", "Naisnet"])
@pytest.mark.parametrize("L", [129, 144, 272, 1024])
def test_solver_is_created_at_wide_hidden_widths(pkg, dev, mode, L):
    s = pkg.NativeSolver(mode, [9] + 4 * [L] + [1], "Sine", spec_for(pkg, "bsb"), T, dev)
    assert s.D == 8 and s.matrix_form == 0       # the fp32-input chain


@pytest.mark.parametrize("mode", ["NAIS-Net", "Naisnet"])
def test_the_new_limit_is_reported(pkg, dev, mode):
    with pytest.raises(ValueError, match="1024"):
        pkg.NativeSolver(mode, [9] + 4 * [1025] + [1], "Sine", spec_for(pkg, "bsb"), T, dev)


def test_width_128_keeps_its_form(pkg, dev):
    """L = 128 stays on the narrow projection kernels and the fp32-input chain."""
    s = pkg.NativeSolver("NAIS-Net", [9] + 4 * [128] + [1], "Sine", spec_for(pkg, "bsb"), T, dev)
    assert s.matrix_form == 0


# ------------------------------------------------------------------ 2. loss and gradient against the oracle
@pytest.mark.parametrize("case", list(CASES))
def test_loss_grad_matches_oracle(pkg, dev, case):
    b = reference(case)
    r = run_case(pkg, dev, case)
    check(r, b["ref"], b["blocks"], CASES[case][4])
    r2 = run_case(pkg, dev, case)
    for k in ("loss", "Y", "Z", "grad"):          # fixed summation orders: a second call is bitwise equal
        np.testing.assert_array_equal(r[k], r2[k])


# ------------------------------------------------------------------ 3. forward only
@pytest.mark.parametrize("case", ["a", "e"])
def test_forward_only_loss(pkg, dev, case):
    full = run_case(pkg, dev, case)
    fwd = run_case(pkg, dev, case, want_grad=False)
    np.testing.assert_allclose(fwd["loss"][0], full["loss"][0], rtol=1e-6)
    np.testing.assert_allclose(fwd["loss"][0], reference(case)["ref"]["loss"], rtol=1e-4)


# ------------------------------------------------------------------ 4. the net_u family
R = 37


def check_abs(got, want, tol, what, scale=None):
    scale = float(np.abs(want).max()) if scale is None else scale
    err = float(np.abs(got - want).max())
    print(f"{what}: max|err| = {err:.3e} = {err / scale if scale else float('nan'):.3e} max|ref| (bound {tol:.0e})")
    assert scale > 0 and np.all(np.isfinite(got))
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale)


_B = {}


def netu_bundle(pkg, dev, case):
    """Solver, points, cotangents and the oracle's autograd results on the
    case's weights, built once and shared (none of the tests changes it)."""
    if case not in _B:
        D = CASES[case][3]
        b = reference(case)
        oracle = b["model"]
        rs = np.random.RandomState(1)
        t = rs.uniform(0.0, 1.0, (R, 1)).astype(np.float32)
        X = (1.0 + 0.3 * rs.normal(size=(R, D))).astype(np.float32)
        gu = rs.normal(size=(R, 1)).astype(np.float32)
        gdu = rs.normal(size=(R, D)).astype(np.float32)
        Xr = torch.from_numpy(X).requires_grad_(True)
        ur, dur = fr.net_u(oracle, torch.from_numpy(t), Xr)
        full = (torch.from_numpy(gu) * ur).sum() + (torch.from_numpy(gdu) * dur).sum()
        xb = torch.autograd.grad(full, Xr, retain_graph=True)[0].numpy()
        oracle.zero_grad(set_to_none=True)
        full.backward()
        g_ref, used = fr.flat_grads(oracle)
        oracle.zero_grad(set_to_none=True)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        _B[case] = dict(s=solver(pkg, dev, case), D=D, t=t, X=X, params=d(b["params"]), td=d(t.reshape(-1)), Xd=d(X),
                        gud=d(gu.reshape(-1)), gdud=d(gdu), u=ur.detach().numpy(), du=dur.detach().numpy(), xb=xb,
                        g_ref=g_ref, used=used)
    return _B[case]


@pytest.mark.parametrize("case", ["a", "d"])
def test_net_u_matches_oracle(pkg, dev, case):
    b = netu_bundle(pkg, dev, case)
    u, du = torch.empty(R, device=dev), torch.empty(R, b["D"], device=dev)
    b["s"].net_u(b["params"], b["td"], b["Xd"], u, du)
    torch.cuda.synchronize()
    check_abs(u.cpu().numpy().reshape(R, 1), b["u"], 1e-4, f"u {case}", scale=max(1.0, float(np.abs(b["u"]).max())))
    check_abs(du.cpu().numpy(), b["du"], 1e-4, f"Du {case}", scale=max(1.0, float(np.abs(b["du"]).max())))


@pytest.mark.parametrize("case", ["a", "d"])
def test_vjp_and_xvjp_match_oracle_autograd(pkg, dev, case):
    b = netu_bundle(pkg, dev, case)
    s, used = b["s"], b["used"]
    args = (b["params"], b["td"], b["Xd"], b["gud"], b["gdud"])
    scale = float(np.abs(b["g_ref"][used]).max())

    def grads_ok(g, what):
        g = g.cpu().numpy()
        check_abs(g[used], b["g_ref"][used], 2e-4, what, scale=scale)
        assert np.all(g[~used] == 0.0)

    g = torch.full_like(b["params"], float("nan"))
    s.net_u_vjp(*args, g)
    torch.cuda.synchronize()
    grads_ok(g, f"vjp grad {case}")
    x1 = torch.full((R, b["D"]), float("nan"), device=dev)
    s.net_u_xvjp(*args, xbar=x1)
    g2 = torch.full_like(b["params"], float("nan"))
    s.net_u_xvjp(*args, grad=g2)
    g3, x3 = torch.full_like(b["params"], float("nan")), torch.full((R, b["D"]), float("nan"), device=dev)
    s.net_u_xvjp(*args, grad=g3, xbar=x3)
    torch.cuda.synchronize()
    check_abs(x1.cpu().numpy(), b["xb"], 2e-4, f"xbar alone {case}")
    check_abs(x3.cpu().numpy(), b["xb"], 2e-4, f"xbar with grad {case}")
    grads_ok(g2, f"xvjp grad alone {case}")
    grads_ok(g3, f"xvjp grad with xbar {case}")
    torch.testing.assert_close(g2, g, rtol=0, atol=0)
    torch.testing.assert_close(g3, g, rtol=0, atol=0)
    torch.testing.assert_close(x3, x1, rtol=0, atol=0)      # fixed summation order: bitwise repeatable


def jet_setup(pkg, dev, L):
    """(solver, oracle, flat params): L = 144 is case a's network; other widths
    the same architecture (NAIS-Net, Sine, D = 8, depth 4) from seed D + L."""
    if L == 144:
        b = reference("a")
        return solver(pkg, dev, "a"), b["model"], b["params"]
    layers = [9] + 4 * [L] + [1]
    torch.manual_seed(8 + L)
    oracle = fr.build_model("NAIS-Net", layers, "Sine")
    return pkg.NativeSolver("NAIS-Net", layers, "Sine", spec_for(pkg, "bsb"), T, dev), oracle, fr.flat_params(oracle)


def jet_points(D):
    rs = np.random.RandomState(1)
    t = rs.uniform(0.0, 1.0, (R, 1)).astype(np.float32)
    X = (1.0 + 0.3 * rs.normal(size=(R, D))).astype(np.float32)
    V = np.random.RandomState(2).normal(size=(R, 4, D + 1)).astype(np.float32)
    V[:, 3, :] = 0.0
    V[:, 3, 0] = 1.0                     # e_t
    return t, X, V


@pytest.mark.parametrize("L", [144, 256])
def test_jets_and_pde_residual_match_oracle(pkg, dev, L):
    """tests/test_gpu_jet.py's bounds: d1 1e-4, d2 and every PDE term 2e-4
    max|ref|, the residual 2e-4 max(scale)."""
    D = 8
    s, oracle, params = jet_setup(pkg, dev, L)
    pd = torch.from_numpy(params).to(dev)
    t, X, V = jet_points(D)
    r1, r2 = jr.jets(oracle, t, X, V)
    d1, d2 = (torch.full((R, 4), float("nan"), device=dev) for _ in range(2))
    s.net_u_jet(pd, torch.from_numpy(t.reshape(-1)).to(dev), torch.from_numpy(X).to(dev), torch.from_numpy(V).to(dev),
                d1=d1, d2=d2)
    torch.cuda.synchronize()
    check_abs(d1.cpu().numpy(), r1, 1e-4, f"d1 L={L}")
    check_abs(d2.cpu().numpy(), r2, 2e-4, f"d2 L={L}")
    want = jr.pde_terms(oracle, fr.make_problem("bsb", D), t, X)
    out = {k: torch.full((R,), float("nan"), device=dev) for k in jr.TERMS}
    s.pde_residual(pd, torch.from_numpy(t.reshape(-1)).to(dev), torch.from_numpy(X).to(dev), **out)
    torch.cuda.synchronize()
    smax = float(np.abs(want["scale"]).max())
    for k in jr.TERMS:
        g = out[k].cpu().numpy().reshape(-1, 1)
        top = smax if k == "residual" else float(np.abs(want[k]).max())
        if top == 0:                     # a term the problem does not have (mu = 0): exactly zero
            assert np.all(g == 0), k
        else:
            check_abs(g, want[k], 2e-4, f"L={L} {k}", scale=top)


def test_jets_keep_their_width_limit(pkg, dev):
    """Hidden widths above 256 stay refused by the jet kernels."""
    b = netu_bundle(pkg, dev, "d")
    D = b["D"]
    V = torch.zeros(R, 1, D + 1, device=dev)
    with pytest.raises(ValueError):
        b["s"].net_u_jet(b["params"], b["td"], b["Xd"], V, d1=torch.empty(R, 1, device=dev))
    with pytest.raises(ValueError):
        b["s"].pde_residual(b["params"], b["td"], b["Xd"], residual=torch.empty(R, device=dev))


# ------------------------------------------------------------------ 5. training steps
@pytest.mark.parametrize("max_norm", [0.0, 1.0], ids=["adam", "adam_clip1"])
def test_train_step_equals_loss_grad_plus_optimizer_step(pkg, dev, max_norm):
    """These widths take dbsde_train_step's two-call form; three steps give
    bit-identical parameters, moments and step state to loss_grad +
    optimizer_step."""
    _, _, _, D, _, _, M, N, _ = CASES["a"]
    b = reference("a")
    Xi = torch.ones(D, device=dev)
    res = []
    for fused in (True, False):
        s = solver(pkg, dev, "a")
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


@pytest.mark.parametrize("case", ["a", "d"])
def test_five_adam_iterations_match_oracle(pkg, dev, case):
    """Five Adam iterations (lr 1e-3, no clipping) from the oracle's initial
    parameters on the oracle's own batches (one RandomState(7) stream, M = 32,
    N = 4): parameters within abs 5e-5, tests/test_gpu_parity.py's bound for
    ten reference iterations.  Without clipping the oracle's own fp32-vs-fp64
    parameter difference after such iterations is 7e-8 .. 2.3e-7."""
    mode, act, problem, D, L, depth, _, _, _ = CASES[case]
    M, N = 32, 4
    model, _ = build(case)
    p = torch.from_numpy(fr.flat_params(model)).to(dev)
    prob = fr.make_problem(problem, D)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    rng = np.random.RandomState(7)
    s = solver(pkg, dev, case)
    g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    Xi = torch.ones(1, D)
    Xid = torch.ones(D, device=dev)
    for it in range(5):
        t, W = fr.fetch_minibatch(M, N, D, T, rng=rng)
        opt.zero_grad()
        loss = fr.loss_function(model, prob, t, W, Xi.clone().requires_grad_(True), M, D)[0]
        loss.backward()
        opt.step()
        s.loss_grad(p, M, N, Xid, t=t.squeeze(-1).float().to(dev).contiguous(), W=W.float().to(dev).contiguous(), grad=g)
        s.optimizer_step(p, g, m, v, kind="Adam", lr=1e-3, step=it + 1)
    torch.cuda.synchronize()
    want = fr.flat_params(model)
    used = s.used_mask.numpy()
    got = p.cpu().numpy()
    print(f"case {case}: max|param err| = {np.abs(got - want)[used].max():.3e}")
    np.testing.assert_allclose(got[used], want[used], rtol=0, atol=5e-5)
    np.testing.assert_array_equal(got[~used], want[~used])


@pytest.mark.parametrize("mode,act", [("NAIS-Net", "Sine"), ("Naisnet", "Tanh")])
def test_fbsnn_surface_at_width_144(pkg, dev, mode, act):
    """An FBSNN subclass takes the wider layers as they are: its torch module
    holds views of the flat vector, loss_function + backward match the oracle
    on the same weights, the module's own forward matches net_u, and a
    device-mode step trains."""
    D, L, M, N = 8, 144, 20, 3
    layers = [D + 1] + 4 * [L] + [1]
    torch.manual_seed(5)
    m = pkg.BlackScholesBarenblatt(np.ones((1, D)), T, M, N, D, layers, mode, act, device=dev)
    m.log_print = False
    oracle = fr.build_model(mode, layers, act)
    fr.set_flat_params(oracle, m.params.cpu().numpy())
    blocks = hidden_blocks(oracle, L)
    named = dict(m.model.named_parameters())
    for off, name in blocks:
        assert tuple(named[name].shape) == (L, L)
        assert named[name].data_ptr() == m.params[off:].data_ptr()
    t, W = fr.fetch_minibatch(M, N, D, T, rng=np.random.RandomState(7))
    Xi = torch.ones(1, D)
    ref = fr.loss_and_grads(oracle, fr.make_problem("bsb", D), t, W, Xi, M, D)
    m.model.zero_grad(set_to_none=True)
    loss, X, Y, y0 = m.loss_function(t.to(dev), W.to(dev), Xi.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(loss), ref["loss"], rtol=1e-4)
    np.testing.assert_array_equal(X.cpu().numpy(), ref["X"])
    g = torch.cat([(named[n].grad if named[n].grad is not None else torch.zeros_like(named[n])).reshape(-1)
                   for n in m.model.state_dict()]).cpu().numpy()
    used = ref["used"]
    assert np.all(g[~used] == 0)
    np.testing.assert_allclose(g[used], ref["grad"][used], rtol=0, atol=2e-4 * np.abs(ref["grad"]).max())
    # the torch module's own forward (networks.py) against the native net_u
    rs = np.random.RandomState(1)
    tt = torch.from_numpy(rs.uniform(0.0, 1.0, (R, 1)).astype(np.float32)).to(dev)
    S = torch.from_numpy((1.0 + 0.3 * rs.normal(size=(R, D))).astype(np.float32)).to(dev)
    with torch.no_grad():
        u, _ = m.net_u(tt, S)
        v = m.model(torch.cat([tt, S], 1))
    check_abs(u.cpu().numpy().reshape(R, 1), v.cpu().numpy().reshape(R, 1), 1e-4, f"net_u vs module {mode}",
              scale=max(1.0, float(v.abs().max())))
    opt = m.new_optimizer_state("Adam", 1e-3)
    before = m.params.clone()
    assert np.isfinite(float(m.device_step(opt, seed=1)))
    assert torch.all(torch.isfinite(m.params)) and float((m.params - before).abs().max()) > 0


# ------------------------------------------------------------------ 6. Heston
def test_heston_naisnet_144(pkg, dev):
    """k = 2 (state 4), Naisnet, L = 144, against fr.heston_loss_and_grads with
    tests/test_gpu_wide_state.py test_heston_wide's bounds."""
    k, L, M, N = 2, 144, 16, 6
    layers = [1 + 2 * k] + 4 * [L] + [1]
    spec = pkg.ProblemSpec(kind="heston", mu_a=0.05, phi_r=0.05, g="call_mean", strike=1.0, g_alpha=10.0, g_cols=k,
                           u_clamp=True, q3=False, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8)
    s = pkg.NativeSolver("Naisnet", layers, "Sine", spec, T, dev)
    assert s.nb == k
    Xi = np.concatenate([np.ones((1, k)), np.full((1, k), 0.2)], 1)
    torch.manual_seed(2 * k + L)
    model = fr.build_heston_model("Naisnet", [2] + layers[1:], "Sine", k)
    blocks = hidden_blocks(model, L)
    assert len(blocks) == 3
    for _, name in blocks:               # no block near the projection branch
        w = model.state_dict()[name].double()
        nrm = float(torch.norm(w.t() @ w))
        assert nrm < 0.9 or nrm > 1.1, (name, nrm)
    params = fr.flat_params(model)
    t, W = fr.fetch_minibatch(M, N, k, T, rng=np.random.RandomState(7))
    ref = fr.heston_loss_and_grads(model, fr.Heston(k=k, payoff="discontinuous"), t, W, np.ones((1, k)), M)
    r = native(s, torch.from_numpy(params).to(dev), M, N, 2 * k, Xi, t.squeeze(-1), W, dev)
    check(r, ref, heston=True)
