"""SiLU and Softplus on the device: loss, Y, Z and gradient of every kernel
family against the fp64 oracle, net_u / its backward / its jets, saturated
pre-activations, the PDE residual, the Python surface, and the old activations
bit for bit against the parent commit.  Needs an MI355X.

Cases, seeds and what each layout selects: tests/act_cases.py (its reference
side runs on the CPU in tests/test_act_cpu.py).  Bounds: depth_cases.BOUNDS as
they stand.  Every variant of a case is compared with the oracle, never with
another variant:

  default    the environment's defaults (at M = 20 the width-110 K = 3 layouts
             run the column-split phase kernels: all their workgroups are
             resident at once)
  fused0     DBSDE_FUSED=0 where the default is fused: the per-layer chain
  x3off      DBSDE_X3=0 DBSDE_TNW_X3=0 where matrix_form != 0: fp32-input MFMA
  tnw0       DBSDE_TNW=0 where the wave-owned weight-gradient tiles apply
  cs1        DBSDE_CS=1 at width 110, K = 3: the column-split form, forced
  cs0        DBSDE_CS=0 there: the 64-row split-bf16 phase kernels, which the
             headline batch (M = 1024) runs

Each run asserts NativeSolver.matrix_form and, from a profiled repeat that must
equal the first run bit for bit, whether the fused phase kernels ran, against
act_cases' expectation table."""
import copy
import hashlib
import os

import numpy as np
import pytest
import torch

import act_cases as ac
import depth_cases as dc
import jet_reference as jr
from conftest import ROOT, load_pkg
from oracle import fbsnn_ref as fr

pytestmark = pytest.mark.gpu

ENV_KEYS = ("DBSDE_FUSED", "DBSDE_TNW", "DBSDE_X3", "DBSDE_TNW_X3", "DBSDE_CS", "DBSDE_CHUNKS", "DBSDE_W256",
            "DBSDE_TNW_ORDER")
VARIANT_ENV = {
    "default": {},
    "fused0": {"DBSDE_FUSED": "0"},
    "tnw0": {"DBSDE_TNW": "0"},
    "x3off": {"DBSDE_X3": "0", "DBSDE_TNW_X3": "0"},
    "cs1": {"DBSDE_CS": "1"},
    "cs0": {"DBSDE_CS": "0"},
}
GOLDEN = os.path.join(ROOT, "tests", "golden", "act_parent_bits.npz")


def variants_of(c):
    return ["default"] + (["fused0"] if c["fused"] else []) + (["tnw0"] if c["tnw"] else []) + \
        (["x3off"] if c["form"] else []) + (["cs1", "cs0"] if c["cs"] else [])


def expected(c, variant):
    """(matrix_form, fused) of a variant from the layout's default columns
    (tests/test_gpu_depths.py's rule, extended to the split-bf16 fused
    layouts).  Without the fused kernels the phase bit (0) goes; a tn_x3 layout
    then runs chainx3 (bit 2), a NAIS layout the fp32 chain and fp32
    weight-gradient tiles (0).  Without the wave-owned tiles their bit (1)
    goes.  Without the split-bf16 forms nothing is left of matrix_form, and
    width 256 has no fp32-input phase kernels: it runs the chain."""
    form, fused = c["form"], c["fused"]
    if variant == "fused0":
        return (0 if c["tnw"] else ((form & ~1) | 4 if form & 2 else form & ~1)), False
    if variant == "tnw0":
        return form & ~2, fused
    if variant == "x3off":
        return 0, fused and c["layers"][1] <= 128
    return form, fused


RUNS = [(case, v) for case, c in ac.CASES.items() for v in variants_of(c)]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def make_solver(pkg, dev, c, env=None):
    """A NativeSolver of layout c (mode, layers, act, problem); env holds while
    the context is created, with every other path switch of the engine unset."""
    old = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env or {})
    try:
        return pkg.NativeSolver(c["mode"], c["layers"], c["act"], dc.spec_for(pkg, c["problem"], c["layers"][0] - 1),
                                dc.T, dev)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def loss_grad(s, dev, b, D):
    """One parity-mode loss_grad into NaN-filled outputs."""
    M, N = b["M"], b["N"]
    params = torch.from_numpy(b["params"]).to(dev)
    nan = lambda n: torch.full((n,), float("nan"), device=dev)
    out = dict(loss=nan(1), X=nan(M * (N + 1) * D), Y=nan(M * (N + 1)), Z=nan(M * (N + 1) * D))
    grad = torch.full_like(params, float("nan"))
    s.loss_grad(params, M, N, torch.from_numpy(b["Xi"]).to(dev).contiguous(),
                t=torch.from_numpy(b["t"]).to(dev).reshape(M, N + 1).contiguous(),
                W=torch.from_numpy(b["W"]).to(dev).contiguous(), grad=grad, **out)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    r["X"] = r["X"].reshape(M, N + 1, D)
    r["Z"] = r["Z"].reshape(M, N + 1, D)
    r["Y"] = r["Y"].reshape(M, N + 1, 1)
    r["grad"] = grad.cpu().numpy()
    return r


def profiled(s, dev, b, D):
    s.profile(True)
    s.profile_reset()
    r = loss_grad(s, dev, b, D)
    names = set(s.profile_read())
    s.profile(False)
    return r, names


# ------------------------------------------------------------------ 1. loss, Y, Z and gradient
@pytest.mark.parametrize("case,variant", RUNS, ids=[f"{c}-{v}" for c, v in RUNS])
def test_loss_grad_matches_fp64_oracle(pkg, dev, case, variant):
    c = ac.CASES[case]
    b = ac.reference(case)
    D = ac.state_dim(case)
    s = make_solver(pkg, dev, c, VARIANT_ENV[variant])
    r = loss_grad(s, dev, b, D)
    rp, names = profiled(s, dev, b, D)
    fused = "fused_fwd_inputgrad" in names
    print(f"{case} {variant}: matrix_form {s.matrix_form}, {'fused' if fused else 'chain'} ({sorted(names)})")
    dc.check(r, b, f"{case} {variant}")
    want_form, want_fused = expected(c, variant)
    assert s.matrix_form == want_form, (case, variant, s.matrix_form, want_form)
    assert fused == want_fused, (case, variant, sorted(names))
    for k in ("loss", "X", "Y", "Z", "grad"):       # fixed summation orders: the repeat is bitwise equal
        np.testing.assert_array_equal(r[k], rp[k], err_msg=k)


@pytest.mark.parametrize("layout", list(ac.LAYOUTS))
def test_expectation_table_is_what_tanh_selects(pkg, dev, layout):
    """The fused / matrix_form columns of act_cases are what a Tanh solver of
    the same layout reports under every variant: each new activation has the
    fused instances tanh has."""
    c = dict(ac.LAYOUTS[layout], act="Tanh")
    b = ac.reference(f"{layout}-SiLU")         # the batch and a parameter vector of the layout
    for variant in variants_of(c):
        s = make_solver(pkg, dev, c, VARIANT_ENV[variant])
        r, names = profiled(s, dev, b, c["layers"][0] - 1)
        assert np.isfinite(r["loss"]).all()
        got = (s.matrix_form, "fused_fwd_inputgrad" in names)
        print(f"{layout} Tanh {variant}: matrix_form {got[0]}, {'fused' if got[1] else 'chain'}")
        assert got == expected(c, variant), (layout, variant, got)


# ------------------------------------------------------------------ 2. net_u, its backward and its jets
R, RJ, ND = 70, 5, 3
NETU_CASES = [f"{lay}-{act}" for lay in ac.NETU_LAYOUTS for act in ac.ACTS]
SAT_CASES = [f"{lay}-{act}" for lay in ac.SAT_LAYOUTS for act in ac.ACTS]


def check_abs(got, want, tol, what):
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print(f"{what}: max|err| = {err:.3e} = {err / scale if scale else float('nan'):.3e} max|ref| (bound {tol:.0e})")
    assert scale > 0 and np.all(np.isfinite(got)), what
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale, err_msg=what)


_B = {}


def netu_bundle(pkg, dev, case, sat=False):
    """Solver, points, cotangents, directions and the oracle's autograd results
    (on the fp64 copy of the case's model), built once and shared."""
    key = (case, sat)
    if key not in _B:
        D = ac.state_dim(case)
        b = ac.reference(case, sat)
        oracle = copy.deepcopy(b["model"]).double()
        rs = np.random.RandomState(1)
        t = rs.uniform(0.0, 1.0, (R, 1)).astype(np.float32)
        X = (1.0 + 0.3 * rs.normal(size=(R, D))).astype(np.float32)
        gu = rs.normal(size=(R, 1)).astype(np.float32)
        gdu = rs.normal(size=(R, D)).astype(np.float32)
        V = np.random.RandomState(2).normal(size=(RJ, ND, D + 1)).astype(np.float32)
        V[:, ND - 1, :] = 0.0
        V[:, ND - 1, 0] = 1.0                # e_t
        Xr = torch.from_numpy(X).double().requires_grad_(True)
        ur, dur = fr.net_u(oracle, torch.from_numpy(t).double(), Xr)
        full = (torch.from_numpy(gu).double() * ur).sum() + (torch.from_numpy(gdu).double() * dur).sum()
        xb = torch.autograd.grad(full, Xr, retain_graph=True)[0].numpy()
        oracle.zero_grad(set_to_none=True)
        full.backward()
        g_ref, used = fr.flat_grads(oracle)
        oracle.zero_grad(set_to_none=True)
        d1, d2 = jr.jets(oracle, t[:RJ].astype(np.float64), X[:RJ].astype(np.float64), V.astype(np.float64))
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        _B[key] = dict(s=make_solver(pkg, dev, ac.CASES[case]), D=D, params=d(b["params"]), td=d(t.reshape(-1)),
                       Xd=d(X), gud=d(gu.reshape(-1)), gdud=d(gdu), Vd=d(V), u=ur.detach().numpy(),
                       du=dur.detach().numpy(), xb=xb, g_ref=g_ref, used=used, d1=d1, d2=d2)
    return _B[key]


def check_net_u(b, dev, what):
    u, du = torch.full((R,), float("nan"), device=dev), torch.full((R, b["D"]), float("nan"), device=dev)
    b["s"].net_u(b["params"], b["td"], b["Xd"], u, du)
    torch.cuda.synchronize()
    check_abs(u.cpu().numpy().reshape(R, 1), b["u"], 1e-4, f"u {what}")
    check_abs(du.cpu().numpy(), b["du"], 1e-4, f"Du {what}")


def check_xvjp(b, dev, what):
    s, used = b["s"], b["used"]
    args = (b["params"], b["td"], b["Xd"], b["gud"], b["gdud"])
    g, xbar = torch.full_like(b["params"], float("nan")), torch.full((R, b["D"]), float("nan"), device=dev)
    s.net_u_xvjp(*args, grad=g, xbar=xbar)
    gv = torch.full_like(b["params"], float("nan"))
    s.net_u_vjp(*args, gv)
    torch.cuda.synchronize()
    check_abs(xbar.cpu().numpy(), b["xb"], 2e-4, f"xbar {what}")
    for name, got in (("xvjp", g.cpu().numpy()), ("vjp", gv.cpu().numpy())):
        assert np.all(np.isfinite(got)), name
        check_abs(got[used], b["g_ref"][used], 2e-4, f"{name} grad {what}")
        assert np.all(got[~used] == 0.0), name


def check_jets(b, dev, what):
    d1, d2 = (torch.full((RJ, ND), float("nan"), device=dev) for _ in range(2))
    b["s"].net_u_jet(b["params"], b["td"][:RJ].contiguous(), b["Xd"][:RJ].contiguous(), b["Vd"], d1=d1, d2=d2)
    torch.cuda.synchronize()
    check_abs(d1.cpu().numpy(), b["d1"], 1e-4, f"d1 {what}")
    check_abs(d2.cpu().numpy(), b["d2"], 2e-4, f"d2 {what}")


@pytest.mark.parametrize("case", NETU_CASES)
def test_net_u_matches_oracle(pkg, dev, case):
    check_net_u(netu_bundle(pkg, dev, case), dev, case)


@pytest.mark.parametrize("case", NETU_CASES)
def test_net_u_xvjp_matches_oracle_autograd(pkg, dev, case):
    check_xvjp(netu_bundle(pkg, dev, case), dev, case)


@pytest.mark.parametrize("case", NETU_CASES)
def test_net_u_jet_matches_oracle(pkg, dev, case):
    check_jets(netu_bundle(pkg, dev, case), dev, case)


# ------------------------------------------------------------------ 3. saturation
@pytest.mark.parametrize("case", SAT_CASES)
def test_saturated_preactivations(pkg, dev, case):
    """The input layer's weight scaled so that the first pre-activation spans
    beyond +-60 (asserted here on the oracle, on the CPU): loss, Z, gradient and
    jets finite and within the same bounds, on the fused kernels (default, and
    the 64-row and fp32-input forms where the layout has them) and on the
    chain.  An exp(+|a|) form or a 1 - s cancellation shows up here."""
    c = ac.CASES[case]
    b = ac.reference(case, sat=True)
    a0 = ac.first_preactivation(b["model"], b["tt"], b["Wt"], b["Xit"], case)
    print(f"{case}: a_0 spans [{a0.min():.1f}, {a0.max():.1f}]")
    assert a0.min() <= -ac.SAT_SPAN and a0.max() >= ac.SAT_SPAN
    D = ac.state_dim(case)
    for variant in variants_of(c):
        if variant == "tnw0":
            continue
        r = loss_grad(make_solver(pkg, dev, c, VARIANT_ENV[variant]), dev, b, D)
        dc.check(r, b, f"{case} saturated {variant}")
    nb = netu_bundle(pkg, dev, case, sat=True)
    check_net_u(nb, dev, f"{case} saturated")
    check_jets(nb, dev, f"{case} saturated")


# ------------------------------------------------------------------ 4. the PDE residual
def check_terms(got, want, what):
    """tests/test_gpu_jet.py's rule: every term within 2e-4 max|term|, the
    residual within 2e-4 max(scale)."""
    assert set(got) == set(jr.TERMS)
    smax = float(np.abs(want["scale"]).max())
    for k in jr.TERMS:
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape, (k, g.shape)
        top = smax if k == "residual" else float(np.abs(want[k]).max())
        if top == 0:
            assert np.all(g == 0), k
        else:
            err = float(np.abs(g - want[k]).max())
            print(f"{what} {k}: max|err| = {err:.3e} = {err / top:.3e} of its scale (bound 2e-04)")
            assert np.all(np.isfinite(g)), k
            np.testing.assert_allclose(g, want[k], rtol=0, atol=2e-4 * top, err_msg=k)


def swapped_oracle(m, mode, layers, act, dtype=torch.float64):
    """The oracle model (built with Tanh, activation swapped) on the weights of
    the package object m."""
    oracle = ac.swap_activation(fr.build_model(mode, layers, "Tanh"), act).to(dtype)
    fr.set_flat_params(oracle, m.params.cpu().numpy())
    return oracle


@pytest.mark.parametrize("act", ac.ACTS)
def test_pde_residual_of_a_bsb_object(pkg, dev, act):
    D, mode, layers, Rp = 100, "NAIS-Net", ac.W110, 64
    torch.manual_seed(0)
    np.random.seed(0)
    m = pkg.BlackScholesBarenblatt(np.ones((1, D)), 1.0, 8, 5, D, layers, mode, act, device=dev)
    assert m.native_coefficients
    oracle = swapped_oracle(m, mode, layers, act)
    rs = np.random.RandomState(1)
    t = rs.uniform(0.0, 1.0, (Rp, 1)).astype(np.float32)
    X = (1.0 + 0.3 * rs.normal(size=(Rp, D))).astype(np.float32)
    want = jr.pde_terms(oracle, fr.make_problem("bsb", D), t.astype(np.float64), X.astype(np.float64), L=m._L)
    got = m.pde_residual(t, X)
    torch.cuda.synchronize()
    check_terms(got, want, f"bsb {act}")
    th = m.theta(t, X)
    check_abs(th.cpu().numpy(), jr.theta(oracle, t.astype(np.float64), X.astype(np.float64)), 1e-4, f"theta {act}")


# ------------------------------------------------------------------ 5. the Python surface
def _surface(pkg, dev, kind):
    torch.manual_seed(1)
    np.random.seed(1)
    if kind == "fbsnn":
        D = 8
        m = pkg.BlackScholesBarenblatt(np.ones((1, D)), 1.0, 16, 4, D, [D + 1] + 4 * [16] + [1], "NAIS-Net", "SiLU",
                                       device=dev)
        X = 1.0 + 0.2 * np.random.RandomState(3).normal(size=(9, D))
    else:
        m = pkg.HestonTwoFactorFBSNN(np.ones((1, 1)), 1.0, 16, 4, 1, None, [2] + 4 * [16] + [1], "Naisnet", "SiLU",
                                     device=dev)
        X = np.stack([np.linspace(0.8, 1.2, 9), np.full(9, 0.2)], 1)
        # the Heston init (zero biases, gain 0.5) leaves the network negative at these points and
        # u = max(net, 0) identically 0: lift the output bias so that the clamp is open
        list(m.model.parameters())[-1].data.fill_(0.5)
    return m, np.linspace(0.0, 0.8, 9).astype(np.float32), X.astype(np.float32)


@pytest.mark.parametrize("kind", ["fbsnn", "heston2"])
def test_python_surface(pkg, dev, kind, tmp_path):
    m, t, X = _surface(pkg, dev, kind)
    assert m.activation == "SiLU" and any(isinstance(x, torch.nn.SiLU) for x in m.model.modules())

    def torch_net_u():
        Xt = torch.from_numpy(X).to(dev).requires_grad_(True)
        u = m.model(torch.cat((torch.from_numpy(t).to(dev).reshape(-1, 1), Xt), 1))
        if kind == "heston2":
            u = torch.clamp(u, min=0.0)       # heston_dnnpde.py:568
        du, = torch.autograd.grad(u.sum(), Xt)
        return u.detach().cpu().numpy(), du.cpu().numpy()

    def compare(what):
        with torch.no_grad():
            u, du = m.net_u(t, X)
        torch.cuda.synchronize()
        wu, wdu = torch_net_u()
        assert (wu > 0).any()
        check_abs(u.cpu().numpy(), wu, 1e-4, f"{kind} u {what}")
        check_abs(du.cpu().numpy(), wdu, 1e-4, f"{kind} Du {what}")

    compare("at init")
    # autograd through net_u into the parameters and X against the torch model's own
    Xg = torch.from_numpy(X).to(dev).requires_grad_(True)
    m.model.zero_grad(set_to_none=True)
    u, du = m.net_u(t, Xg)
    (u.sum() + (du * du).sum()).backward()
    grads = lambda: {n: None if p.grad is None else p.grad.detach().clone().reshape(-1).cpu().numpy()
                     for n, p in m.model.named_parameters()}
    got_p, got_x = grads(), Xg.grad.cpu().numpy()
    m.model.zero_grad(set_to_none=True)
    Xr = torch.from_numpy(X).to(dev).requires_grad_(True)
    ur = m.model(torch.cat((torch.from_numpy(t).to(dev).reshape(-1, 1), Xr), 1))
    if kind == "heston2":
        ur = torch.clamp(ur, min=0.0)
    dur, = torch.autograd.grad(ur.sum(), Xr, create_graph=True)
    (ur.sum() + (dur * dur).sum()).backward()
    want_p = grads()
    m.model.zero_grad(set_to_none=True)
    used = [n for n, g in want_p.items() if g is not None]
    assert used and all(got_p[n] is None or not got_p[n].any() for n in want_p if n not in used)
    check_abs(np.concatenate([got_p[n] for n in used]), np.concatenate([want_p[n] for n in used]), 2e-4,
              f"{kind} parameter gradient through net_u")
    check_abs(got_x, Xr.grad.cpu().numpy(), 2e-4, f"{kind} X gradient through net_u")

    before = m.params.clone()
    m.train_device(3, 1e-3, seed=2)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(m.params).all()) and float((m.params - before).abs().max()) > 0
    compare("after three device steps")
    path = str(tmp_path / "model.pt")
    m.save_model(path)
    trained = m.params.clone()
    m2, _, _ = _surface(pkg, dev, kind)
    assert not torch.equal(m2.params, trained)
    m2.load_model(path)
    assert torch.equal(m2.params, trained) and m2.iteration == m.iteration
    with torch.no_grad():
        a, b = m.net_u(t, X), m2.net_u(t, X)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------ 6. the old activations are untouched
OLD_VARIANTS = ("default", "cs0", "x3off", "fused0")


def old_bundle(act):
    """nais110_K3 with one of the reference's activations: depth_cases' seed
    and batch, the oracle's own model."""
    lay = ac.LAYOUTS["nais110_K3"]
    torch.manual_seed(100 + len(lay["layers"]))
    model = fr.build_model(lay["mode"], lay["layers"], act)
    t, W, Xi = ac.batch("nais110_K3-SiLU")
    return dict(params=fr.flat_params(model), M=lay["M"], N=lay["N"], t=t.squeeze(-1).numpy(), W=W.numpy(),
                Xi=Xi.numpy())


def old_bits(pkg, dev, act, variant):
    """(loss bits, gradient sha256, 256 evenly spaced gradient elements' bits)."""
    c = dict(ac.LAYOUTS["nais110_K3"], act=act)
    r = loss_grad(make_solver(pkg, dev, c, VARIANT_ENV[variant]), dev, old_bundle(act), 100)
    g = np.ascontiguousarray(r["grad"], np.float32)
    assert np.isfinite(g).all() and np.isfinite(r["loss"]).all()
    digest = np.frombuffer(hashlib.sha256(g.tobytes()).digest(), np.uint8)
    return r["loss"].astype(np.float32).view(np.uint32), digest, g[::max(1, g.size // 256)][:256].view(np.uint32)


@pytest.mark.parametrize("variant", OLD_VARIANTS)
@pytest.mark.parametrize("act", ["Sine", "Tanh"])
def test_old_activations_keep_their_bits(pkg, dev, act, variant):
    """Loss and gradient of nais110_K3 with Sine and with Tanh, bit for bit
    what the parent commit's library gave on an MI355X
    (tests/golden/act_parent_bits.npz: loss bits, the gradient's sha256 and 256
    of its elements, recorded by running this function on the parent build)."""
    gold = np.load(GOLDEN)
    loss, digest, sample = old_bits(pkg, dev, act, variant)
    key = f"{act}-{variant}"
    np.testing.assert_array_equal(loss, gold[key + "-loss"], err_msg="loss bits")
    np.testing.assert_array_equal(sample, gold[key + "-sample"], err_msg="gradient sample bits")
    np.testing.assert_array_equal(digest, gold[key + "-sha256"], err_msg="gradient sha256")
