"""dbsde_loss_grad, the K != 3 chunk pipeline and the net_u family at every
supported depth and at unequal FC widths, against the fp64 oracle.  Needs an
MI355X.

Cases, seeds, bounds and what each case selects in the engine:
tests/depth_cases.py (its reference side runs on the CPU in
tests/test_depth_reference_cpu.py).  Every variant of a case is compared with
the oracle, never with another variant:

  default    the environment's defaults
  fused0     DBSDE_FUSED=0 where the default is fused: the per-layer chain
  tnw0       DBSDE_TNW=0 where the wave-owned weight-gradient tiles apply: the
             split-K TN GEMM (P = 4 and P = 12 layouts through the slab finalize)
  x3off      DBSDE_X3=0 DBSDE_TNW_X3=0 where matrix_form != 0: fp32-input MFMA

Each run asserts NativeSolver.matrix_form; from a profiled repeat that must
equal the first run bit for bit, whether `fused_fwd_inputgrad` ran; and from
one profiled dbsde_train_step, whose gradient must equal them too, whether the
wave-owned weight-gradient tiles are the context's layout (the update then
rides in `grad_finalize_update`).

Measured on an MI355X when these tests were written, default variant: the
observed path (matrix_form; fused phase kernels or per-layer chain; wave-owned
tiles or split-K weight gradient) and each quantity's max error as a fraction
of its bound (tensor: the worst parameter tensor against its own maximum).

  case              form path  wgrad    loss      Y        Z        grad     tensor
  nais16_K1          0   fused tnw      6.84e-05  0.00266  0.00228  0.000428 0.00114
  fc16_K1            2   fused split-K  0.000331  0.00185  0.000944 0.00049  0.000895
  resnet16_K1        2   fused split-K  0.00067   0.00299  0.00135  0.000596 0.00093
  nais16_K2          0   fused split-K  0.000608  0.00243  0.00253  0.000742 0.00158
  fc16_K2            2   fused split-K  0.000655  0.00168  0.000888 0.000374 0.000737
  resnet16_K2        2   fused split-K  0.000511  0.00164  0.00275  0.00036  0.000952
  nais16_K3          0   fused tnw      0.000151  0.0014   0.00348  0.00119  0.00124
  fc16_K3            2   fused split-K  0.000473  0.00151  0.00113  0.000313 0.000628
  resnet16_K3        2   fused split-K  0.000191  0.003    0.00317  0.000772 0.00117
  nais16_K4          0   chain split-K  0.000233  0.00402  0.0037   0.00069  0.00201
  fc16_K4            6   chain split-K  4.32e-05  0.00238  0.00159  0.000437 0.000934
  resnet16_K4        6   chain split-K  0.000926  0.00422  0.00427  0.000876 0.00245
  nais16_K5          0   chain tnw      0.00027   0.00399  0.003    0.000583 0.00254
  fc16_K5            6   chain split-K  0.00016   0.00217  0.00148  0.000508 0.000731
  resnet16_K5        6   chain split-K  0.000595  0.00679  0.00593  0.00115  0.00159
  nais16_K6          0   chain split-K  0.000103  0.00432  0.00319  0.000936 0.00153
  fc16_K6            6   chain split-K  7.35e-05  0.00115  0.000654 0.000581 0.000744
  resnet16_K6        6   chain split-K  0.000367  0.00401  0.006    0.000536 0.00143
  nais110_K1         0   chain tnw      1.11e-05  0.00439  0.00219  0.000627 0.00157
  nais110_K2         0   chain split-K  0.000237  0.003    0.0042   0.000747 0.00152
  nais110_K5         0   chain tnw      7.56e-06  0.004    0.00558  0.000581 0.00229
  nais110_K6         0   chain split-K  0.000498  0.00501  0.00541  0.00102  0.00309
  naisnet110_K1      0   chain tnw      0.00189   0.00567  0.0021   0.00318  0.00394
  naisnet110_K2      0   chain split-K  0.00167   0.00406  0.00231  0.00293  0.00413
  fc256_K1           6   chain split-K  0.000539  0.00339  0.0012   0.000844 0.00219
  fc256_K2           6   chain split-K  0.000891  0.00361  0.00126  0.000945 0.00201
  fc256_K4           6   chain split-K  0.00133   0.00522  0.00115  0.00118  0.00256
  fc256_K6           6   chain split-K  0.00152   0.005    0.000974 0.00103  0.00302
  fc_48_32_16        0   chain split-K  0.00078   0.00163  0.00105  0.000311 0.000723
  fc_16_64_32_48     0   chain split-K  0.000691  0.00308  0.0011   0.000876 0.00127
  fc_33_20_130_7     0   chain split-K  0.000251  0.00326  0.00119  0.000379 0.000813
  fc_16_to_112       0   chain split-K  0.000147  0.00643  0.00197  0.00113  0.00196
  fc_d200_64_32_16   0   chain split-K  0.000528  0.00619  0.00201  0.000956 0.00156

What these tests notice, checked once on a temporary build at nais16 and
nais110, K = 5: an entry of launch_tnw's order[] replaced by its neighbour (one
problem never computed) and one dropped finalize window of a block problem
p = K + j each fail the default loss-and-gradient case of both networks and
the xvjp gradient of nais110_K5.  Swapping two entries of order[] is no
defect: the kernel addresses operands and output by the problem index it
reads there, so any permutation computes the same bits, and every test passes.
"""
import copy
import os

import numpy as np
import pytest
import torch

import depth_cases as dc
import jet_reference as jr
from conftest import load_pkg
from oracle import fbsnn_ref as fr

pytestmark = pytest.mark.gpu

ENV_KEYS = ("DBSDE_FUSED", "DBSDE_TNW", "DBSDE_X3", "DBSDE_TNW_X3", "DBSDE_CS", "DBSDE_CHUNKS", "DBSDE_W256",
            "DBSDE_TNW_ORDER")
VARIANT_ENV = {
    "default": {},
    "fused0": {"DBSDE_FUSED": "0"},
    "tnw0": {"DBSDE_TNW": "0"},
    "x3off": {"DBSDE_X3": "0", "DBSDE_TNW_X3": "0"},
}


def variants_of(case):
    c = dc.CASES[case]
    return ["default"] + (["fused0"] if c["fused"] else []) + (["tnw0"] if c["tnw"] else []) + \
        (["x3off"] if c["form"] else [])


def expected(case, variant):
    """(matrix_form, fused, tnw) of a variant, from the case's default
    columns: without the fused kernels a tn_x3 layout runs chainx3 (bit 2);
    without the split-bf16 forms nothing is left of matrix_form; the NAIS
    layouts' form is 0 with either weight-gradient kernel."""
    c = dc.CASES[case]
    form, fused, tnw = c["form"], c["fused"], c["tnw"]
    if variant == "fused0":
        return (form | 4 if form & 2 else form), False, tnw
    if variant == "x3off":
        return 0, fused, tnw
    if variant == "tnw0":
        return form, fused, False
    return form, fused, tnw


RUNS = [(case, v) for case in dc.CASES for v in variants_of(case)]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def make_solver(pkg, dev, case, env=None):
    """The case's NativeSolver; env holds while the context is created, with
    every other path switch of the engine unset."""
    c = dc.CASES[case]
    old = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env or {})
    try:
        return pkg.NativeSolver(c["mode"], c["layers"], c["act"], dc.spec_for(pkg, c["problem"], dc.state_dim(case)),
                                dc.T, dev)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def loss_grad(s, dev, b, D, seed=None):
    """One loss_grad into NaN-filled outputs: parity mode on the bundle's t, W,
    or device mode (seed)."""
    M, N = b["M"], b["N"]
    params = torch.from_numpy(b["params"]).to(dev)
    nan = lambda n: torch.full((n,), float("nan"), device=dev)
    out = dict(loss=nan(1), X=nan(M * (N + 1) * D), Y=nan(M * (N + 1)), Z=nan(M * (N + 1) * D))
    grad = torch.full_like(params, float("nan"))
    Xi = torch.from_numpy(b["Xi"]).to(dev).contiguous()
    if seed is None:
        s.loss_grad(params, M, N, Xi, t=torch.from_numpy(b["t"]).to(dev).reshape(M, N + 1).contiguous(),
                    W=torch.from_numpy(b["W"]).to(dev).contiguous(), grad=grad, **out)
    else:
        s.loss_grad(params, M, N, Xi, seed=seed, grad=grad, **out)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    r["X"] = r["X"].reshape(M, N + 1, D)
    r["Z"] = r["Z"].reshape(M, N + 1, D)
    r["Y"] = r["Y"].reshape(M, N + 1, 1)
    r["grad"] = grad.cpu().numpy()
    return r


def profiled(s, dev, b, D, seed=None):
    """The same call with the profiler on: (results, names of what ran)."""
    s.profile(True)
    s.profile_reset()
    r = loss_grad(s, dev, b, D, seed)
    names = set(s.profile_read())
    s.profile(False)
    return r, names


def train_step_probe(s, dev, b):
    """One profiled dbsde_train_step (Adam, device step counter, no clip) on
    copies of the parameters: (its gradient, names of what ran).  The update
    rides in the gradient finalize (`grad_finalize_update`) exactly where the
    context runs the wave-owned weight-gradient tiles (csrc/step.hip
    dbsde_train_step), which is how a test can see that choice."""
    M, N = b["M"], b["N"]
    p = torch.from_numpy(b["params"]).to(dev).clone()
    g = torch.full_like(p, float("nan"))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    state = torch.zeros(2, dtype=torch.float64, device=dev)
    s.profile(True)
    s.profile_reset()
    s.train_step(p, M, N, torch.from_numpy(b["Xi"]).to(dev).contiguous(), g, m, v,
                 dict(kind="Adam", lr=1e-3, step=1, step_state=state, step_parity=0),
                 t=torch.from_numpy(b["t"]).to(dev).reshape(M, N + 1).contiguous(),
                 W=torch.from_numpy(b["W"]).to(dev).contiguous())
    torch.cuda.synchronize()
    names = set(s.profile_read())
    s.profile(False)
    assert torch.isfinite(p).all() and float((p.cpu() - torch.from_numpy(b["params"])).abs().max()) > 0
    return g.cpu().numpy(), names


# ------------------------------------------------------------------ 1. loss and gradient at every depth
@pytest.mark.parametrize("case,variant", RUNS, ids=[f"{c}-{v}" for c, v in RUNS])
def test_loss_grad_matches_fp64_oracle(pkg, dev, case, variant):
    b = dc.reference(case)
    D = dc.state_dim(case)
    s = make_solver(pkg, dev, case, VARIANT_ENV[variant])
    r = loss_grad(s, dev, b, D)
    rp, names = profiled(s, dev, b, D)
    fused = "fused_fwd_inputgrad" in names
    gt, tnames = train_step_probe(s, dev, b)
    tnw = "grad_finalize_update" in tnames
    print(f"{case} {variant}: matrix_form {s.matrix_form}, {'fused' if fused else 'chain'}, "
          f"{'wave-owned tiles' if tnw else 'split-K'} ({sorted(names)})")
    dc.check(r, b, f"{case} {variant}")
    want_form, want_fused, want_tnw = expected(case, variant)
    assert s.matrix_form == want_form, (case, variant, s.matrix_form, want_form)
    assert fused == want_fused, (case, variant, sorted(names))
    assert tnw == want_tnw and ("optimizer" in tnames) == (not want_tnw), (case, variant, sorted(tnames))
    assert "tn_weight_grad" in names and "grad_finalize" in names, sorted(names)
    for k in ("loss", "X", "Y", "Z", "grad"):       # fixed summation orders: the repeat is bitwise equal
        np.testing.assert_array_equal(r[k], rp[k], err_msg=k)
    np.testing.assert_array_equal(gt, r["grad"], err_msg="train_step's gradient")


# ------------------------------------------------------------------ 2. the chunk pipeline at K != 3
@pytest.mark.parametrize("case", list(dc.CHUNK_CASES))
def test_two_chunk_pipeline_at_other_depths(pkg, dev, case):
    """Width 16 at K = 1 (NAIS-Net: the wave-tile weight gradient's slices per
    chunk, tnw_piped) and K = 2 (FC: the split-bf16 row splits per chunk,
    tn_piped) with M = 128, N = 3: two chunks of one 64-path unit each, 512
    rows, the chunk boundary at row 256.  A context created under
    DBSDE_CHUNKS=2 against one created without it (a single launch of each
    phase at this size), in device mode: loss rel 1e-5, gradient abs 1e-5
    max|grad|, X bit for bit; and its parity-mode run against the oracle with
    the bounds of every other case here.  A profiled repeat shows that the
    chunked context runs the pipelined section."""
    M, N = dc.CHUNK_CASES[case]
    D = dc.state_dim(case)
    b = dc.reference(case, M, N)
    two = make_solver(pkg, dev, case, {"DBSDE_CHUNKS": "2"})
    one = make_solver(pkg, dev, case)
    r2, r1 = loss_grad(two, dev, b, D, seed=5), loss_grad(one, dev, b, D, seed=5)
    top = float(np.abs(r1["grad"]).max())
    print(f"{case}: two chunks vs one, loss rel {abs(r2['loss'][0] - r1['loss'][0]) / abs(r1['loss'][0]):.3e}, "
          f"grad {np.abs(r2['grad'] - r1['grad']).max() / top:.3e} max|grad|")
    for r in (r1, r2):
        assert all(np.all(np.isfinite(r[k])) for k in ("loss", "X", "Y", "Z", "grad"))
    assert top > 0
    np.testing.assert_array_equal(r2["X"], r1["X"])
    np.testing.assert_allclose(r2["loss"], r1["loss"], rtol=1e-5)
    np.testing.assert_allclose(r2["grad"], r1["grad"], rtol=0, atol=1e-5 * top)
    dc.check(loss_grad(two, dev, b, D), b, f"{case} two chunks, parity mode")
    dc.check(loss_grad(one, dev, b, D), b, f"{case} one chunk, parity mode")
    _, names2 = profiled(two, dev, b, D)
    _, names1 = profiled(one, dev, b, D)
    assert "fused_phases_pipelined" in names2 and "fused_fwd_inputgrad" not in names2, sorted(names2)
    assert "fused_fwd_inputgrad" in names1 and "fused_phases_pipelined" not in names1, sorted(names1)


# ------------------------------------------------------------------ 3. net_u, its backward and its jets
R, RJ, ND = 70, 5, 3


def check_abs(got, want, tol, what):
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print(f"{what}: max|err| = {err:.3e} = {err / scale if scale else float('nan'):.3e} max|ref| (bound {tol:.0e})")
    assert scale > 0 and np.all(np.isfinite(got)), what
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale, err_msg=what)


_B = {}


def netu_bundle(pkg, dev, case):
    """Solver, points, cotangents, directions and the oracle's autograd results
    (on the fp64 copy of the case's model) built once and shared; no test
    changes them."""
    if case not in _B:
        D = dc.state_dim(case)
        b = dc.reference(case)
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
        _B[case] = dict(s=make_solver(pkg, dev, case), D=D, params=d(b["params"]), td=d(t.reshape(-1)), Xd=d(X),
                        gud=d(gu.reshape(-1)), gdud=d(gdu), Vd=d(V), u=ur.detach().numpy(), du=dur.detach().numpy(),
                        xb=xb, g_ref=g_ref, used=used, d1=d1, d2=d2)
    return _B[case]


@pytest.mark.parametrize("case", dc.NETU_CASES)
def test_net_u_matches_oracle(pkg, dev, case):
    b = netu_bundle(pkg, dev, case)
    u, du = torch.full((R,), float("nan"), device=dev), torch.full((R, b["D"]), float("nan"), device=dev)
    b["s"].net_u(b["params"], b["td"], b["Xd"], u, du)
    torch.cuda.synchronize()
    check_abs(u.cpu().numpy().reshape(R, 1), b["u"], 1e-4, f"u {case}")
    check_abs(du.cpu().numpy(), b["du"], 1e-4, f"Du {case}")


@pytest.mark.parametrize("case", dc.NETU_CASES)
def test_net_u_xvjp_matches_oracle_autograd(pkg, dev, case):
    b = netu_bundle(pkg, dev, case)
    s, used = b["s"], b["used"]
    args = (b["params"], b["td"], b["Xd"], b["gud"], b["gdud"])
    g, xbar = torch.full_like(b["params"], float("nan")), torch.full((R, b["D"]), float("nan"), device=dev)
    s.net_u_xvjp(*args, grad=g, xbar=xbar)
    gv = torch.full_like(b["params"], float("nan"))
    s.net_u_vjp(*args, gv)
    torch.cuda.synchronize()
    check_abs(xbar.cpu().numpy(), b["xb"], 2e-4, f"xbar {case}")
    for what, got in (("xvjp", g.cpu().numpy()), ("vjp", gv.cpu().numpy())):
        assert np.all(np.isfinite(got)), what
        check_abs(got[used], b["g_ref"][used], 2e-4, f"{what} grad {case}")
        assert np.all(got[~used] == 0.0), what


@pytest.mark.parametrize("case", dc.NETU_CASES)
def test_net_u_jet_matches_oracle(pkg, dev, case):
    b = netu_bundle(pkg, dev, case)
    d1, d2 = (torch.full((RJ, ND), float("nan"), device=dev) for _ in range(2))
    b["s"].net_u_jet(b["params"], b["td"][:RJ].contiguous(), b["Xd"][:RJ].contiguous(), b["Vd"], d1=d1, d2=d2)
    torch.cuda.synchronize()
    check_abs(d1.cpu().numpy(), b["d1"], 1e-4, f"d1 {case}")
    check_abs(d2.cpu().numpy(), b["d2"], 2e-4, f"d2 {case}")
