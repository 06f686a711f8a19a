"""The optimizer and L-BFGS device kernels against torch beyond the defaults
(DESIGN row a8): optim_kernel / opt_apply / opt_step_scalars / make_optargs and
the fused update of tilefin_kernel and proj_backward_kernel (csrc/kernels.hpp,
csrc/step.hip), vec_reduce / vec_axpby / lbfgs_direction (csrc/vec.hpp).
Needs an MI355X.

Every comparison of an optimizer update or an L-BFGS direction uses one rule
(tests/optim_reference.py tolerance): with x64 the float64 truth and x32 the
working-precision reference (torch fp32; the numpy mirror for the direction),
e32 = max|x32 - x64| and the device must satisfy max|x_dev - x64| <= 8 e32
(floor 2^-24 max|x64| when e32 == 0).  The margin is over the reference's own
rounding error: the kernels round every product and sum on its own where
torch's CPU kernels fuse some (lerp, addcmul).  The vector reductions and axpby
have derived bounds, stated at their tests.

Measured on an MI355X: the largest max|x_dev - x64| / e32 over every case of
this file (each comparison prints its own as a RATIO line under pytest -s).
1.00 means the device result equals torch's fp32 result bit for bit wherever
the error is largest.

  single update (a: both option sets, t = 1 .. 1,000,007, device and host
  step count, contexts S and L) / 25-step trajectory (b)

  kind       params        m             v
  Adam       1.00 / 1.00   2.49 / 1.00   1.70 / 0.79
  AdamW      1.00 / 0.82   2.49 / 1.00   1.70 / 0.40
  SGD        1.00 / 1.00   -             -
  RMSprop    1.00 / 1.00   -             2.31 / 1.50
  Adagrad    1.28 / 1.00   -             5.63 / 1.00
  Adamax     4.30 / 1.00   2.49 / 1.00   1.00 / 1.00
  Adadelta   1.00 / 1.00   1.82 / 1.09   1.99 / 1.87
  ASGD       1.00 / 1.00   1.00 / 1.00   -            (m = ax)

  clipping (c), Adam and SGD: params 1.00, the clipped gradient 0.02 (torch's
  fp32 norm is the less accurate one)
  L-BFGS direction (h): num = 1: 1.00, 3: 1.00, 100: 1.00, 128: 1.03

Nothing is above the margin of 8, so no tensor has a margin of its own.  The
values above 1 are where the kernel's separately rounded steps meet a fused
torch op: g + wd p then g g (Adagrad's sum, addcmul), the lerp of the first
moments, m / u under Adamax's addcdiv.
"""
import ctypes
import math
from importlib import import_module

import numpy as np
import pytest
import torch

import optim_reference as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu

F64 = np.float64
M_SENTINEL, V_SENTINEL = 7.5, -3.25      # what the unused elements of m / v hold before a call


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def _spec(pkg):
    return pkg.ProblemSpec(mu_a=0.05, sig_a=0.2, phi_r=0.05, g="call_mean", strike=1.0)


@pytest.fixture(scope="module")
def ctx_s(pkg, dev):
    """Context S: one block of the 256 x 256 grid-stride loop, a ragged tail, unused elements."""
    s = pkg.NativeSolver("NAIS-Net", [5, 16, 16, 16, 16, 1], "Sine", _spec(pkg), 1.0, dev)
    assert s.nparams < 65536 and s.nparams % 256 != 0 and not s.used_mask.all()
    return s


@pytest.fixture(scope="module")
def ctx_l(pkg, dev):
    """Context L: the grid-stride second pass runs and all 256 norm partials carry data."""
    s = pkg.NativeSolver("NAIS-Net", [101, 110, 110, 110, 110, 1], "Sine", _spec(pkg), 1.0, dev)
    assert s.nparams > 65536 and not s.used_mask.all()
    return s


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _sets(kind):
    return {"default": (R.DEFAULT_LR, R.DEFAULTS[kind]), "nondefault": (R.LRS[kind], R.NONDEFAULT[kind])}


class _Report:
    """Figures first, verdict after: every comparison prints its ratio, the
    test fails at the end if any was outside the rule."""

    def __init__(self):
        self.bad = []

    def rule(self, tag, got, x64, x32, sel=None, margin=R.MARGIN):
        got, x64, x32 = (np.asarray(a, F64) for a in (got, x64, x32))
        if sel is not None:
            got, x64, x32 = got[sel], x64[sel], x32[sel]
        tol, e32 = R.tolerance(x64, x32, margin)
        err = float(np.abs(got - x64).max())
        ratio = err / e32 if e32 > 0 else err / tol
        print(f"RATIO {tag} err={err:.3e} e32={e32:.3e} ratio={ratio:.2f}{'' if e32 > 0 else ' (of the floor)'}")
        if not err <= tol:
            self.bad.append((tag, err, e32, tol))

    def check(self, tag, ok):
        if not ok:
            self.bad.append((tag,))

    def done(self):
        assert not self.bad, self.bad


def _device_buffers(dev, used, p, g, m, v):
    """Device copies; the unused elements of m / v hold the sentinels."""
    n = p.size
    mm = np.zeros(n, np.float32) if m is None else m.copy()
    vv = np.zeros(n, np.float32) if v is None else v.copy()
    mm[~used], vv[~used] = M_SENTINEL, V_SENTINEL
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (p, g, mm, vv)) + (mm, vv)


def _step_keywords(kind, lr, opts, t, mode, dev, parity=0):
    kw = dict(kind=kind, lr=lr, **opts)
    state = None
    if mode == "device":
        state = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
        state[parity] = float(t - 1)
        kw.update(step_state=state, step_parity=parity)
    else:
        kw.update(step=t)
        if kind == "ASGD":     # the fp32 values torch's recursion stored after update t - 1
            eta, mu = R.asgd_eta_mu(t, R.f32(lr), R.f32(opts["lambd"]))
            kw.update(asgd_eta=R.f32(eta), asgd_mu=R.f32(mu))
    return kw, state


def _single_update(rep, s, dev, kind, setname, t, modes=("device", "host")):
    used = s.used_mask.numpy()
    lr, opts = _sets(kind)[setname]
    p, g, m, v = R.make_inputs(s.nparams, used, kind, seed=1000 + t % 997)
    if t == 1:
        m = v = None
    x64 = R.reference_update(kind, p, g, m, v, t, lr, torch.float64, used=used, **opts)
    x32 = R.reference_update(kind, p, g, m, v, t, lr, torch.float32, used=used, **opts)
    owned = R.STATE_KEYS[kind]
    for mode in modes:
        for parity in ((0, 1) if mode == "device" else (0,)):
            tag = f"{kind} {setname} t={t} {mode}{parity if mode == 'device' else ''}"
            P, G, Mb, Vb, m0, v0 = _device_buffers(dev, used, p, g, m, v)
            kw, state = _step_keywords(kind, lr, opts, t, mode, dev, parity)
            s.optimizer_step(P, G, Mb, Vb, **kw)
            torch.cuda.synchronize()
            gp, gg, gm, gv = (x.cpu().numpy() for x in (P, G, Mb, Vb))
            rep.rule(f"{tag} params", gp, x64[0], x32[0], used)
            for name, got, before, i in (("m", gm, m0, 1), ("v", gv, v0, 2)):
                if name in owned:
                    rep.rule(f"{tag} {name}", got, x64[i], x32[i], used)
                    rep.check(f"{tag} unused {name} untouched", _same_bits(got[~used], before[~used]))
                else:
                    rep.check(f"{tag} {name} not owned, untouched", _same_bits(got, before))
            rep.check(f"{tag} unused params untouched", _same_bits(gp[~used], p[~used]))
            rep.check(f"{tag} used params moved", bool(np.any(gp[used] != p[used])))
            rep.check(f"{tag} gradient buffer unchanged without a clip", _same_bits(gg, g))
            if state is not None:
                st = state.cpu().numpy()
                rep.check(f"{tag} counter", st[1 - parity] == float(t) and st[parity] == float(t - 1))


# --------------------------------------------------------------------------- a. single update from injected state
@pytest.mark.parametrize("setname", ["default", "nondefault"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_single_update_matches_torch(ctx_s, dev, kind, setname):
    """Update t of every kind from injected state, t in {1, 2, 37, 1000,
    1,000,007} (the last is ASGD's averaging branch), step count from the
    device counter (both parities) and from the host: params and the owned
    moments by the rule; unused elements, moments the kind does not own and
    the gradient buffer bitwise unchanged."""
    rep = _Report()
    for t in R.STEPS:
        _single_update(rep, ctx_s, dev, kind, setname, t)
    rep.done()


@pytest.mark.parametrize("setname", ["default", "nondefault"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_single_update_past_one_grid_pass(ctx_l, dev, kind, setname):
    """The same at more than 65,536 parameters (the grid-stride second pass)."""
    rep = _Report()
    for t in (1, 37):
        _single_update(rep, ctx_l, dev, kind, setname, t)
    rep.done()


def test_asgd_averaging_branch_on_the_device(ctx_s, dev):
    """t = 1,000,007: mu = 1/6, so ax += (p - ax) mu and ax != p afterwards."""
    s, t = ctx_s, 1_000_007
    used = s.used_mask.numpy()
    lr, opts = _sets("ASGD")["nondefault"]
    p, g, m, v = R.make_inputs(s.nparams, used, "ASGD", seed=1000 + t % 997)
    for mode in ("device", "host"):
        P, G, Mb, Vb, _, _ = _device_buffers(dev, used, p, g, m, v)
        kw, _ = _step_keywords("ASGD", lr, opts, t, mode, dev)
        if mode == "host":
            assert kw["asgd_mu"] == R.f32(1.0 / 6.0)
        s.optimizer_step(P, G, Mb, Vb, **kw)
        torch.cuda.synchronize()
        gp, ax = P.cpu().numpy(), Mb.cpu().numpy()
        assert np.all(ax[used] != gp[used])
        want = m[used].astype(F64) + (gp[used].astype(F64) - m[used]) * R.f32(1.0 / 6.0)
        np.testing.assert_allclose(ax[used], want, rtol=0, atol=2.0 ** -22 * np.abs(want).max())


# --------------------------------------------------------------------------- b. short trajectories
@pytest.mark.parametrize("kind", R.KINDS)
def test_trajectory_of_25_updates(ctx_s, dev, kind):
    """25 updates with the device counter (alternating parity) and gradients
    g U(0.5, 2) per step against a float64 torch trajectory fed the same fp32
    gradients; the counter reads 25."""
    s = ctx_s
    used = s.used_mask.numpy()
    lr, opts = _sets(kind)["nondefault"]
    p, g, _, _ = R.make_inputs(s.nparams, used, kind, seed=77)
    rs = np.random.RandomState(78)
    grads = [(g * np.float32(rs.uniform(0.5, 2.0))).astype(np.float32) for _ in range(25)]
    x64 = R.reference_trajectory(kind, p, grads, lr, torch.float64, used=used, **opts)
    x32 = R.reference_trajectory(kind, p, grads, lr, torch.float32, used=used, **opts)
    P, G, Mb, Vb, m0, v0 = _device_buffers(dev, used, p, g, None, None)
    state = torch.zeros(2, dtype=torch.float64, device=dev)
    for k, gk in enumerate(grads):
        G.copy_(torch.from_numpy(gk))
        s.optimizer_step(P, G, Mb, Vb, kind=kind, lr=lr, step=k + 1, step_state=state, step_parity=k & 1, **opts)
    torch.cuda.synchronize()
    assert int(state[25 & 1].item()) == 25
    rep = _Report()
    gp, gm, gv = (x.cpu().numpy() for x in (P, Mb, Vb))
    rep.rule(f"traj {kind} params", gp, x64[0], x32[0], used)
    for name, got, before, i in (("m", gm, m0, 1), ("v", gv, v0, 2)):
        if name in R.STATE_KEYS[kind]:
            rep.rule(f"traj {kind} {name}", got, x64[i], x32[i], used)
            rep.check(f"traj {kind} unused {name}", _same_bits(got[~used], before[~used]))
        else:
            rep.check(f"traj {kind} {name} not owned", _same_bits(got, before))
    rep.check(f"traj {kind} unused params", _same_bits(gp[~used], p[~used]))
    rep.done()


# --------------------------------------------------------------------------- c. clipping
@pytest.mark.parametrize("norm", [10.0, 0.1])
@pytest.mark.parametrize("kind", ["Adam", "SGD"])
def test_clip_grad_norm(ctx_l, dev, kind, norm):
    """max_norm = 1 with the gradient norm above it (coefficient 1 / 10) and
    below it (clamped to exactly 1): params by the rule, and the gradient
    buffer afterwards is torch's clipped gradient -- bitwise the input in the
    second case.  The unused elements of the gradient buffer hold garbage:
    torch has no gradient there, so they are outside the norm and stay."""
    s, t = ctx_l, 2
    used = s.used_mask.numpy()
    lr, opts = _sets(kind)["nondefault"]
    p, g, m, v = R.make_inputs(s.nparams, used, kind, seed=5)
    g = (g * np.float32(norm / np.linalg.norm(g.astype(F64)))).astype(np.float32)
    g[~used] = 1000.0
    x64 = R.reference_update(kind, p, g, m, v, t, lr, torch.float64, used=used, max_norm=1.0, **opts)
    x32 = R.reference_update(kind, p, g, m, v, t, lr, torch.float32, used=used, max_norm=1.0, **opts)
    P, G, Mb, Vb, _, _ = _device_buffers(dev, used, p, g, m, v)
    kw, _ = _step_keywords(kind, lr, opts, t, "device", dev)
    s.optimizer_step(P, G, Mb, Vb, max_norm=1.0, **kw)
    torch.cuda.synchronize()
    gp, gg = P.cpu().numpy(), G.cpu().numpy()
    rep = _Report()
    rep.rule(f"clip {kind} norm={norm} params", gp, x64[0], x32[0], used)
    if norm < 1.0:
        rep.check("gradient bitwise unchanged below max_norm", _same_bits(gg, g))
        rep.check("torch's is too", _same_bits(x32[3], g))
    else:
        rep.rule(f"clip {kind} norm={norm} gradient", gg, x64[3], x32[3], used)
        rep.check("clipped to norm 1", abs(np.linalg.norm(gg[used].astype(F64)) - 1.0) < 1e-5)
    rep.check("unused gradient elements untouched", _same_bits(gg[~used], g[~used]))
    rep.check("unused params untouched", _same_bits(gp[~used], p[~used]))
    rep.done()


# --------------------------------------------------------------------------- d. NaN skip
@pytest.mark.parametrize("kind", R.KINDS)
def test_nonfinite_loss_skips_every_kind(ctx_s, dev, kind):
    """A NaN, +inf or -inf loss leaves params, m, v and the device step count
    unchanged; the finite call after them is a fresh optimizer's first update,
    bit for bit."""
    s = ctx_s
    used = s.used_mask.numpy()
    lr, opts = _sets(kind)["nondefault"]
    p, g, _, _ = R.make_inputs(s.nparams, used, kind, seed=9)

    def run(losses):
        P, G, Mb, Vb, m0, v0 = _device_buffers(dev, used, p, g, None, None)
        state = torch.zeros(2, dtype=torch.float64, device=dev)
        for k, lv in enumerate(losses):
            loss = torch.tensor([lv], device=dev)
            s.optimizer_step(P, G, Mb, Vb, kind=kind, lr=lr, step=k + 1, step_state=state, step_parity=k & 1,
                             skip_nonfinite_loss=loss, **opts)
            torch.cuda.synchronize()
            if not math.isfinite(lv):
                assert _same_bits(P.cpu().numpy(), p) and _same_bits(Mb.cpu().numpy(), m0)
                assert _same_bits(Vb.cpu().numpy(), v0) and _same_bits(G.cpu().numpy(), g)
                assert float(state[(k + 1) & 1].item()) == 0.0
        return [x.cpu().numpy() for x in (P, Mb, Vb)], int(state[len(losses) & 1].item())

    skipped, n_skipped = run([float("nan"), float("inf"), float("-inf"), 1.0])
    fresh, n_fresh = run([1.0])
    assert n_skipped == n_fresh == 1
    for a, b in zip(skipped, fresh):
        assert _same_bits(a, b)
    assert np.any(fresh[0][used] != p[used])


# --------------------------------------------------------------------------- e. the fused update
LAYOUTS = {
    "NAIS-Net-16-K3": ("NAIS-Net", [5, 16, 16, 16, 16, 1]),
    "Naisnet-16-K3": ("Naisnet", [5, 16, 16, 16, 16, 1]),
    "NAIS-Net-16-K1": ("NAIS-Net", [5, 16, 16, 1]),
    "NAIS-Net-110-K3": ("NAIS-Net", [101, 110, 110, 110, 110, 1]),
    "NAIS-Net-16-K5": ("NAIS-Net", [5] + 6 * [16] + [1]),         # the finalize table at P = 12 problem tiles
    "NAIS-Net-110-K1": ("NAIS-Net", [101, 110, 110, 1]),          # 7-block tiles at P = 4
}
FUSED_CASES = [("NAIS-Net-16-K3", k) for k in R.KINDS] + \
    [(lay, k) for lay in ("Naisnet-16-K3", "NAIS-Net-16-K1", "NAIS-Net-110-K3", "NAIS-Net-16-K5", "NAIS-Net-110-K1")
     for k in ("Adam", "Adadelta", "ASGD")]


@pytest.fixture(scope="module")
def fused_ctx(pkg, dev):
    cache = {}

    def get(layout):
        if layout not in cache:
            mode, layers = LAYOUTS[layout]
            nets = import_module(pkg.__name__ + ".networks")
            torch.manual_seed(0)
            flat = torch.cat([q.reshape(-1) for q in nets.make_model(mode, layers, "Sine").state_dict().values()])
            cache[layout] = (pkg.NativeSolver(mode, layers, "Sine", _spec(pkg), 1.0, dev), flat.float().contiguous())
        return cache[layout]
    return get


def _launches(s, name):
    return s.profile_read().get(name, {"launches": 0})["launches"]


@pytest.mark.parametrize("layout,kind", FUSED_CASES)
def test_fused_update_equals_separate_launches(fused_ctx, dev, layout, kind):
    """dbsde_train_step with the update folded into the gradient finalize
    (non-default options, device counter with alternating parity) over three
    steps at M = 64, N = 5 == dbsde_loss_grad + dbsde_optimizer_step on a twin
    copy: params, m, v and the counter bit-identical, unused elements
    untouched in both arms.  The profile proves which arm ran: no `optimizer`
    launch in the fused one, three with max_norm = 1 (the documented
    fallback)."""
    s, p0 = fused_ctx(layout)
    used = s.used_mask.numpy()
    lr, opts = _sets(kind)["nondefault"]
    M, N, D = 64, 5, s.D
    Xi = torch.ones(D, device=dev)
    p0n = p0.numpy()
    zeros = np.zeros(s.nparams, np.float32)

    def arm(fused, max_norm=0.0):
        P, G, Mb, Vb, m0, v0 = _device_buffers(dev, used, p0n, zeros, None, None)
        state = torch.zeros(2, dtype=torch.float64, device=dev)
        loss = torch.zeros(1, device=dev)
        for k in range(3):
            # the keywords FBSNN._opt_kwargs builds, with this test's options
            kw = dict(kind=kind, lr=lr, max_norm=max_norm, step=k + 1, skip_nonfinite_loss=None, step_state=state,
                      step_parity=k & 1, **opts)
            if fused:
                s.train_step(P, M, N, Xi, G, Mb, Vb, kw, seed=k, loss=loss)
            else:
                s.loss_grad(P, M, N, Xi, seed=k, grad=G, loss=loss)
                s.optimizer_step(P, G, Mb, Vb, **kw)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (P, Mb, Vb, G)], int(state[3 & 1].item()), (m0, v0)

    a, na, (m0, v0) = arm(True)
    b, nb, _ = arm(False)
    assert na == nb == 3
    for name, x, y in zip(("params", "m", "v", "grad"), a, b):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"{layout} {kind} {name}")   # (NaN == NaN bitwise)
    for arm_out in (a, b):
        assert _same_bits(arm_out[0][~used], p0n[~used])
        assert _same_bits(arm_out[1][~used], m0[~used]) and _same_bits(arm_out[2][~used], v0[~used])
    assert np.any(a[0][used] != p0n[used])
    print(f"FUSED {layout} {kind} finite={bool(np.isfinite(a[0]).all())}")
    # which arm ran
    s.profile(True)
    try:
        s.profile_reset()
        arm(True)
        assert _launches(s, "optimizer") == 0 and _launches(s, "grad_finalize_update") == 3
        s.profile_reset()
        arm(True, max_norm=1.0)
        assert _launches(s, "optimizer") == 3 and _launches(s, "grad_finalize_update") == 0
    finally:
        s.profile_reset()
        s.profile(False)


# --------------------------------------------------------------------------- f. dbsde_vec_reduce
VEC_N = [1, 255, 256, 257, 65_535, 65_537, 200_003]


def _wide(rs, n):
    return (rs.choice([-1.0, 1.0], n) * np.exp(rs.uniform(-9.0, 9.0, n))).astype(np.float32)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", VEC_N)
def test_vec_reduce(ctx_s, dev, n, offset):
    """dot / asum against math.fsum within n 2^-52 sum|a_i b_i| (resp. sum|a_i|),
    the bound of an fp64 sum of exact products in any order; amax exactly.
    offset 1: views starting at an odd element of a larger buffer, as the rows
    of S / Y that _lbfgs_step passes."""
    rs = np.random.RandomState(n)
    a, b = _wide(rs, n), _wide(rs, n)
    bufa = torch.from_numpy(np.concatenate([_wide(rs, offset), a, _wide(rs, 3)])).to(dev)
    bufb = torch.from_numpy(np.concatenate([_wide(rs, offset), b, _wide(rs, 3)])).to(dev)
    ta, tb = bufa[offset:offset + n], bufb[offset:offset + n]
    a64, b64 = a.astype(F64), b.astype(F64)
    prod = a64 * b64                                     # exact: 24 x 24 bits
    got = ctx_s.vec_reduce("dot", ta, tb)
    assert abs(got - math.fsum(prod)) <= n * 2.0 ** -52 * math.fsum(np.abs(prod))
    got = ctx_s.vec_reduce("asum", ta)
    assert abs(got - math.fsum(np.abs(a64))) <= n * 2.0 ** -52 * math.fsum(np.abs(a64))
    assert ctx_s.vec_reduce("amax", ta) == float(np.abs(a64).max())
    # the largest magnitude negative and in the last element
    a[n - 1] = -np.float32(3.0e4)
    bufa[offset + n - 1] = float(a[n - 1])
    assert ctx_s.vec_reduce("amax", ta) == 3.0e4


@pytest.mark.parametrize("where", ["first", "last", "past-65536"])
def test_vec_reduce_propagates_nan(ctx_s, dev, where):
    """One NaN element: amax is NaN as tensor.abs().max() (not 0 or the largest
    finite magnitude, which the L-BFGS driver would read as converged), and so
    are asum and dot."""
    n = 200_003
    rs = np.random.RandomState(4)
    a, b = _wide(rs, n), _wide(rs, n)
    a[{"first": 0, "last": n - 1, "past-65536": 70_001}[where]] = np.nan
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    assert math.isnan(float(torch.from_numpy(a).abs().max()))
    for op in ("amax", "asum", "dot"):
        assert math.isnan(ctx_s.vec_reduce(op, ta, tb if op == "dot" else None)), op


# --------------------------------------------------------------------------- g. dbsde_vec_axpby
@pytest.mark.parametrize("n", VEC_N)
def test_vec_axpby(ctx_s, dev, n):
    """z = alpha x + beta y within 1.01 2^-23 (|alpha x| + |beta y|) per element
    (two product roundings and the sum's, with or without contraction), for
    y = None, z aliasing x, z aliasing y and beta = 0 with y given; alpha = -1
    is the negation bitwise; elements past n stay."""
    rs = np.random.RandomState(n + 1)
    pad = 5
    x = (rs.standard_normal(n + pad) * np.exp(rs.uniform(-3, 3, n + pad))).astype(np.float32)
    y = (rs.standard_normal(n + pad) * np.exp(rs.uniform(-3, 3, n + pad))).astype(np.float32)
    alpha, beta = R.f32(0.37), R.f32(-1.7)
    dv = lambda a: torch.from_numpy(a.copy()).to(dev)   # noqa: E731

    def check(z, al, be, yy):
        z = z.cpu().numpy()
        ax = al * x[:n].astype(F64)
        by = be * yy[:n].astype(F64) if yy is not None else np.zeros(n)
        assert np.all(np.abs(z[:n] - (ax + by)) <= 1.01 * 2.0 ** -23 * (np.abs(ax) + np.abs(by)))
        return z

    sentinel = np.full(n + pad, 123.0, np.float32)
    Z, X, Y = dv(sentinel), dv(x), dv(y)
    ctx_s.vec_axpby(Z[:n], X[:n], alpha, Y[:n], beta)
    z = check(Z, alpha, beta, y)
    assert _same_bits(z[n:], sentinel[n:])
    Z = dv(sentinel)
    ctx_s.vec_axpby(Z[:n], X[:n], alpha)                       # y = None
    assert _same_bits(check(Z, alpha, 0.0, None)[n:], sentinel[n:])
    ctx_s.vec_axpby(Z[:n], X[:n], alpha, Y[:n], 0.0)           # beta = 0 with y given
    check(Z, alpha, 0.0, y)
    Z = dv(sentinel)
    ctx_s.vec_axpby(Z[:n], X[:n], -1.0)                        # negation
    assert _same_bits(Z.cpu().numpy()[:n], -x[:n])
    X2 = dv(x)
    ctx_s.vec_axpby(X2[:n], X2[:n], alpha, Y[:n], beta)        # z aliases x
    assert _same_bits(check(X2, alpha, beta, y)[n:], x[n:])
    Y2 = dv(y)
    ctx_s.vec_axpby(Y2[:n], X[:n], alpha, Y2[:n], beta)        # z aliases y
    assert _same_bits(check(Y2, alpha, beta, y)[n:], y[n:])
    assert _same_bits(X.cpu().numpy(), x) and _same_bits(Y.cpu().numpy(), y)


# --------------------------------------------------------------------------- h. dbsde_lbfgs_direction
@pytest.mark.parametrize("num", [0, 1, 3, 100, 128])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 82_003])
def test_lbfgs_direction(ctx_s, dev, n, num):
    """The two-loop recursion over a wrapped, non-contiguous ring of history
    rows (ld = n and n + 5) against the float64 recursion by the rule, the
    numpy mirror as the working-precision reference; num = 0 is -g h_diag
    bitwise.  Rows outside `slots` and columns past n are NaN and must not
    reach the result; the elements of d's buffer past n stay."""
    rep = _Report()
    for ld in (n, n + 5):
        g, S, Y, slots, ro, h = R.lbfgs_history(n, num, ld, seed=n + num)
        dbuf = torch.full((n + 4,), 55.0, device=dev)
        tg, tS, tY = (torch.from_numpy(a).to(dev) for a in (g, S, Y))
        ctx_s.lbfgs_direction(tg, tS, tY, slots, ro, h, dbuf[:n])
        torch.cuda.synchronize()
        d = dbuf.cpu().numpy()
        assert np.all(d[n:] == 55.0)
        assert np.isfinite(d[:n]).all()
        if num == 0:
            assert _same_bits(d[:n], -g * np.float32(h))
            continue
        truth = R.lbfgs_direction_reference(g, S, Y, slots, ro, h, mirror=False)
        mirror = R.lbfgs_direction_reference(g, S, Y, slots, ro, h, mirror=True)
        rep.rule(f"direction n={n} num={num} ld={ld}", d[:n], truth, mirror)
    rep.done()


def test_lbfgs_direction_rejects_bad_arguments(pkg, ctx_s, dev):
    """More than 128 history entries, a negative slot and ld < n are
    DBSDE_EINVAL (ValueError) and launch nothing."""
    s, n = ctx_s, 300
    g = torch.ones(n, device=dev)
    d = torch.full((n,), 55.0, device=dev)
    S = torch.ones(132, n, device=dev)
    lib, vp = s.lib, ctypes.c_void_p

    def raw(ld, nn, slots, num):
        sl = (ctypes.c_int * len(slots))(*slots)
        ro = (ctypes.c_float * len(slots))(*([1.0] * len(slots)))
        return lib.dbsde_lbfgs_direction(s.ctx, vp(g.data_ptr()), vp(S.data_ptr()), vp(S.data_ptr()), ld, nn, sl, ro,
                                         num, 1.0, vp(d.data_ptr()))

    s.profile(True)
    try:
        s.profile_reset()
        with pytest.raises(ValueError):
            s.lbfgs_direction(g, S, S, list(range(129)), [1.0] * 129, 1.0, d)
        with pytest.raises(ValueError):
            s.lbfgs_direction(g, S, S, [0, -1, 2], [1.0] * 3, 1.0, d)
        with pytest.raises(ValueError):
            s.lbfgs_direction(g, S[:, :n - 1].contiguous(), S[:, :n - 1].contiguous(), [0, 1], [1.0] * 2, 1.0, d)
        einval = pkg._lib.DBSDE_EINVAL
        assert raw(n - 1, n, [0, 1], 2) == einval          # ld < n at the C ABI
        assert raw(n, n, list(range(129)), 129) == einval
        assert raw(n, n, [0, -1, 2], 3) == einval
        assert _launches(s, "lbfgs_direction") == 0
        assert raw(n, n, [0, 1], 2) == pkg._lib.DBSDE_OK     # the same call with good arguments runs
        assert _launches(s, "lbfgs_direction") == 1
    finally:
        s.profile_reset()
        s.profile(False)
    torch.cuda.synchronize()
    assert torch.isfinite(d).all() and not bool((d == 55.0).all())
