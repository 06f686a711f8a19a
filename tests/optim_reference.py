"""Torch-CPU reference of the optimizer update (dbsde_optimizer_step, the fused
update of dbsde_train_step) and of the L-BFGS two-loop recursion
(dbsde_lbfgs_direction, include/dbsde.h) -- test infrastructure only.

reference_update is ONE torch.optim.<kind> update number t from injected state
(step = t - 1, the moments, ASGD's eta / mu), single-tensor path
(foreach=False), in float64 (the truth: the fp32 inputs upcast) or float32 (the
reference at working precision).  Only the used elements are handed to torch:
NAIS-Net's never-used input_layers[K] has grad None there, so torch applies no
weight decay and no state update to it; the unused elements come back as given.

The options reach the device as C floats (dbsde_optim), so the reference
rounds each of them to binary32 first (f32opts): both sides then compute with
the same numbers.  The non-default sets (NONDEFAULT) are exactly representable
anyway.

lbfgs_direction_reference is the recursion of include/dbsde.h in float64
(mirror=False, the truth) or in the kernel's arithmetic (mirror=True: fp32
vectors, fp64 dot products rounded to fp32, fp32 al / be).

tolerance(x64, x32, margin) is the rule every comparison of the optimizer and
direction tests uses: margin x the reference's own rounding error
e32 = max|x32 - x64|, floored at 2^-24 max|x64| when e32 == 0.
"""
from __future__ import annotations

import numpy as np
import torch

KINDS = ("Adam", "AdamW", "SGD", "RMSprop", "Adagrad", "Adamax", "Adadelta", "ASGD")
STEPS = (1, 2, 37, 1000, 1_000_007)
MARGIN = 8.0

# which device buffers a kind owns, and the torch state key behind each
STATE_KEYS = {
    "Adam": dict(m="exp_avg", v="exp_avg_sq"),
    "AdamW": dict(m="exp_avg", v="exp_avg_sq"),
    "SGD": dict(),
    "RMSprop": dict(v="square_avg"),
    "Adagrad": dict(v="sum"),
    "Adamax": dict(m="exp_avg", v="exp_inf"),
    "Adadelta": dict(m="acc_delta", v="square_avg"),
    "ASGD": dict(m="ax"),
}

# torch.optim defaults (optim.X(params, lr=lr)), in NativeSolver.optimizer_step's keywords
DEFAULTS = {
    "Adam": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "AdamW": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
    "SGD": dict(weight_decay=0.0),
    "RMSprop": dict(alpha=0.99, eps=1e-8, weight_decay=0.0),
    "Adagrad": dict(eps=1e-10, lr_decay=0.0, weight_decay=0.0),
    "Adamax": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "Adadelta": dict(rho=0.9, eps=1e-6, weight_decay=0.0),
    "ASGD": dict(lambd=1e-4, weight_decay=0.0),
}
DEFAULT_LR = 1e-3

# one non-default set per kind, every value exactly representable in binary32
# (ASGD's alpha / t0 stay at torch's defaults: the ABI hard-codes them)
#
# The values are chosen so that every option moves the parameters by at least
# 100 tolerances at every step count of STEPS where torch's formula depends on
# it at all (tests/test_optim_reference_cpu.py holds them to that):
#   Adagrad: clr = lr / (1 + (t - 1) lr_decay) shrinks every other option's
#     effect with t and bounds the whole update by clr, so lr is 1, lr_decay
#     2^-12 (clr = 4.1e-3 at t = 10^6+7, and still 187 tolerances at t = 2) and
#     eps 2^-10;
#   ASGD: eta ~ lr / 22 at t = 10^6+7, so weight_decay is 0.25.
LR = 2.0 ** -7
LRS = {k: LR for k in KINDS}
LRS["Adagrad"] = 1.0
# (kind, option) pairs torch's update does not depend on at t = 1 from zero
# moments: the bias-corrected first step of Adam / AdamW / Adamax is g and g^2
# (|g| + eps for Adamax) whatever the betas, and Adagrad's clr is lr
INERT_AT_FIRST_STEP = {("Adam", "beta1"), ("Adam", "beta2"), ("AdamW", "beta1"), ("AdamW", "beta2"),
                       ("Adamax", "beta1"), ("Adamax", "beta2"), ("Adagrad", "lr_decay")}
NONDEFAULT = {
    "Adam": dict(betas=(0.75, 0.9375), eps=2.0 ** -13, weight_decay=0.125),
    "AdamW": dict(betas=(0.75, 0.9375), eps=2.0 ** -13, weight_decay=0.125),
    "SGD": dict(weight_decay=0.125),
    "RMSprop": dict(alpha=0.875, eps=2.0 ** -13, weight_decay=0.125),
    "Adagrad": dict(eps=2.0 ** -10, lr_decay=2.0 ** -12, weight_decay=0.125),
    "Adamax": dict(betas=(0.75, 0.9375), eps=2.0 ** -13, weight_decay=0.125),
    "Adadelta": dict(rho=0.75, eps=2.0 ** -13, weight_decay=0.125),
    "ASGD": dict(lambd=2.0 ** -7, weight_decay=0.25),
}


def single_option_variants(kind):
    """(option name, the non-default set with that one option back at torch's
    default); the two betas count as one option each."""
    nd, df = NONDEFAULT[kind], DEFAULTS[kind]
    for k, v in nd.items():
        if k == "betas":
            yield "beta1", dict(nd, betas=(df["betas"][0], v[1]))
            yield "beta2", dict(nd, betas=(v[0], df["betas"][1]))
        else:
            yield k, dict(nd, **{k: df[k]})


def f32(x):
    """x rounded to binary32, as a Python float (what a C float argument holds)."""
    return float(np.float32(x))


def f32opts(options):
    return {k: tuple(f32(b) for b in v) if isinstance(v, tuple) else f32(v) for k, v in options.items()}


def asgd_eta_mu(t, lr, lambd):
    """ASGD's (eta, mu) going into update t: what torch's recursion stored after
    update t - 1 (lr and 1 before the first), as Python floats before the
    rounding to the fp32 state tensors."""
    if t <= 1:
        return lr, 1.0
    tp = t - 1
    return lr / ((1 + lambd * lr * tp) ** 0.75), 1 / max(1, tp - 1e6)


def make_inputs(n, used, kind, seed):
    """(p, g, m, v) fp32 of the issue's distributions: p ~ N(0,1);
    g = N(0,1) exp(U(-9,0)) with every 17th element exactly 0; m ~ 1e-2 N(0,1)
    (non-negative for Adadelta's acc_delta); v ~ U(0, 1e-3); g, m, v zero on
    the unused elements."""
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n).astype(np.float32)
    g = (rs.standard_normal(n) * np.exp(rs.uniform(-9.0, 0.0, n))).astype(np.float32)
    g[::17] = 0.0
    m = (1e-2 * rs.standard_normal(n)).astype(np.float32)
    if kind == "Adadelta":
        m = np.abs(m)
    v = rs.uniform(0.0, 1e-3, n).astype(np.float32)
    for x in (g, m, v):
        x[~used] = 0.0
    return p, g, m, v


def reference_update(kind, p, g, m, v, t, lr, dtype, used=None, max_norm=None, **options):
    """Update number t of torch.optim.<kind>(lr, **options) on parameters p with
    gradient g from injected state (m, v as STATE_KEYS maps them; zero moments
    when None).  Returns (p, m, v) as float64 arrays (a buffer the kind does
    not own comes back as given), and the clipped gradient as a fourth item
    when max_norm is given (clip_grad_norm_ before the step)."""
    n = p.size
    used = np.ones(n, bool) if used is None else np.asarray(used, bool)
    opts = f32opts(options)
    lr = f32(lr)
    tt = lambda a: torch.tensor(np.asarray(a)[used], dtype=dtype)   # noqa: E731
    P = tt(p).requires_grad_(True)
    opt = getattr(torch.optim, kind)([P], lr=lr, foreach=False, **opts)
    # one zero-gradient step creates the state; then the parameters are restored
    P.grad = torch.zeros_like(P)
    opt.step()
    with torch.no_grad():
        P.copy_(tt(p))
    st = opt.state[P]
    keys = STATE_KEYS[kind]
    with torch.no_grad():
        if "step" in st:
            st["step"].fill_(float(t - 1))
        for buf, key in keys.items():
            src = m if buf == "m" else v
            st[key].copy_(tt(src) if src is not None else torch.zeros_like(P))
        if kind == "ASGD":
            eta, mu = asgd_eta_mu(t, lr, opts.get("lambd", 1e-4))
            st["eta"].copy_(torch.as_tensor(eta))
            st["mu"].copy_(torch.as_tensor(mu))
    P.grad = tt(g)
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_([P], max_norm=max_norm, foreach=False)
    gc = P.grad.detach().clone()
    opt.step()
    assert "step" not in st or float(st["step"]) == float(t)

    def full(base, sub):
        out = (np.zeros(n) if base is None else np.asarray(base)).astype(np.float64)
        out[used] = sub.detach().double().numpy()
        return out

    res = (full(p, P),
           full(m, st[keys["m"]]) if "m" in keys else (None if m is None else np.asarray(m, np.float64)),
           full(v, st[keys["v"]]) if "v" in keys else (None if v is None else np.asarray(v, np.float64)))
    return res + (full(g, gc),) if max_norm is not None else res


def reference_trajectory(kind, p, grads, lr, dtype, used=None, **options):
    """len(grads) updates of a fresh torch.optim.<kind>(lr, **options) fed the
    fp32 gradients `grads` in turn; (p, m, v) as reference_update returns them
    (zeros for a buffer the kind does not own)."""
    n = p.size
    used = np.ones(n, bool) if used is None else np.asarray(used, bool)
    P = torch.tensor(p[used], dtype=dtype).requires_grad_(True)
    opt = getattr(torch.optim, kind)([P], lr=f32(lr), foreach=False, **f32opts(options))
    for g in grads:
        P.grad = torch.tensor(np.asarray(g)[used], dtype=dtype)
        opt.step()
    st, keys = opt.state[P], STATE_KEYS[kind]

    def full(base, sub):
        out = np.asarray(base, np.float64).copy()
        out[used] = sub.detach().double().numpy()
        return out

    z = np.zeros(n)
    return (full(p, P), full(z, st[keys["m"]]) if "m" in keys else z, full(z, st[keys["v"]]) if "v" in keys else z)


def tolerance(x64, x32, margin=MARGIN):
    """(tol, e32): margin x the working-precision reference's own error
    e32 = max|x32 - x64|; when e32 == 0 the floor 2^-24 max|x64|."""
    x64, x32 = np.asarray(x64, np.float64), np.asarray(x32, np.float64)
    e32 = float(np.abs(x32 - x64).max())
    if e32 == 0.0:
        return 2.0 ** -24 * float(np.abs(x64).max()), 0.0
    return margin * e32, e32


def lbfgs_history(n, num, ld, seed):
    """A wrapped ring of L-BFGS history from a diagonal SPD quadratic:
    s_i ~ N(0,1), y_i = A s_i with A = diag(U(0.5, 2)), ro_i = fp32(1 / (y_i . s_i)),
    h_diag = ys / (y . y) of the newest pair as torch computes it (fp32
    scalars), in [num + 3, ld] matrices whose other rows and columns past n
    are NaN.  Returns (g, S, Y, slots (oldest first), ro, h_diag)."""
    rs = np.random.RandomState(seed)
    rows = num + 3
    A = rs.uniform(0.5, 2.0, n)
    g = rs.standard_normal(n).astype(np.float32)
    S = np.full((rows, ld), np.nan, np.float32)
    Y = np.full((rows, ld), np.nan, np.float32)
    # the ring after wrap-around: three free rows spread over it, the live
    # rows in ring order starting past the middle
    free = {0, rows // 2, rows - 1}
    live = [r for r in range(rows) if r not in free]
    k = num // 3
    slots = live[k:] + live[:k]
    assert len(slots) == num
    ro, h_diag = [], 1.0
    for r in slots:
        s = rs.standard_normal(n).astype(np.float32)
        y = (A * s).astype(np.float32)
        S[r, :n], Y[r, :n] = s, y
        ys = np.float32(np.dot(y.astype(np.float64), s.astype(np.float64)))
        ro.append(float(np.float32(1.0) / ys))
        h_diag = float(ys / np.float32(np.dot(y.astype(np.float64), y.astype(np.float64))))
    return g, S, Y, slots, ro, h_diag


def lbfgs_direction_reference(g, S, Y, slots, ro, h_diag, mirror):
    """The two-loop recursion of include/dbsde.h over history rows `slots`
    (oldest first), columns [0, n) of S / Y:
      q = -g;  for i = num-1..0: al_i = (s_i . q) ro_i;  q += -al_i y_i
      r = q h_diag;  for i = 0..num-1: be_i = (y_i . r) ro_i;  r += (al_i - be_i) s_i
    mirror=False: all float64.  mirror=True: fp32 vectors with every product
    and sum rounded, fp64 dot products rounded to fp32, fp32 al / be."""
    n = np.asarray(g).size
    num = len(slots)
    if not mirror:
        d = np.float64
        q = -np.asarray(g, d)
        al = [0.0] * num
        for i in range(num - 1, -1, -1):
            s, y = S[slots[i], :n].astype(d), Y[slots[i], :n].astype(d)
            al[i] = float(np.dot(s, q)) * float(ro[i])
            q = q + (-al[i]) * y
        q = q * float(h_diag)
        for i in range(num):
            s, y = S[slots[i], :n].astype(d), Y[slots[i], :n].astype(d)
            be = float(np.dot(y, q)) * float(ro[i])
            q = q + (al[i] - be) * s
        return q
    f = np.float32
    dot = lambda u, w: f(np.dot(u.astype(np.float64), w.astype(np.float64)))   # noqa: E731
    q = -np.asarray(g, f)
    al = [f(0)] * num
    for i in range(num - 1, -1, -1):
        s, y = S[slots[i], :n], Y[slots[i], :n]
        al[i] = f(dot(s, q) * f(ro[i]))
        q = (q + (f(-al[i]) * y).astype(f)).astype(f)
    q = (q * f(h_diag)).astype(f)
    for i in range(num):
        s, y = S[slots[i], :n], Y[slots[i], :n]
        be = f(dot(y, q) * f(ro[i]))
        q = (q + (f(al[i] - be) * s).astype(f)).astype(f)
    return q.astype(np.float64)
