"""The conditions under which tests/test_gpu_optimizers.py means something,
checked on the reference alone (tests/optim_reference.py).  CPU.

Sensitivity: every option of every kind's non-default set, put back to
torch's default on its own, moves the fp32 reference's parameters by at least
100 tolerances (the tolerance rule of optim_reference.tolerance on params) at
every step count the GPU test uses -- so a device kernel that ignored the
option, or read the wrong one, cannot pass.  The only exceptions are the
(option, t = 1) pairs torch's own formula does not depend on
(INERT_AT_FIRST_STEP); those are asserted to be inert, and are live at t >= 2.
"""
import numpy as np
import pytest
import torch

import optim_reference as R
from test_host_logic import _CpuVecSolver

N = 4001
USED = np.ones(N, bool)
USED[100:164] = False          # a never-used block, as NAIS-Net's input_layers[K]


def _case(kind, t, seed=1):
    p, g, m, v = R.make_inputs(N, USED, kind, seed)
    if t == 1:                 # the first step starts from zero moments
        m = v = None
    return p, g, m, v


@pytest.mark.parametrize("t", R.STEPS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_every_option_moves_the_reference(kind, t):
    p, g, m, v = _case(kind, t)
    lr = R.LRS[kind]
    run = lambda dtype, o: R.reference_update(kind, p, g, m, v, t, lr, dtype, used=USED, **o)   # noqa: E731
    x64, x32 = run(torch.float64, R.NONDEFAULT[kind]), run(torch.float32, R.NONDEFAULT[kind])
    tol, e32 = R.tolerance(x64[0], x32[0])
    assert 0.0 < e32 < 1e-6
    for name, opts in R.single_option_variants(kind):
        moved = np.abs(run(torch.float32, opts)[0] - x32[0]).max()
        print(f"{kind} t={t} {name}: moved {moved:.3e} = {moved / tol:.1f} tolerances")
        if t == 1 and (kind, name) in R.INERT_AT_FIRST_STEP:
            assert moved <= tol, (kind, name, t, moved, tol)
        else:
            assert moved >= 100.0 * tol, (kind, name, t, moved, tol)


@pytest.mark.parametrize("kind", R.KINDS)
def test_unused_elements_come_back_as_given(kind):
    p, g, m, v = _case(kind, 37)
    m[~USED], v[~USED] = 3.0, 5.0
    out = R.reference_update(kind, p, g, m, v, 37, R.LRS[kind], torch.float32, used=USED, **R.NONDEFAULT[kind])
    for got, given in zip(out, (p, m, v)):
        np.testing.assert_array_equal(got[~USED], given[~USED].astype(np.float64))
    assert np.all(out[0][USED] != p[USED])       # weight decay 2^-3 acts on every used element


def test_first_step_equals_a_fresh_torch_optimizer():
    """t = 1 from injected zero state is torch's plain first step."""
    for kind in R.KINDS:
        p, g, _, _ = _case(kind, 1)
        got = R.reference_update(kind, p, g, None, None, 1, R.LRS[kind], torch.float32, **R.NONDEFAULT[kind])[0]
        P = torch.tensor(p, requires_grad=True)
        opt = getattr(torch.optim, kind)([P], lr=R.LRS[kind], foreach=False, **R.NONDEFAULT[kind])
        P.grad = torch.tensor(g)
        opt.step()
        np.testing.assert_array_equal(got, P.detach().double().numpy())


def test_injected_state_equals_torch_trajectory():
    """Update t from the state torch itself reached after t - 1 updates is
    torch's update t (the injection reproduces every piece of state)."""
    rs = np.random.RandomState(3)
    for kind in R.KINDS:
        p, g, _, _ = _case(kind, 1)
        P = torch.tensor(p, requires_grad=True)
        opt = getattr(torch.optim, kind)([P], lr=R.LRS[kind], foreach=False, **R.NONDEFAULT[kind])
        for _ in range(4):
            P.grad = torch.tensor(g * np.float32(rs.uniform(0.5, 2.0)))
            opt.step()
        st = opt.state[P]
        keys = R.STATE_KEYS[kind]
        p4 = P.detach().numpy().copy()
        m4 = st[keys["m"]].numpy().copy() if "m" in keys else None
        v4 = st[keys["v"]].numpy().copy() if "v" in keys else None
        got = R.reference_update(kind, p4, g, m4, v4, 5, R.LRS[kind], torch.float32, **R.NONDEFAULT[kind])
        P.grad = torch.tensor(g)
        opt.step()
        np.testing.assert_array_equal(got[0], P.detach().double().numpy(), err_msg=kind)
        for buf, i in (("m", 1), ("v", 2)):
            if buf in keys:
                np.testing.assert_array_equal(got[i], st[keys[buf]].double().numpy(), err_msg=kind)


def test_asgd_averaging_branch_at_a_million_steps():
    """ASGD at t = 1,000,007 takes torch's mu != 1 branch: ax += (p - ax) mu."""
    t = 1_000_007
    eta, mu = R.asgd_eta_mu(t, R.LRS["ASGD"], R.NONDEFAULT["ASGD"]["lambd"])
    assert mu == 1.0 / 6.0 and mu < 1.0 and 0.0 < eta < R.LRS["ASGD"]
    assert R.asgd_eta_mu(1_000_001, R.LR, 1e-4)[1] == 1.0      # the last step of the copy branch
    p, g, m, v = _case("ASGD", t)
    pn, ax, _ = R.reference_update("ASGD", p, g, m, None, t, R.LRS["ASGD"], torch.float32, used=USED,
                                   **R.NONDEFAULT["ASGD"])
    assert np.all(ax[USED] != pn[USED])
    want = m[USED].astype(np.float64) + (pn[USED] - m[USED]) * float(np.float32(mu))
    np.testing.assert_allclose(ax[USED], want, rtol=0, atol=2.0 ** -22 * np.abs(want).max())


def test_clip_returns_torchs_clipped_gradient():
    p, g, m, v = _case("Adam", 2)
    big = (g * np.float32(10.0 / np.linalg.norm(g.astype(np.float64)))).astype(np.float32)
    out = R.reference_update("Adam", p, big, m, v, 2, R.LR, torch.float32, used=USED, max_norm=1.0)
    assert abs(np.linalg.norm(out[3]) - 1.0) < 1e-5
    small = (big * np.float32(0.01)).astype(np.float32)
    out = R.reference_update("Adam", p, small, m, v, 2, R.LR, torch.float32, used=USED, max_norm=1.0)
    np.testing.assert_array_equal(out[3], small.astype(np.float64))   # torch multiplies by exactly 1.0


@pytest.mark.parametrize("n,num,ld", [(7, 0, 7), (7, 3, 7), (40, 5, 45), (300, 12, 300)])
def test_two_loop_mirror_agrees_with_the_cpu_stand_in(n, num, ld):
    """One definition of the recursion against the other: the mirror equals
    the _CpuVecSolver.lbfgs_direction contract of tests/test_host_logic.py
    (the stand-in the L-BFGS driver is tested on), and the float64 truth
    agrees with both to fp32 rounding."""
    g, S, Y, slots, ro, h = R.lbfgs_history(n, num, ld, seed=5)
    mirror = R.lbfgs_direction_reference(g, S, Y, slots, ro, h, mirror=True)
    truth = R.lbfgs_direction_reference(g, S, Y, slots, ro, h, mirror=False)
    d = torch.zeros(n)
    tS, tY = torch.from_numpy(S[:, :n].copy()), torch.from_numpy(Y[:, :n].copy())
    _CpuVecSolver().lbfgs_direction(torch.from_numpy(g), tS, tY, slots, ro, h, d)
    scale = np.abs(truth).max()
    np.testing.assert_allclose(d.double().numpy(), mirror, rtol=0, atol=2.0 ** -20 * scale)
    np.testing.assert_allclose(mirror, truth, rtol=0, atol=(num + 1) * 2.0 ** -18 * scale)
    if num == 0:
        np.testing.assert_array_equal(mirror, (-g * np.float32(h)).astype(np.float64))
