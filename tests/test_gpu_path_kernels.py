"""Every path kernel instance of csrc/paths.hpp that launch_paths
(csrc/rollout.hip) selects for diagonal, Cholesky-correlated (nb <= 128) and
plain Heston contexts, at the ragged shapes, sizes and keys of
tests/path_cases.py, against oracle/philox.py.  Needs an MI355X.
(Correlated Heston, two-factor Heston and nb > 128 sweep shapes in their own
suites.)

Which arm of launch_paths and which instance each test reaches:

  test_correlated_fetch_and_rollout     the `c->Lt && !ra.W` arm: rollout_corr_kernel<NBLK> for
                                        every NBLK = 1..8 (both sides of each block edge; D = 127,
                                        128 in a wide context, Dp = 144), as PATH_FETCH_DW,
                                        PATH_FETCH_W and PATH_ROLLOUT
  test_correlated_high_bit_key          the same arm, NBLK = 8, every key word above 2^31
  test_correlated_odd_shard             the same arm, NBLK = 8, path0 = 5
  test_correlated_prefetched            the same arm through dbsde_prefetch (side = true), NBLK 2, 8
  test_correlated_callers_grid          the same arm with p.t, NBLK 2, 8
  test_correlated_per_path_xi           the same arm with xi_rows = M, NBLK 2, 8
  test_diagonal_fetch_and_rollouts      fetch_diag_kernel (the last arm); rollout_draw_kernel +
                                        rollout_chain_kernel<false> (the rollout2 arm, in-step);
                                        rollout4_kernel (the PATH_ROLLOUT arm, prefetched)
  test_diagonal_per_path_xi             the rollout2 and rollout4 arms with xi_rows = M
  test_diagonal_callers_grid            rollout4_kernel with p.t
  test_diagonal_high_bit_key, _odd_shard    fetch_diag, rollout2 and rollout4 arms
  test_heston_*                         the `c->heston` arm: rollout_heston_kernel as fetch and rollout
  test_loss_pins_the_placement_of_sigma_dw  the correlated arm (NBLK 2, 8) and the rollout2 arm,
                                        followed by the whole step
  test_loss_on_the_prefetched_diagonal_rollout  rollout4_kernel, followed by the whole step

Not reached here, by design: the heston2 arm, the wide / correlated-Heston arm
(rollout_corrw_kernel and its chains) -- tests/test_gpu_heston2.py,
tests/test_gpu_heston_corr.py, tests/test_gpu_wide_state.py.

The fetch outputs t, dW and W are written by the path kernels themselves: they
are filled with NaN before the call and must be finite afterwards.  X is not:
the path kernels write the context's path buffers (xin, sdw) and the step
copies X out of xin in full, so a NaN-filled X says nothing about them.
Instead device_X dirties the path buffer before every measured rollout
(dirty_path_buffer): a device-mode step with Xi = NaN leaves NaN in every state
column of xin and sdw, and a net_u call with t = X = NaN, which involves no
path kernel, leaves NaN in the t and state columns of xin.  A row or column
group that the measured rollout skips is then NaN in X, or, in sdw and the t
column, in the loss.  No test here leaves a prefetch pending, so both the
dirtying calls and the measured rollout use path buffer 0 (pick_buffer).
The constant-1 column is 1 after every writer and cannot be dirtied: the loss
tests therefore also run as the first rollout of a new context, whose freshly
allocated path buffers hold zeros.

The sigma dW rows, the t column and the constant-1 column have no export.  The
sigma dW values are pinned through X (diag_step / heston_step return both);
their placement, and the t column, are pinned through the loss only
(test_loss_*: the correlated and two-pass arms in-step, rollout4_kernel
prefetched, the latter at D = 3 and 15 where the 1 column sits in a column
group without a live dimension), and only at M N <= 64: one misplaced row then
moves the loss by about 1 / (M N) >= 1e-2 of itself, against a tolerance of
1e-4.  A misplaced row at larger batches, and the t and 1 columns of the
Heston kernel, are beyond what this module sees.
"""
import ctypes

import numpy as np
import pytest
import torch

import path_cases as pc
from conftest import load_pkg
from oracle import philox as ph

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


_SOLVERS = {}


@pytest.fixture(scope="module", autouse=True)
def _contexts_end_with_the_module():
    yield
    _SOLVERS.clear()


def solver(pkg, dev, c, fresh=False):
    """One context per (family, size): BASKET with factor(D), DIAG, or Heston
    (Naisnet, the context of test_heston_device_mode).  fresh: a new context,
    not kept."""
    key = (c["family"], c["D"])
    if fresh or key not in _SOLVERS:
        D = pc.state_dim(c)
        if c["family"] == "heston":
            s = pkg.NativeSolver("Naisnet", pc.layers(D), "Sine", pkg.ProblemSpec(g_cols=c["D"], **pc.HESTON), pc.T, dev)
        else:
            spec = pc.BASKET if c["family"] == "corr" else pc.DIAG
            s = pkg.NativeSolver("NAIS-Net", pc.layers(D), "Sine", pkg.ProblemSpec(**spec), pc.T, dev)
            if c["family"] == "corr":
                s.set_corr(pc.factor(c["D"]))
        assert s.D == D and s.nb == c["D"]
        if fresh:
            return s
        _SOLVERS[key] = s
    return _SOLVERS[key]


def _finite(a, what):
    assert np.all(np.isfinite(a)), f"{what}: {np.count_nonzero(~np.isfinite(a))} elements were never written"
    return a


def fetch(pkg, s, dev, M, N, key, increments):
    """dbsde_brownian into NaN-filled buffers: (t [M, N+1], dW [M, N, nb] or W [M, N+1, nb])."""
    t = torch.full((M, N + 1), NAN, device=dev)
    W = torch.full((M, N if increments else N + 1, s.nb), NAN, device=dev)
    xi = torch.zeros(s.D, device=dev)
    b = pkg._lib.Batch(M, N, None, None, key["seed"], key["offset"], key["path0"], ctypes.c_void_p(xi.data_ptr()), 1)
    s._bind_stream()
    pkg._lib.check(s.lib.dbsde_brownian(s.ctx, ctypes.byref(b), ctypes.c_void_p(t.data_ptr()),
                                        ctypes.c_void_p(W.data_ptr()), int(increments)), s.ctx)
    torch.cuda.synchronize()
    return _finite(t.cpu().numpy(), "t"), _finite(W.cpu().numpy(), "dW" if increments else "W")


def dirty_path_buffer(s, dev, M, N):
    """NaN into the rows of the path buffer the next rollout of this shape
    writes (module docstring)."""
    D, R = s.D, M * (N + 1)
    par = torch.zeros(s.nparams, device=dev)
    s.loss_grad(par, M, N, torch.full((D,), NAN, device=dev), seed=77, loss=torch.empty(1, device=dev))
    bad_t, bad_X = torch.full((R,), NAN, device=dev), torch.full((R * D,), NAN, device=dev)
    s.net_u(par, bad_t, bad_X, torch.empty(R, device=dev), torch.empty(R * D, device=dev))
    torch.cuda.synchronize()


def device_X(s, dev, M, N, Xi, key, tgrid=None, prefetch=False, params=None, want_grad=False, dirty=True):
    """X [M, N+1, D] of a device-mode loss_grad (zero parameters unless given)
    after dirty_path_buffer; prefetch: the batch is rolled out by dbsde_prefetch
    and consumed by the loss_grad.  want_grad: (X, loss, grad)."""
    D = s.D
    if dirty:
        dirty_path_buffer(s, dev, M, N)
    par = torch.zeros(s.nparams, device=dev) if params is None else torch.from_numpy(params).to(dev)
    xi = torch.as_tensor(np.asarray(Xi, np.float32)).to(dev).contiguous()
    xi = xi.reshape(-1) if xi.shape[0] == 1 else xi
    X = torch.full((M * (N + 1) * D,), NAN, device=dev)
    loss = torch.full((1,), NAN, device=dev)
    grad = torch.full((s.nparams,), NAN, device=dev) if want_grad else None
    t = None if tgrid is None else torch.from_numpy(np.ascontiguousarray(tgrid)).to(dev)
    if prefetch:
        assert t is None
        s.prefetch(M, N, xi, **key)
    s.loss_grad(par, M, N, xi, t=t, grad=grad, loss=loss, X=X, **key)
    torch.cuda.synchronize()
    Xn = _finite(X.cpu().numpy(), "X").reshape(M, N + 1, D)
    assert np.isfinite(float(loss))
    if want_grad:
        return Xn, float(loss), _finite(grad.cpu().numpy(), "grad")
    return Xn


def check_corr_increments(c, dW, M=None, key=None):
    """|dW - L dz| <= corr_bound elementwise; prints and returns the worst ratio."""
    L = pc.factor(c["D"])
    dz = pc.dz_ref(c, M, key)
    ratio = float((np.abs(dW.astype(np.float64) - pc.corr_ref(L, dz)) / pc.corr_bound(L, dz)).max())
    print(f"corr D={c['D']} NBLK={pc.nblk(c['D'])} M={dW.shape[0]} N={dW.shape[1]}: max |dW - L dz| / bound = {ratio:.4f}")
    assert ratio <= 1.0, ratio
    return ratio


def check_fetch(pkg, s, dev, c, M=None, key=None):
    """The two fetch outputs of a case against the oracle; returns the device dW."""
    M, N, key = M or c["M"], c["N"], key or pc.key_of(c)
    t, dW = fetch(pkg, s, dev, M, N, key, increments=True)
    tgrid = np.broadcast_to(ph.time_grid(N, pc.T), (M, N + 1))
    np.testing.assert_array_equal(t, tgrid)
    if c["family"] == "corr":
        check_corr_increments(c, dW, M, key)
    else:
        np.testing.assert_allclose(dW, pc.dz_ref(c, M, key), rtol=pc.DW_TOL, atol=pc.DW_TOL)
    t2, W = fetch(pkg, s, dev, M, N, key, increments=False)
    np.testing.assert_array_equal(t2, tgrid)
    np.testing.assert_array_equal(W, ph.brownian_W(dW))
    return dW


# --------------------------------------------------------------------------
# correlated: rollout_corr_kernel<1..8>
# --------------------------------------------------------------------------
CORR_FULL_CASES = [c for c in pc.CORR_CASES if c["D"] in pc.CORR_FULL]


@pytest.mark.parametrize("c", pc.CORR_CASES, ids=pc.ids(pc.CORR_CASES))
def test_correlated_fetch_and_rollout(pkg, dev, c):
    s = solver(pkg, dev, c)
    dW = check_fetch(pkg, s, dev, c)
    Xi = pc.xi_shared(c)
    X = device_X(s, dev, c["M"], c["N"], Xi, pc.key_of(c))
    np.testing.assert_array_equal(X, pc.x_ref(c, Xi, dW))


@pytest.mark.parametrize("c", CORR_FULL_CASES, ids=pc.ids(CORR_FULL_CASES))
def test_correlated_prefetched(pkg, dev, c):
    s = solver(pkg, dev, c)
    Xi, key = pc.xi_shared(c), pc.key_of(c)
    X = device_X(s, dev, c["M"], c["N"], Xi, key)
    Xp = device_X(s, dev, c["M"], c["N"], Xi, key, prefetch=True)
    np.testing.assert_array_equal(Xp, X)


@pytest.mark.parametrize("c", CORR_FULL_CASES, ids=pc.ids(CORR_FULL_CASES))
def test_correlated_callers_grid(pkg, dev, c):
    s = solver(pkg, dev, c)
    Xi, key, tg = pc.xi_shared(c), pc.key_of(c), pc.caller_grid(c)
    _, dW = fetch(pkg, s, dev, c["M"], c["N"], key, increments=True)
    X = device_X(s, dev, c["M"], c["N"], Xi, key, tgrid=tg)
    np.testing.assert_array_equal(X, pc.x_ref(c, Xi, dW, tgrid=tg))


@pytest.mark.parametrize("c", CORR_FULL_CASES, ids=pc.ids(CORR_FULL_CASES))
def test_correlated_per_path_xi(pkg, dev, c):
    s = solver(pkg, dev, c)
    Xi, key = pc.xi_per_path(c), pc.key_of(c)
    assert Xi.shape == (c["M"], c["D"])
    _, dW = fetch(pkg, s, dev, c["M"], c["N"], key, increments=True)
    X = device_X(s, dev, c["M"], c["N"], Xi, key)
    np.testing.assert_array_equal(X, pc.x_ref(c, Xi, dW))


def check_high_key(pkg, dev, c):
    assert c["key"] == "high"
    s = solver(pkg, dev, c)
    dW = check_fetch(pkg, s, dev, c)
    Xi = pc.xi_shared(c)
    X = device_X(s, dev, c["M"], c["N"], Xi, pc.key_of(c))
    np.testing.assert_array_equal(X, pc.x_ref(c, Xi, dW))
    return X


def check_shard(pkg, dev, c, prefetch=False):
    """The odd-path0 shard of a case against rows path0 .. path0 + M of the
    full batch (itself checked against the oracle): dW and X bit for bit."""
    assert c["key"] == "shard"
    s = solver(pkg, dev, c)
    M, N, Mf, p0 = c["M"], c["N"], c["full_M"], pc.SHARD_PATH0
    full = check_fetch(pkg, s, dev, c, M=Mf, key=pc.KEY0)
    _, part = fetch(pkg, s, dev, M, N, pc.key_of(c), increments=True)
    np.testing.assert_array_equal(part, full[p0:p0 + M])
    Xi = pc.xi_shared(c)
    Xf = device_X(s, dev, Mf, N, Xi, pc.KEY0, prefetch=prefetch)
    np.testing.assert_array_equal(Xf, pc.x_ref(c, Xi, full))
    Xs = device_X(s, dev, M, N, Xi, pc.key_of(c), prefetch=prefetch)
    np.testing.assert_array_equal(Xs, Xf[p0:p0 + M])


def test_correlated_high_bit_key(pkg, dev):
    check_high_key(pkg, dev, pc.CORR_KEY_CASES[0])


def test_correlated_odd_shard(pkg, dev):
    check_shard(pkg, dev, pc.CORR_KEY_CASES[1])


# --------------------------------------------------------------------------
# diagonal: fetch_diag_kernel, rollout_draw_kernel + rollout_chain_kernel, rollout4_kernel
# --------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.DIAG_CASES, ids=pc.ids(pc.DIAG_CASES))
def test_diagonal_fetch_and_rollouts(pkg, dev, c):
    s = solver(pkg, dev, c)
    dW = check_fetch(pkg, s, dev, c)
    Xi = pc.xi_shared(c)
    ref = pc.x_ref(c, Xi, dW)
    np.testing.assert_array_equal(device_X(s, dev, c["M"], c["N"], Xi, pc.key_of(c)), ref)                  # two-pass
    np.testing.assert_array_equal(device_X(s, dev, c["M"], c["N"], Xi, pc.key_of(c), prefetch=True), ref)   # rollout4


def test_diagonal_per_path_xi(pkg, dev):
    c = pc.DIAG_XI_CASE
    s = solver(pkg, dev, c)
    Xi, key = pc.xi_per_path(c), pc.key_of(c)
    _, dW = fetch(pkg, s, dev, c["M"], c["N"], key, increments=True)
    ref = pc.x_ref(c, Xi, dW)
    np.testing.assert_array_equal(device_X(s, dev, c["M"], c["N"], Xi, key), ref)
    np.testing.assert_array_equal(device_X(s, dev, c["M"], c["N"], Xi, key, prefetch=True), ref)


def test_diagonal_callers_grid(pkg, dev):
    c = pc.DIAG_GRID_CASE
    s = solver(pkg, dev, c)
    Xi, key, tg = pc.xi_shared(c), pc.key_of(c), pc.caller_grid(c)
    _, dW = fetch(pkg, s, dev, c["M"], c["N"], key, increments=True)
    X = device_X(s, dev, c["M"], c["N"], Xi, key, tgrid=tg)
    np.testing.assert_array_equal(X, pc.x_ref(c, Xi, dW, tgrid=tg))


def test_diagonal_high_bit_key(pkg, dev):
    c = pc.DIAG_KEY_CASES[0]
    X = check_high_key(pkg, dev, c)
    Xp = device_X(solver(pkg, dev, c), dev, c["M"], c["N"], pc.xi_shared(c), pc.key_of(c), prefetch=True)
    np.testing.assert_array_equal(Xp, X)


@pytest.mark.parametrize("prefetch", [False, True], ids=["in_step", "prefetched"])
def test_diagonal_odd_shard(pkg, dev, prefetch):
    check_shard(pkg, dev, pc.DIAG_KEY_CASES[1], prefetch=prefetch)


# --------------------------------------------------------------------------
# plain Heston: rollout_heston_kernel
# --------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.HESTON_CASES, ids=pc.ids(pc.HESTON_CASES))
def test_heston_fetch_and_rollout(pkg, dev, c):
    s = solver(pkg, dev, c)
    dW = check_fetch(pkg, s, dev, c)
    Xi = pc.xi_shared(c)
    X = device_X(s, dev, c["M"], c["N"], Xi, pc.key_of(c))
    np.testing.assert_array_equal(X, pc.x_ref(c, Xi, dW))


def test_heston_per_path_xi(pkg, dev):
    c = pc.HESTON_XI_CASE
    s = solver(pkg, dev, c)
    Xi, key = pc.xi_per_path(c), pc.key_of(c)
    assert Xi.shape == (c["M"], 2 * c["D"])
    _, dW = fetch(pkg, s, dev, c["M"], c["N"], key, increments=True)
    X = device_X(s, dev, c["M"], c["N"], Xi, key)
    np.testing.assert_array_equal(X, pc.x_ref(c, Xi, dW))


def test_heston_high_bit_key(pkg, dev):
    check_high_key(pkg, dev, pc.HESTON_KEY_CASES[0])


def test_heston_odd_shard(pkg, dev):
    check_shard(pkg, dev, pc.HESTON_KEY_CASES[1])


# --------------------------------------------------------------------------
# placement of the sigma dW rows
# --------------------------------------------------------------------------
def check_loss(pkg, dev, c, prefetch, buffers):
    """Device-mode loss and gradient at non-zero parameters against the oracle
    on the fetched (t, W): loss rel 1e-4, gradient abs 2e-4 max|grad| (the
    parity suite's).  tests/test_path_cases_cpu.py holds the oracle's own
    sensitivity to the rounding of W to a tenth of that.  buffers: "dirtied"
    (NaN in the t, state and sigma dW columns) or "fresh" (the rollout is the
    first of a new context, whose path buffers hold zeros: the constant-1
    column)."""
    fresh = buffers == "fresh"
    s = solver(pkg, dev, c, fresh=fresh)
    M, N, key = c["M"], c["N"], pc.key_of(c)
    _, params = pc.loss_model(c)
    assert params.size == s.nparams
    t, W = fetch(pkg, s, dev, M, N, key, increments=False)
    _, dW = fetch(pkg, s, dev, M, N, key, increments=True)
    ref = pc.loss_reference(c, t, W)
    Xi = pc.xi_shared(c)
    X, loss, grad = device_X(s, dev, M, N, Xi, key, params=params, want_grad=True, prefetch=prefetch, dirty=not fresh)
    np.testing.assert_array_equal(X, pc.x_ref(c, Xi, dW))
    el = abs(loss - ref["loss"]) / abs(ref["loss"])
    eg = np.abs(grad - ref["grad"])[ref["used"]].max() / np.abs(ref["grad"]).max()
    print(f"{c['id']}: loss {loss:.6g} (oracle {ref['loss']:.6g}), rel {el:.3g}; grad err {eg:.3g} of max|grad|")
    assert np.all(grad[~ref["used"]] == 0)
    assert el <= pc.LOSS_RTOL, el
    assert eg <= pc.GRAD_ATOL, eg


BUFFERS = ["dirtied", "fresh"]


@pytest.mark.parametrize("buffers", BUFFERS)
@pytest.mark.parametrize("c", pc.LOSS_CASES, ids=pc.ids(pc.LOSS_CASES))
def test_loss_pins_the_placement_of_sigma_dw(pkg, dev, c, buffers):
    check_loss(pkg, dev, c, False, buffers)


DIAG_LOSS_CASES = [c for c in pc.LOSS_CASES if c["family"] == "diag"]


@pytest.mark.parametrize("buffers", BUFFERS)
@pytest.mark.parametrize("c", DIAG_LOSS_CASES, ids=pc.ids(DIAG_LOSS_CASES))
def test_loss_on_the_prefetched_diagonal_rollout(pkg, dev, c, buffers):
    """rollout4_kernel's sigma dW rows, t column and constant-1 column."""
    check_loss(pkg, dev, c, True, buffers)
