"""The references of tests/test_gpu_heston_corr.py held to their own conditions
(tests/heston_corr_reference.py, oracle/philox.py, oracle/fbsnn_ref.py).  CPU
only: no device code runs here."""
import numpy as np
import pytest
import torch

import heston_corr_reference as hc
import jet_reference as jr
from conftest import load_pkg
from oracle import fbsnn_ref as fr
from oracle import philox as ph


def test_pde_helper_diffusion_is_the_trace_formula():
    """k = 2, fp64: the helper's diffusion term is 1/2 tr(A L L^T A^T H), H the
    Hessian of u = max(net, 0) in x by explicit double autograd."""
    k, R = 2, 12
    torch.manual_seed(1)
    model = fr.build_heston_model("Naisnet", [2] + 4 * [16] + [1], "Tanh", k).double()
    rs = np.random.RandomState(2)
    t = rs.uniform(0.0, 1.0, (R, 1))
    X = np.concatenate([1.0 + 0.3 * rs.normal(size=(R, k)), 0.2 + 0.05 * rs.uniform(size=(R, k))], 1)
    with torch.no_grad():
        raw = model(torch.cat([torch.from_numpy(t), torch.from_numpy(X)], 1)).numpy().ravel()
    # an output bias that leaves both clamped and open rows
    flat = fr.flat_params(model)
    flat[-1] -= np.median(raw)
    fr.set_flat_params(model, flat)
    model = model.double()
    L = hc.random_factor(k)
    assert abs(L[1, 0]) > 0.05
    got = hc.pde_terms(model, t, X, k, L=L, **hc.HESTON)["diffusion"]
    h = hc.HESTON
    _, A = jr.heston_coefficients(X, k, h["kappa"], h["theta"], h["sigma"], h["rho"])
    A = A.numpy()
    want = np.empty((R, 1))
    n_open = 0
    for r in range(R):
        tr = torch.from_numpy(t[r])

        def u_of(x):
            return torch.clamp(model(torch.cat((tr, x))[None, :]), min=0.0).sum()

        H = torch.autograd.functional.hessian(u_of, torch.from_numpy(X[r])).numpy()
        n_open += int(np.abs(H).max() > 0)
        B = A[r] @ L                       # [2k, k]: the diffusion matrix Sigma(x) L
        want[r, 0] = 0.5 * np.trace(B @ B.T @ H)
    assert 0 < n_open < R                  # both clamped and open rows
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("case", list(hc.LOSS_CASES))
def test_x_tolerance_condition_of_the_loss_reference(case):
    """The loss-and-gradient test reads the device's X (stepped on dW) against
    the X of fr.heston_loss_function (stepped on the fp32 differences of W =
    fp32(fp64 cumsum of dW), torch's sqrt) within rtol 1e-5 / atol 1e-6.  That
    has to hold between the two references themselves, at its inputs."""
    k, _, M, _ = hc.LOSS_CASES[case]
    L = hc.random_factor(k)
    dW = hc.oracle_increments(case, L)
    Xr, _ = ph.heston_rollout(hc.xi_state(k), dW, hc.T)
    torch.manual_seed(0)
    model = fr.build_heston_model("Naisnet", [2, 16, 16, 16, 16, 1], "Sine", k)   # X does not depend on it
    t = torch.from_numpy(np.broadcast_to(ph.time_grid(hc.N, hc.T), (M, hc.N + 1)).copy())[..., None]
    W = torch.from_numpy(ph.brownian_W(dW))
    xi = torch.ones((1, k), requires_grad=True)     # the reference's Xi, as fr.heston_loss_and_grads passes it
    _, X, _, _ = fr.heston_loss_function(model, fr.Heston(k=k), t, W, xi, M)
    X = X.detach().numpy()
    err = np.abs(X - Xr)
    print(f"{case}: max|X - X'| = {err.max():.3e}, max over entries of err / (1e-6 + 1e-5 |X|) = "
          f"{(err / (1e-6 + 1e-5 * np.abs(Xr))).max():.3f}")
    np.testing.assert_allclose(X, Xr, rtol=1e-5, atol=1e-6)


def test_independent_diffusion_differs_at_the_pde_test_points():
    """Without L the diffusion term is off by more than ten times the PDE
    test's tolerance (2e-4 max|term|): that test cannot pass on a kernel that
    ignores the factor."""
    oracle, _, t, X, clamped = hc.pde_setup()
    L = hc.object_factor(load_pkg())
    assert L.shape == (hc.PDE_K, hc.PDE_K) and np.abs(np.tril(L, -1)).max() > 0
    corr = hc.pde_terms(oracle, t, X, hc.PDE_K, L=L, **hc.HESTON)
    ind = hc.pde_terms(oracle, t, X, hc.PDE_K, L=None, **hc.HESTON)
    want = jr.heston_pde_terms(oracle, t, X, hc.PDE_K, hc.HESTON["kappa"], hc.HESTON["theta"], hc.HESTON["sigma"],
                               hc.HESTON["rho"])
    for key in jr.TERMS:                   # L = None is the existing reference
        np.testing.assert_array_equal(ind[key], want[key])
    tol = 2e-4 * float(np.abs(corr["diffusion"]).max())
    gap = float(np.abs(ind["diffusion"] - corr["diffusion"]).max())
    print(f"max|diffusion(I) - diffusion(L)| = {gap:.3e} = {gap / tol:.1f} x the tolerance {tol:.3e}")
    assert gap > 10 * tol
    assert np.all(corr["diffusion"][clamped] == 0)
