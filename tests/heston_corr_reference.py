"""References for the correlated k-asset Heston (a Cholesky factor L [k, k]
between the assets' Brownian motions, dbsde_set_corr on a Heston context) --
test infrastructure only.  Everything here composes existing pieces:

  * random_factor: the factor recipe of tests/test_gpu_wide_state.py
    (test_correlated_device_mode_wide);
  * pde_terms: the seven PDE terms with the diffusion columns of Sigma(x) . L,
    as jet_reference.heston_coefficients -> A @ L -> directions ->
    jets(clamp=True) -> _contract (L = None: jet_reference.heston_pde_terms);
  * pde_setup: the CPU half of tests/test_gpu_jet.py's heston_setup (oracle
    weights fixed by the seed alone, output bias moved to the median raw
    output so that about half of the rows clamp), and object_factor, the
    factor a HestonFBSNN(correlation_type="random_correlation") constructed
    right after np.random.seed(seed) holds;
  * the shapes and seeds the loss-and-gradient test runs, shared with the CPU
    test that holds the reference to its own condition on them.
"""
from __future__ import annotations

import numpy as np
import torch

import jet_reference as jr
from oracle import fbsnn_ref as fr
from oracle import philox as ph

T = 1.0
N = 10
HESTON = dict(kappa=2.0, theta=0.2, sigma=0.3, rho=0.8)

# loss-and-gradient cases: name -> (k, hidden width, M, seed).  The variance
# starts at 0.2 and often crosses the sqrt(max(v, 1e-8)) kink, where the two CPU
# references (stepping on dW, and on the fp32 differences of W) part by more
# than the X tolerance for some draws (2 to 5 times the bound at a quarter of
# the seeds 1..60 for k = 50 and k = 130).  The seeds below are the ones of
# that scan, made on the references alone, at which they agree best (0.03 to
# 0.37 of the bound; tests/test_heston_corr_cpu.py holds them to it).
LOSS_CASES = {
    "k3_m24": (3, 16, 24, 11),
    "k3_m7": (3, 16, 7, 11),
    "k50_w110": (50, 110, 24, 34),      # the fused form, Dp = 112
    "k130_wide": (130, 16, 16, 8),      # the wide chain
}
PDE_K, PDE_SEED, PDE_R = 3, 42, 48


def random_factor(k, seed=None):
    """Cholesky factor [k, k] (float64) of a random correlation matrix."""
    rs = np.random.RandomState(k if seed is None else seed)
    A = rs.normal(size=(k, k))
    C = A @ A.T + k * np.eye(k)
    d = np.sqrt(np.diag(C))
    return np.linalg.cholesky(C / np.outer(d, d))


def xi_state(k, v0=0.2):
    """[S_1..S_k, v_1..v_k] = [1.., v0..] as one row."""
    return np.concatenate([np.ones((1, k)), np.full((1, k), v0)], 1)


def pde_terms(model, t, X, k, L=None, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8, phi_r=0.05):
    """The seven terms [R, 1] (numpy) of the Heston PDE whose assets' Brownian
    motions are correlated by L (None: independent), in the dtype of t / X."""
    tt, Xt = torch.as_tensor(t), torch.as_tensor(X)
    u, du = fr.heston_net_u(model, tt, Xt.clone().requires_grad_(True))
    u, du = u.detach().numpy(), du.detach().numpy()
    mu, A = jr.heston_coefficients(X, k, kappa, theta, sigma, rho)
    if L is not None:
        A = torch.matmul(A, torch.as_tensor(np.asarray(L), dtype=A.dtype))
    d1, d2 = jr.jets(model, t, X, jr.directions(A), clamp=True)
    return jr._contract(u, du, mu.numpy(), phi_r * u, d1, d2)


def pde_setup(k=PDE_K, seed=PDE_SEED, R=PDE_R):
    """(oracle model, flat params, t [R, 1], X [R, 2k], clamped [R]): the recipe
    of tests/test_gpu_jet.py's heston_setup without the device object."""
    layers, act = [2] + 4 * [16] + [1], "Tanh"
    torch.manual_seed(seed)
    oracle = fr.build_heston_model("Naisnet", layers, act, k)
    rs = np.random.RandomState(5)
    t = rs.uniform(0.0, 1.0, (R, 1)).astype(np.float32)
    X = np.concatenate([1.0 + 0.3 * rs.normal(size=(R, k)), 0.2 + 0.05 * rs.uniform(size=(R, k))], 1).astype(np.float32)
    flat = fr.flat_params(oracle).astype(np.float32)
    z = torch.cat([torch.from_numpy(t), torch.from_numpy(X)], 1)
    with torch.no_grad():
        raw = oracle(z).numpy().ravel()
    flat[-1] -= np.float32(np.median(raw))       # the output bias is the last parameter
    fr.set_flat_params(oracle, flat)
    with torch.no_grad():
        raw = oracle(z).numpy().ravel()
    clamped = raw < 0
    assert 0.25 * R < int(clamped.sum()) < 0.75 * R, int(clamped.sum())
    assert float(np.abs(raw).min()) > 1e-4, float(np.abs(raw).min())   # the reference alone decides every mask
    return oracle, flat, t, X, clamped


def object_factor(pkg, k=PDE_K, seed=PDE_SEED):
    """The Cholesky factor of FBSNN.generate_correlation_matrix(k) drawn right
    after np.random.seed(seed) ("random_correlation")."""
    obj = object.__new__(pkg.HestonFBSNN)
    obj.correlation_type = "random_correlation"
    np.random.seed(seed)
    return np.linalg.cholesky(obj.generate_correlation_matrix(k))


def loss_case_model(case):
    """(layers of the native solver, oracle model, flat params) of a loss case."""
    k, width, _, _ = LOSS_CASES[case]
    torch.manual_seed(k + width)
    model = fr.build_heston_model("Naisnet", [2] + 4 * [width] + [1], "Sine", k)
    return [1 + 2 * k] + 4 * [width] + [1], model, fr.flat_params(model)


def oracle_increments(case, L):
    """The device-mode increments of a loss case as the oracle draws them."""
    k, _, M, seed = LOSS_CASES[case]
    return ph.increments(seed, 0, 0, M, N, k, T, L=np.asarray(L, np.float32))
