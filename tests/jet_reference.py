"""Torch-CPU reference of dbsde_net_u_jet and dbsde_pde_residual (csrc/jet.hip,
include/dbsde.h) -- test infrastructure only.

Jets: the oracle model (oracle/fbsnn_ref.py) is evaluated on z + s v with s a
[R, nd, 1] zero tensor that requires grad; d1 = grad(sum y, s) with
create_graph and d2 = grad(sum d1, s) are the first and second directional
derivatives along v at every (point, direction) row, each row on its own.

PDE terms: u, Du by the oracle's net_u, the coefficients by
oracle.fbsnn_ref.Problem.mu / sigma / phi (Heston: restated here in torch from
the formulas of include/dbsde.h), the diffusion columns a_j = column j of
sigma . L, and

  u_t = d1 along e_t        drift = mu . Du        diffusion = 1/2 sum_j d2(a_j)
  residual = u_t + drift + diffusion - phi
  scale = |u_t| + |drift| + 1/2 sum_j |d2(a_j)| + |phi|
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import fbsnn_ref as ref

TERMS = ("u", "u_t", "drift", "diffusion", "phi", "residual", "scale")


def jets(model, t, X, V, clamp=False):
    """d1, d2 [R, nd] (numpy) of the oracle model along V [R, nd, D+1] at the
    points (t [R, 1], X [R, D]); clamp: of max(model, 0) (heston_net_u)."""
    z = torch.cat((torch.as_tensor(t), torch.as_tensor(X)), 1)
    V = torch.as_tensor(V)
    R, nd, n = V.shape
    assert z.shape == (R, n)
    s = torch.zeros((R, nd, 1), dtype=z.dtype, requires_grad=True)
    y = model((z[:, None, :] + s * V).reshape(R * nd, n))
    if clamp:
        y = torch.clamp(y, min=0.0)
    d1 = torch.autograd.grad(y.sum(), s, create_graph=True)[0]
    d2 = torch.autograd.grad(d1.sum(), s, allow_unused=True)[0] if d1.requires_grad else None
    if d2 is None:
        d2 = torch.zeros_like(d1)
    return d1.detach().reshape(R, nd).numpy(), d2.detach().reshape(R, nd).numpy()


def theta(model, t, X, clamp=False):
    """autograd.grad(u, t) [R, 1] of the oracle model."""
    tt = torch.as_tensor(t).clone().requires_grad_(True)
    u = model(torch.cat((tt, torch.as_tensor(X)), 1))
    if clamp:
        u = torch.clamp(u, min=0.0)
    return torch.autograd.grad(u.sum(), tt)[0].numpy()


def heston_coefficients(X, k, kappa, theta_, sigma, rho, mu_a=0.05):
    """mu [R, 2k] and the diffusion columns A [R, 2k, k] of include/dbsde.h's
    kind HESTON: column i = Sigma_i . (1, 1)^T in the (S_i, v_i) plane."""
    X = torch.as_tensor(X)
    S, v = X[:, :k], X[:, k:]
    mu = torch.cat([mu_a * S, kappa * (theta_ - v)], 1).clamp(-100, 100)
    sv = torch.sqrt(torch.clamp(v, min=1e-8))
    a_s = (sv * S).clamp(-100, 100) + (rho * (sigma * sv)).clamp(-100, 100)
    a_v = (rho * (sv * S)).clamp(-100, 100) + (sigma * sv).clamp(-100, 100)
    A = torch.zeros((X.shape[0], 2 * k, k), dtype=X.dtype)
    for i in range(k):
        A[:, i, i] = a_s[:, i]
        A[:, k + i, i] = a_v[:, i]
    return mu, A


def directions(A):
    """V [R, 1 + nb, D + 1]: e_t, then the columns of A [R, D, nb]."""
    R, D, nb = A.shape
    V = torch.zeros((R, 1 + nb, D + 1), dtype=A.dtype)
    V[:, 0, 0] = 1.0
    V[:, 1:, 1:] = A.transpose(1, 2)
    return V


def _contract(u, du, mu, phi, d1, d2):
    u_t = d1[:, :1]
    drift = np.sum(mu * du, axis=1, keepdims=True)
    diffusion = 0.5 * np.sum(d2[:, 1:], axis=1, keepdims=True)
    scale = np.abs(u_t) + np.abs(drift) + 0.5 * np.sum(np.abs(d2[:, 1:]), axis=1, keepdims=True) + np.abs(phi)
    return dict(u=u, u_t=u_t, drift=drift, diffusion=diffusion, phi=phi,
                residual=u_t + drift + diffusion - phi, scale=scale)


def pde_terms(model, problem, t, X, L=None):
    """The seven terms [R, 1] (numpy) for an oracle.fbsnn_ref.Problem."""
    tt, Xt = torch.as_tensor(t), torch.as_tensor(X)
    u, du = ref.net_u(model, tt, Xt.clone().requires_grad_(True))
    u, du = u.detach(), du.detach()
    A = problem.sigma(tt, Xt, u)
    if L is not None:
        A = torch.matmul(A, torch.as_tensor(np.asarray(L), dtype=A.dtype))
    d1, d2 = jets(model, t, X, directions(A))
    mu = problem.mu(tt, Xt, u, du).numpy()
    phi = problem.phi(tt, Xt, u, du).numpy()
    return _contract(u.numpy(), du.numpy(), mu, phi, d1, d2)


def heston_pde_terms(model, t, X, k, kappa, theta_, sigma, rho, phi_r=0.05):
    """The same for the Heston problem (u = max(net, 0), phi = phi_r u)."""
    tt, Xt = torch.as_tensor(t), torch.as_tensor(X)
    u, du = ref.heston_net_u(model, tt, Xt.clone().requires_grad_(True))
    u, du = u.detach().numpy(), du.detach().numpy()
    mu, A = heston_coefficients(X, k, kappa, theta_, sigma, rho)
    d1, d2 = jets(model, t, X, directions(A), clamp=True)
    return _contract(u, du, mu.numpy(), phi_r * u, d1, d2)
