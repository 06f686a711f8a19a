"""The path kernels (csrc/paths.hpp, dispatched by launch_paths in
csrc/rollout.hip) at ragged shapes -- test infrastructure only: the case table
of tests/test_gpu_path_kernels.py and the reference helpers it shares with
tests/test_path_cases_cpu.py.  numpy and oracle/philox.py; torch and
oracle/fbsnn_ref.py are imported only inside the loss helpers.

Shapes (M, N): SHAPES.  N mod 4 covers 0, 1, 2, 3 (a Philox block holds 4
steps) and N sits below, at and above RC_AHEAD = 8 (the Euler chains load 8
steps ahead); M sits below, at, just above and at two-plus 16-path groups (the
correlated kernel's workgroup, and M D around the 256-thread workgroups of the
others).

Families:
  corr    rollout_corr_kernel<NBLK>, NBLK = ceil(D / 16) = 1..8, BASKET spec,
          dense factor(D).  CORR_D holds both sides of every block edge and the
          two sizes D = 127, 128 whose context is wide (Dp = 144) while
          nb <= 128 still selects this kernel.  D in CORR_FULL run every
          shape, the others one shape each, rotating through SHAPES.
  diag    fetch_diag_kernel, rollout_draw_kernel + rollout_chain_kernel
          (in-step), rollout4_kernel (prefetched, or a caller's grid), DIAG spec
          (mu_a, sig_a and sig_b all non-zero).  D = 3, 7, 11-style sizes put
          the constant-1 column into a column group without a live dimension;
          D = 14 gives Dp = 16, D = 15 gives Dp = 32.
  heston  rollout_heston_kernel (no factor), the spec of
          tests/test_gpu_device_rng.py test_heston_device_mode; M k is never a
          multiple of 256.

Keys: KEY0, and per family one case at high_key(M) (seed, offset and path0 all
need their upper bits) and one odd path0 = 5 shard of a larger batch.

corr_bound(L, dz) is the elementwise bound on |dW - L dz| of a correlated
increment, for any summation order:

    sum_j |L_ij| (2e-6 |dz_j| + 2e-6)  +  (nb + 2) 2^-24 sum_j |L_ij dz_j|

The first term is the Box-Muller tolerance of the uncorrelated increments
(rtol = atol = 2e-6 against oracle/philox.py, tests/test_gpu_device_rng.py)
pushed through L; the second is the gamma_n bound of an fp32 sum of nb
products plus the final rounding (Higham, Accuracy and Stability of Numerical
Algorithms, section 3.1).  Nothing in it is measured.

Loss cases (LOSS_CASES): M N <= 64, so that one misplaced sigma dW row moves
the loss by about 1 / (M N) >= 1e-2 of itself, far above the parity
tolerance LOSS_RTOL = 1e-4.
"""
from __future__ import annotations

import numpy as np

from oracle import philox as ph

T = 1.0
SHAPES = [(1, 1), (15, 2), (17, 3), (33, 4), (16, 7), (40, 9), (3, 13), (18, 8)]

BASKET = dict(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=0.0, g="call_mean", strike=1.0)
DIAG = dict(mu_a=0.05, sig_a=0.2, sig_b=0.1, phi_r=0.05, g="sumsq")
HESTON = dict(kind="heston", mu_a=0.05, phi_r=0.05, g="call_mean", strike=1.0, u_clamp=True, q3=False, kappa=2.0,
              theta=0.2, sigma=0.3, rho=0.8)   # + g_cols = k

KEY0 = dict(seed=9, offset=0, path0=0)
SHARD_PATH0 = 5
DW_TOL = 2e-6                       # Box-Muller: rtol = atol on the uncorrelated increments
LOSS_RTOL, GRAD_ATOL = 1e-4, 2e-4   # tests/test_gpu_parity.py: loss rel, gradient abs / max|grad|


def high_key(M):
    """Every key word needs its upper half: key = (seed ^ (offset >> 32), seed >> 32),
    counter words path0 + m (just below 2^32) and offset & 0xffffffff."""
    return dict(seed=2 ** 40 + 5, offset=2 ** 33 + 7, path0=2 ** 32 - M - 3)


def nblk(D):
    return (D + 15) // 16


def layers(D):
    return [D + 1, 16, 16, 16, 16, 1]


def _case(family, D, M, N, key="default", full_M=None, tag=""):
    c = dict(family=family, D=D, M=M, N=N, key=key, full_M=full_M)
    c["id"] = f"{family}{D}_M{M}_N{N}" + ("" if key == "default" else "_" + key) + tag
    return c


# --------------------------------------------------------------------------
# the table
# --------------------------------------------------------------------------
CORR_D = [1, 3, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 126, 127, 128]
CORR_FULL = [17, 113, 128]
DIAG_D = [1, 2, 3, 7, 13, 14, 15, 126]
HESTON_K = [1, 2, 7, 33]


def _corr_cases():
    out = [_case("corr", D, M, N) for D in CORR_FULL for M, N in SHAPES]
    rest = [D for D in CORR_D if D not in CORR_FULL]
    out += [_case("corr", D, *SHAPES[i % len(SHAPES)]) for i, D in enumerate(rest)]
    return out


CORR_CASES = _corr_cases()
# high-bit key: NBLK = 8 in a wide context, three 16-path groups, N = 4 q + 1;
# shard: paths 5 .. 22 of the 40-path batch (both 16-path group edges inside)
CORR_KEY_CASES = [_case("corr", 128, 40, 9, key="high"), _case("corr", 113, 18, 9, key="shard", full_M=40)]

DIAG_CASES = [_case("diag", D, *SHAPES[i]) for i, D in enumerate(DIAG_D)]
DIAG_KEY_CASES = [_case("diag", 7, 33, 4, key="high"), _case("diag", 13, 18, 9, key="shard", full_M=40)]
DIAG_XI_CASE = _case("diag", 3, 33, 4, tag="_xi")       # per-path Xi [M, D]
DIAG_GRID_CASE = _case("diag", 15, 18, 8, tag="_grid")    # a caller's time grid

# k = 1, 2, 7, 33 rotate through SHAPES from its second entry
HESTON_CASES = [_case("heston", k, *SHAPES[1 + i]) for i, k in enumerate(HESTON_K)]
HESTON_KEY_CASES = [_case("heston", 7, 40, 9, key="high"), _case("heston", 33, 11, 8, key="shard", full_M=18)]
HESTON_XI_CASE = _case("heston", 2, 3, 13, tag="_xi")   # per-path Xi [M, 2 k]

# placement of the sigma dW rows, through the loss: M N <= 64
LOSS_CASES = [_case("corr", 17, 17, 3), _case("corr", 113, 15, 2), _case("corr", 128, 3, 13),
              _case("diag", 3, 15, 2), _case("diag", 15, 17, 3)]
# seed of each loss case's parameters (tests/test_path_cases_cpu.py holds every
# case to the sensitivity condition; a case that fails it gets another seed)
LOSS_SEED = {c["id"]: 1000 + c["D"] for c in LOSS_CASES}

FAMILIES = {
    "corr": CORR_CASES + CORR_KEY_CASES,
    "diag": DIAG_CASES + DIAG_KEY_CASES + [DIAG_XI_CASE, DIAG_GRID_CASE],
    "heston": HESTON_CASES + HESTON_KEY_CASES + [HESTON_XI_CASE],
}


def ids(cases):
    return [c["id"] for c in cases]


def key_of(c):
    """The batch key (seed, offset, path0) of a case."""
    if c["key"] == "high":
        return high_key(c["M"])
    if c["key"] == "shard":
        return dict(KEY0, path0=SHARD_PATH0)
    return dict(KEY0)


def state_dim(c):
    return 2 * c["D"] if c["family"] == "heston" else c["D"]


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
_FACTORS = {}


def factor(D):
    """fp32 Cholesky factor of 0.3 11^T + 0.5 I + 0.2 corrcoef(normal(D, 3 D)),
    seeded by D: dense, no entry of the lower triangle is zero."""
    if D not in _FACTORS:
        rs = np.random.RandomState(D)
        C = 0.3 * np.ones((D, D)) + 0.5 * np.eye(D) + 0.2 * np.atleast_2d(np.corrcoef(rs.normal(size=(D, 3 * D))))
        L = np.linalg.cholesky(C).astype(np.float32)
        L.setflags(write=False)
        _FACTORS[D] = L
    return _FACTORS[D]


def xi_shared(c):
    """Xi [1, D]: 1.0 / 0.5 alternating, so that a swapped column shows.
    Heston: S alternates 1.0 / 0.5, v alternates 0.2 / 0.1."""
    k = c["D"]
    a = np.where(np.arange(k) % 2 == 0, 1.0, 0.5)
    if c["family"] == "heston":
        return np.concatenate([a, 0.2 * a])[None, :].astype(np.float32)
    return a[None, :].astype(np.float32)


def xi_per_path(c):
    """Xi [M, D] from uniform(0.5, 1.5) (Heston: v from uniform(0.1, 0.3))."""
    rs = np.random.RandomState(7 * c["D"] + c["M"])
    k = c["D"]
    x = rs.uniform(0.5, 1.5, size=(c["M"], k))
    if c["family"] == "heston":
        x = np.concatenate([x, rs.uniform(0.1, 0.3, size=(c["M"], k))], 1)
    return x.astype(np.float32)


def caller_grid(c):
    """A per-path non-uniform grid [M, N+1] (tests/test_gpu_round3.py
    test_correlated_device_batch_on_an_explicit_time_grid)."""
    rs = np.random.RandomState(11 * c["D"] + c["N"])
    tg = np.sort(rs.uniform(0, 1, size=(c["M"], c["N"] + 1)), 1).astype(np.float32)
    tg[:, 0] = 0.0
    return tg


# --------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------
def dz_ref(c, M=None, key=None):
    """The uncorrelated oracle increments sqrt(dt) z [M, N, nb] of a case."""
    k = key or key_of(c)
    return ph.increments(k["seed"], k["offset"], k["path0"], M or c["M"], c["N"], c["D"], T)


def corr_ref(L, dz):
    """L dz in fp64 (not rounded)."""
    return np.einsum("ij,mnj->mni", np.asarray(L, np.float64), np.asarray(dz, np.float64))


def corr_bound(L, dz):
    """Elementwise bound [M, N, nb] on |dW - corr_ref(L, dz)| (module docstring)."""
    A = np.abs(np.asarray(L, np.float64))
    z = np.abs(np.asarray(dz, np.float64))
    nb = A.shape[0]
    draw = np.einsum("ij,mnj->mni", A, DW_TOL * z + DW_TOL)
    summ = (nb + 2) * 2.0 ** -24 * np.einsum("ij,mnj->mni", A, z)
    return draw + summ


def corr_fp32(L, dz, descending=False):
    """L dz accumulated in fp32, one rounded product and one rounded sum per j,
    j ascending or descending."""
    L = np.asarray(L, np.float32)
    dz = np.asarray(dz, np.float32)
    acc = np.zeros(dz.shape[:2] + (L.shape[0],), np.float32)
    js = range(L.shape[1])
    for j in (reversed(js) if descending else js):
        acc = acc + L[:, j][None, None, :] * dz[:, :, j][:, :, None]
    return acc


def x_ref(c, Xi, dW, tgrid=None):
    """The oracle rollout of the device increments dW of a case."""
    if c["family"] == "heston":
        return ph.heston_rollout(Xi, dW, T, HESTON["mu_a"], HESTON["kappa"], HESTON["theta"], HESTON["sigma"],
                                 HESTON["rho"], tgrid=tgrid)[0]
    spec = BASKET if c["family"] == "corr" else DIAG
    return ph.rollout(Xi, dW, T, spec["mu_a"], spec["sig_a"], spec.get("sig_b", 0.0), tgrid=tgrid)


# --------------------------------------------------------------------------
# the loss cases
# --------------------------------------------------------------------------
class _DiagProblem:
    """DIAG in the form oracle/fbsnn_ref.py loss_function reads: mu = mu_a X,
    sigma = diag(sig_a X + sig_b), phi = phi_r Y, g = sum X^2."""

    def mu(self, t, X, Y, Z):
        return DIAG["mu_a"] * X

    def sigma(self, t, X, Y):
        import torch
        return torch.diag_embed(DIAG["sig_a"] * X + DIAG["sig_b"])

    def phi(self, t, X, Y, Z):
        return DIAG["phi_r"] * (Y)

    def g(self, X):
        import torch
        return torch.sum(X ** 2, 1, keepdim=True)


def loss_problem(c):
    from oracle import fbsnn_ref as fr
    return fr.make_problem("basket", c["D"]) if c["family"] == "corr" else _DiagProblem()


def loss_model(c):
    """The oracle NAIS-Net of a loss case with its parameters normal(0, 0.3),
    seeded per case; returns (model, flat fp32 parameters)."""
    import torch
    from oracle import fbsnn_ref as fr
    torch.manual_seed(0)
    model = fr.build_model("NAIS-Net", layers(c["D"]), "Sine")
    n = sum(p.numel() for p in model.state_dict().values())
    params = np.random.RandomState(LOSS_SEED[c["id"]]).normal(0.0, 0.3, size=n).astype(np.float32)
    fr.set_flat_params(model, params)
    return model, params


def loss_reference(c, t, W, double=False):
    """fbsnn_ref.loss_and_grads of a loss case on (t [M, N+1], W [M, N+1, D]),
    in fp32, or with the model, t, W and Xi in double."""
    import copy
    import torch
    from oracle import fbsnn_ref as fr
    model, _ = loss_model(c)
    dt = torch.float64 if double else torch.float32
    if double:
        model = copy.deepcopy(model).double()
    tt = torch.as_tensor(np.array(t)).to(dt).reshape(c["M"], c["N"] + 1, 1)
    WW = torch.as_tensor(np.array(W)).to(dt)
    Xi = torch.as_tensor(xi_shared(c)).to(dt)
    return fr.loss_and_grads(model, loss_problem(c), tt, WW, Xi, c["M"], c["D"])
