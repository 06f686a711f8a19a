"""The preconditions of tests/test_gpu_path_kernels.py, on the CPU: the case
table of tests/path_cases.py reaches what it claims to reach, the bound on the
correlated increments holds for the reference alone and fails on a dropped
block, a transposed factor and a shifted path, the oracle's Philox key uses
all 64 bits of seed and offset and all 32 of the path word, and every loss
case has a reference tight enough for the tolerance it is used with.  No GPU.
"""
import numpy as np
import pytest

import path_cases as pc
from oracle import philox as ph


# --------------------------------------------------------------------------
# coverage of the table
# --------------------------------------------------------------------------
def test_correlated_cases_reach_every_instance_and_both_wide_sizes():
    assert {pc.nblk(c["D"]) for c in pc.CORR_CASES} == set(range(1, 9))
    assert {c["D"] for c in pc.CORR_CASES} == set(pc.CORR_D)
    for b in range(1, 8):          # both sides of every block edge
        assert {16 * b, 16 * b + 1} <= set(pc.CORR_D)
    assert {127, 128} <= set(pc.CORR_D)            # nb <= 128 with Dp = 144
    for D in pc.CORR_FULL:
        assert [(c["M"], c["N"]) for c in pc.CORR_CASES if c["D"] == D] == pc.SHAPES


@pytest.mark.parametrize("family", list(pc.FAMILIES))
def test_every_family_covers_the_ragged_shapes_and_keys(family):
    cases = pc.FAMILIES[family]
    assert {c["N"] % 4 for c in cases} == {0, 1, 2, 3}
    Ms = {c["M"] for c in cases}
    assert min(Ms) < 16 and 16 in Ms and max(Ms) > 16
    assert any(c["M"] % 16 in (1, 15) for c in cases)
    # more than one Philox block with the last one partly used
    assert any(c["N"] > 4 and c["N"] % 4 for c in cases)
    assert sorted(c["key"] for c in cases if c["key"] != "default") == ["high", "shard"]
    assert len({c["id"] for c in cases}) == len(cases)
    for c in cases:
        k = pc.key_of(c)
        assert 0 <= k["path0"] and k["path0"] + (c["full_M"] or c["M"]) <= 2 ** 32
        if c["key"] == "shard":
            assert k["path0"] % 2 == 1 and k["path0"] + c["M"] <= c["full_M"]


def test_shapes_and_sizes_are_the_ragged_ones():
    assert {N % 4 for _, N in pc.SHAPES} == {0, 1, 2, 3}
    assert {np.sign(N - 8) for _, N in pc.SHAPES} == {-1, 0, 1}      # the chains load 8 steps ahead
    assert {M for M, _ in pc.SHAPES} >= {1, 15, 16, 17, 33}
    for c in pc.FAMILIES["heston"]:
        assert (c["M"] * c["D"]) % 256 != 0
        assert ((c["full_M"] or c["M"]) * c["D"]) % 256 != 0
    # the constant-1 column (D + 1) in a column group without a live dimension
    assert {D for D in pc.DIAG_D if (D + 1) % 4 == 0} == {3, 7, 15}
    pad16 = lambda n: (n + 15) // 16 * 16
    assert pad16(14 + 2) == 16 and pad16(15 + 2) == 32 and pad16(126 + 2) == 128 and pad16(127 + 2) == 144
    assert pc.DIAG["sig_a"] != 0 and pc.DIAG["sig_b"] != 0 and pc.DIAG["mu_a"] != 0
    for c in pc.LOSS_CASES:
        assert c["M"] * c["N"] <= 64 and (c["M"], c["N"]) in pc.SHAPES


def test_factor_is_dense_and_a_factor():
    for D in pc.CORR_D:
        L = pc.factor(D).astype(np.float64)
        assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0)
        np.testing.assert_allclose(np.diag(L @ L.T), 1.0, atol=1e-5)
        if D > 1:
            low = np.abs(L[np.tril_indices(D, -1)])
            assert np.all(low > 0) and np.median(low) > 1e-2        # no idle entry in the triangle


# --------------------------------------------------------------------------
# the bound on the correlated increments
# --------------------------------------------------------------------------
MB, NB = 40, 13


@pytest.fixture(scope="module")
def bound_inputs():
    out = {}
    for D in pc.CORR_D:
        dz = ph.increments(9, 0, 0, MB, NB, D, pc.T)
        L = pc.factor(D)
        out[D] = (L, dz, pc.corr_ref(L, dz), pc.corr_bound(L, dz))
    return out


def test_fp32_reference_sums_stay_inside_the_bound(bound_inputs):
    worst = 0.0
    for D, (L, dz, ref, bound) in bound_inputs.items():
        assert np.all(bound > 0)
        for desc in (False, True):
            r = float((np.abs(pc.corr_fp32(L, dz, desc) - ref) / bound).max())
            worst = max(worst, r)
            assert r <= 1.0, (D, desc, r)
    print(f"fp32 ascending / descending sums: worst |err| / bound = {worst:.3g}")


def test_the_bound_has_teeth(bound_inputs):
    for D, (L, dz, ref, bound) in bound_inputs.items():
        # the 4 left-most columns of the last 16-row block dropped (one K-step of one output block)
        Lm = np.array(L)
        Lm[16 * (pc.nblk(D) - 1):, :4] = 0
        r = float((np.abs(pc.corr_ref(Lm, dz) - ref) / bound).max())
        assert r > 1.0, ("block", D, r)
        if D == 128:
            assert r > 1e4, r
        # the factor transposed (D = 1: its own transpose)
        if D > 1:
            r = float((np.abs(pc.corr_ref(L.T, dz) - ref) / bound).max())
            assert r > 1.0, ("transpose", D, r)
        # the path index shifted by one
        dz1 = ph.increments(9, 0, 1, MB, NB, D, pc.T)
        r = float((np.abs(pc.corr_ref(L, dz1) - ref) / bound).max())
        assert r > 1.0, ("path", D, r)


# --------------------------------------------------------------------------
# 64-bit keys
# --------------------------------------------------------------------------
def test_the_high_key_needs_every_upper_bit():
    M, N, D = 18, 5, 3
    k = pc.high_key(M)
    assert k["seed"] >> 32 and k["offset"] >> 32 and k["path0"] >> 31 and k["path0"] + M <= 2 ** 32
    full = ph.increments(k["seed"], k["offset"], k["path0"], M, N, D, pc.T)
    assert np.all(np.isfinite(full))
    variants = {
        "seed high word dropped": (k["seed"] & 0xFFFFFFFF, k["offset"], k["path0"]),
        "offset high word dropped": (k["seed"], k["offset"] & 0xFFFFFFFF, k["path0"]),
        "path0 wrapped to 31 bits": (k["seed"], k["offset"], k["path0"] & 0x7FFFFFFF),
    }
    for name, (s, o, p0) in variants.items():
        other = ph.increments(s, o, p0, M, N, D, pc.T)
        assert not np.any(other == full), name
    # the shard at path0 + 16 draws rows 16.. of the full batch, below 2^32 as at 0
    np.testing.assert_array_equal(ph.increments(k["seed"], k["offset"], k["path0"] + 16, M - 16, N, D, pc.T), full[16:])
    f0 = ph.increments(9, 0, 0, 40, 9, D, pc.T)
    np.testing.assert_array_equal(ph.increments(9, 0, pc.SHARD_PATH0, 18, 9, D, pc.T), f0[5:23])


# --------------------------------------------------------------------------
# the loss cases: the reference's own error is a tenth of the GPU tolerance
# --------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.LOSS_CASES, ids=pc.ids(pc.LOSS_CASES))
def test_loss_reference_is_insensitive_to_the_rounding_of_W(c):
    """The device consumes dW; the oracle differences W = fp32(cumsum dW).  In
    fp32 on that W and in fp64 on the uncast cumulative sum the oracle's loss
    must agree to 1e-5 relative (gradient: 2e-5 of its maximum), a tenth of
    what tests/test_gpu_path_kernels.py allows the device."""
    M, N, D = c["M"], c["N"], c["D"]
    L = pc.factor(D) if c["family"] == "corr" else None
    dW = ph.increments(9, 0, 0, M, N, D, pc.T, L=L)
    t = np.broadcast_to(ph.time_grid(N, pc.T), (M, N + 1))
    W64 = np.zeros((M, N + 1, D))
    W64[:, 1:] = np.cumsum(dW.astype(np.float64), axis=1)
    r32 = pc.loss_reference(c, t, ph.brownian_W(dW))
    r64 = pc.loss_reference(c, t, W64, double=True)
    np.testing.assert_array_equal(r32["used"], r64["used"])
    el = abs(r32["loss"] - r64["loss"]) / abs(r64["loss"])
    eg = np.abs(r32["grad"] - r64["grad"]).max() / np.abs(r64["grad"]).max()
    print(f"{c['id']}: loss {r64['loss']:.6g}, fp32 vs fp64 rel {el:.3g}, grad {eg:.3g} of max|grad|")
    assert np.isfinite(r64["loss"]) and r64["loss"] > 0
    assert el <= 0.1 * pc.LOSS_RTOL, el
    assert eg <= 0.1 * pc.GRAD_ATOL, eg
