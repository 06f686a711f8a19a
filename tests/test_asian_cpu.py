"""The arithmetic-average (Asian) problem without a GPU: asian_step and the
row-sum order of csrc/sde.hpp, compiled as plain host C++ (g++
-ffp-contract=off, as tests/test_sde_step_cpu.py does), equal the numpy chain
of tests/asian_reference.py bit for bit; the references of the GPU tests are
held to each other and to the exact expectation of the scheme; the Python
surface that needs no device."""
import os
import subprocess

import numpy as np
import pytest
import torch

import asian_reference as ar
from conftest import PKG_NAME, ROOT, load_pkg
from oracle import philox as ph

f32 = np.float32
CSRC = os.path.join(ROOT, PKG_NAME, "csrc")
M, N, T, SEED = 3, 13, 1.0, 5

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sde.hpp"
#ifdef __HIPCC__
#error "this driver is the plain host C++ build of sde.hpp"
#endif
using namespace dbsde;

static float rd() {
  char b[64];
  if (scanf("%63s", b) != 1) exit(2);
  return strtof(b, nullptr);
}
static std::vector<float> rdn(size_t n) {
  std::vector<float> v(n);
  for (auto& x : v) x = rd();
  return v;
}

// argv: M N k; stdin: mu_a sig_a sig_b T, t [N+1], Xi [M, 1 + k], dw [M, N, k]
// stdout: X [M, N+1, 1 + k], then the row sums [M, N]
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int M = atoi(argv[1]), N = atoi(argv[2]), k = atoi(argv[3]), D = k + 1;
  const std::vector<float> c = rdn(4);
  const std::vector<float> t = rdn(N + 1), xi = rdn((size_t)M * D), dw = rdn((size_t)M * N * k);
  std::vector<float> X((size_t)M * (N + 1) * D), sums((size_t)M * N);
  for (int m = 0; m < M; ++m) {
    std::vector<float> x(xi.begin() + (size_t)m * D, xi.begin() + (size_t)(m + 1) * D);
    for (int n = 0; n <= N; ++n) {
      float* Xr = &X[((size_t)m * (N + 1) + n) * D];
      for (int d = 0; d < D; ++d) Xr[d] = x[d];
      if (n == N) break;
      const float dt = rn_sub(t[n + 1], t[n]);
      const float s = asian_row_sum(&x[1], k);
      sums[(size_t)m * N + n] = s;
      asian_step(asian_mean(s, k), dt, c[3], x[0]);
      for (int i = 0; i < k; ++i) diag_step(c[0], c[1], c[2], dt, dw[((size_t)m * N + n) * k + i], x[1 + i]);
    }
  }
  for (float v : X) printf("%a\n", (double)v);
  for (float v : sums) printf("%a\n", (double)v);
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("asian_step")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("k", [1, 3, 16, 17, 70])
@pytest.mark.parametrize("Tm", [1.0, 0.7])
def test_step_and_row_sum_order_equal_the_numpy_chain(driver, k, Tm):
    """Unequal prices, sig_b != 0, T = 0.7 (a division that rounds); k = 70 has
    lanes with 4 and with 5 terms."""
    coef = dict(mu_a=0.05, sig_a=0.2, sig_b=0.1)
    Xi = np.concatenate([np.full((M, 1), 0.25), np.random.RandomState(k).uniform(0.5, 1.5, (M, k))], 1).astype(f32)
    dw = ph.increments(SEED, 0, 0, M, N, k, Tm)
    words = [np.asarray(a, f32).ravel() for a in ([coef["mu_a"], coef["sig_a"], coef["sig_b"], Tm],
                                                  ph.time_grid(N, Tm), Xi, dw)]
    text = " ".join(float(v).hex() for v in np.concatenate(words))
    out = subprocess.run([driver, str(M), str(N), str(k)], input=text, capture_output=True, text=True, check=True)
    vals = np.array([float.fromhex(w) for w in out.stdout.split()], np.float64)
    got = vals.astype(f32)
    assert np.array_equal(got.astype(np.float64), vals)
    nx = M * (N + 1) * (k + 1)
    X, sums = got[:nx].reshape(M, N + 1, k + 1), got[nx:].reshape(M, N)
    Xr, sdw = ar.rollout(Xi, dw, Tm, **coef)
    np.testing.assert_array_equal(bits(X), bits(Xr))
    ref_sums = np.stack([ar.row_sum(Xr[:, n, 1:]) for n in range(N)], 1)
    np.testing.assert_array_equal(bits(sums), bits(ref_sums))
    assert np.all(sdw[:, :, 0] == 0) and np.abs(sdw[:, :, 1:]).min() > 0
    assert Xr[:, -1, 0].min() > 0.25 + 0.3                    # the average moved
    if k == 70:
        seq = np.zeros(M, f32)
        for i in range(k):
            seq = seq + Xr[:, 3, 1 + i]
        assert np.any(bits(seq) != bits(ref_sums[:, 3]))       # the order is felt: not the sequential sum


def test_left_point_rule_in_closed_form():
    """dw = 0, mu_a = 0: S stays at Xi, so A_N = A_0 + mean S exactly where the
    arithmetic is exact (prices that are multiples of 1/8, N = 4, T = 1)."""
    k, Nn = 5, 4
    Xi = np.array([[0.5, 1.0, 1.25, 0.75, 1.5, 0.5]], f32)
    X, sdw = ar.rollout(Xi, np.zeros((2, Nn, k), f32), 1.0, mu_a=0.0, sig_a=0.2)
    np.testing.assert_array_equal(X[:, -1, 0], f32(0.5 + 1.0))
    np.testing.assert_array_equal(X[:, 2, 0], f32(0.5 + 0.5))
    assert np.all(sdw == 0)


# ---------------------------------------------------------------- the references against each other
_ARB = {}


def arbiter_restatement(pkg, k):
    """The numpy restatement of the arbiter's two points at k assets, once per process."""
    if k not in _ARB:
        c = ar.ARBITER
        sp = ar.spec(pkg, "call_mean", strike=0.0, mu_a=c["mu_a"], sig_a=c["sig_a"])
        X = np.stack([ar.arbiter_point(k)] * len(c["ts"]))
        _ARB[k] = (sp, X, ar.mc_value(sp, np.array(c["ts"], f32), X, T, c["n_steps"], c["mc"], seed=c["seed"]))
    return _ARB[k]


@pytest.mark.parametrize("k", ar.ARBITER["ks"])
def test_restatement_lies_within_4_stderr_of_the_exact_expectation(k):
    """Strike 0, mu = 0.05, sigma = 0.4, N = 50, mc = 2^18: the call is always in
    the money (S stays positive: asserted through min A_T > A_p), so its value
    is the exact expectation of the Euler scheme.  The GPU arm of this check is
    tests/test_gpu_asian.py::test_mc_arbiter."""
    pkg = load_pkg()
    c = ar.ARBITER
    sp, X, ref = arbiter_restatement(pkg, k)
    for p, t in enumerate(c["ts"]):
        want = ar.euler_expectation(X[p], t, T, c["n_steps"], float(f32(c["mu_a"])), float(f32(ar.R_RATE)))
        err, se = abs(ref["value"][p] - want), ref["stderr"][p]
        print(f"k={k} t={t}: restatement {ref['value'][p]:.6f} +- {se:.2e}, exact {want:.6f}, |diff| {err:.2e} = "
              f"{err / se:.2f} stderr")
        assert se > 0 and err <= 4 * se
        assert ref["ambiguous"][p] == 0


def test_call_minus_put_is_the_discounted_forward_in_the_restatement():
    pkg = load_pkg()
    k, n_steps, mc = 3, 6, 2048
    X, t = ar.mc_points(k)[:2], ar.MC_T_POINTS[:2]
    call = ar.mc_value(ar.spec(pkg, "call_mean"), t, X, T, n_steps, mc, seed=2)
    put = ar.mc_value(ar.spec(pkg, "put_mean"), t, X, T, n_steps, mc, seed=2)
    disc = np.exp(-float(f32(ar.R_RATE)) * (1.0 - t.astype(np.float64)))
    np.testing.assert_allclose(call["value"] - put["value"], disc * (call["mean_AT"] - 1.0), rtol=0, atol=1e-12)
    assert np.all(call["value"] > 0) and np.all(put["value"] > 0)


def test_restated_delta_is_the_derivative_of_the_restated_value():
    """Smooth payoff, common draws: the pathwise delta equals a central
    difference of two bumped points in every column, A included, within the
    truncation bound of tests/asian_reference.py (h = 1/256, exact in fp32; the
    point is at the money, where the delta is not small)."""
    pkg = load_pkg()
    k, n_steps, mc, h = 3, 6, 512, 1.0 / 256
    sp = ar.spec(pkg, "smooth_call")
    x = np.array([0.5, 1.0, 1.125, 0.875], f32)
    ref = ar.mc_value(sp, [0.5], x[None], T, n_steps, mc, seed=2, delta=True)
    tol = ar.central_difference_bound(ref["dA_max"][0], h)
    assert abs(ref["mean_AT"][0] - 1.0) < 0.05 and np.all(tol < 1e-3 * np.abs(ref["delta"][0]))
    for d in range(k + 1):
        e = np.zeros(k + 1, f32)
        e[d] = h
        up = ar.mc_value(sp, [0.5], (x + e)[None], T, n_steps, mc, seed=2)["value"][0]
        dn = ar.mc_value(sp, [0.5], (x - e)[None], T, n_steps, mc, seed=2)["value"][0]
        err = abs((up - dn) / (2 * h) - ref["delta"][0, d])
        print(f"column {d}: pathwise {ref['delta'][0, d]:.6f}, |central difference - it| {err:.2e} (bound {tol[d]:.2e})")
        assert err <= tol[d] + 1e-12, d


@pytest.mark.parametrize("case", list(ar.LOSS_CASES))
def test_loss_cases_have_rows_on_both_sides_of_the_kink(case):
    k, Mc = ar.LOSS_CASES[case][:2]
    dw = ph.increments(ar.LOSS_SEED + k, 0, 0, Mc, ar.N, k, T)
    X, _ = ar.rollout(ar.xi_state(k), dw, T, **ar.COEF)
    a = X[:, -1, 0].astype(np.float64) - ar.LOSS_STRIKE
    print(f"{case}: A_T - K in [{a.min():.4f}, {a.max():.4f}], {int((a > 0).sum())} of {Mc} in the money")
    assert (a > 1e-4).sum() >= 1 and (a < -1e-4).sum() >= 1 and np.abs(a).min() > 1e-4      # no row near the tie


def test_fp64_loss_paths_are_the_fp32_chain():
    """The fp64 autograd loss rolls out the process the numpy chain rolls out:
    X within fp32 rounding, and the terminal Z term is the A column's alone."""
    case = "fused16_k3"
    k, Mc = ar.LOSS_CASES[case][:2]
    model, _ = ar.loss_model(case)
    dw = ph.increments(ar.LOSS_SEED + k, 0, 0, Mc, ar.N, k, T)
    prob = ar.AsianProblem(k, "call_mean", ar.LOSS_STRIKE)
    ref = ar.loss_and_grads(model, prob, ph.time_grid(ar.N, T), dw, ar.xi_state(k))
    X, sdw = ar.rollout(ar.xi_state(k), dw, T, **ar.COEF)
    np.testing.assert_allclose(X, ref["X"], rtol=1e-5, atol=1e-6)
    assert np.isfinite(ref["loss"]) and np.abs(ref["grad"]).max() > 0
    ZN = ref["Z"][:, -1, :]
    assert np.abs(ZN[:, 1:]).max() > 1e-3                     # u_S at T is not penalised: it stays what the net gives


# ---------------------------------------------------------------- the Python surface without a device
def test_spec_functions_know_the_A_row():
    pkg = load_pkg()
    gen = __import__("importlib").import_module(PKG_NAME + ".generic")
    k, Tm = 4, 0.7
    sp = ar.spec(pkg, "put_mean", strike=0.9, sig_b=0.1)
    with pytest.raises(ValueError, match="needs T"):
        gen.spec_functions(sp)
    f = gen.spec_functions(sp, T=Tm)
    prob = ar.AsianProblem(k, "put_mean", 0.9, T=Tm, sig_b=0.1)
    rs = np.random.RandomState(1)
    X = torch.tensor(np.concatenate([rs.uniform(0.5, 1.2, (6, 1)), rs.uniform(0.5, 1.5, (6, k))], 1))
    t, Y, Z = torch.zeros(6, 1), torch.ones(6, 1, dtype=X.dtype), torch.ones(6, k + 1, dtype=X.dtype)
    np.testing.assert_allclose(f["mu_tf"](t, X), prob.mu(t, X), rtol=1e-14)
    np.testing.assert_allclose(f["sigma_tf"](t, X), prob.sigma(t, X), rtol=1e-14)
    assert tuple(f["sigma_tf"](t, X).shape) == (6, k + 1, k) and bool((f["sigma_tf"](t, X)[:, 0, :] == 0).all())
    np.testing.assert_allclose(f["g_tf"](X), prob.g(X), rtol=1e-14)
    np.testing.assert_allclose(f["phi_tf"](t, X, Y, Z), prob.phi(t, X, Y, Z), rtol=1e-14)
    dg = f["Dg_tf"](X)
    assert bool((dg[:, 1:] == 0).all()) and bool((dg[:, 0] != 0).any())
    plain = gen.spec_functions(pkg.ProblemSpec(mu_a=0.05, sig_a=0.2))     # a spec without the average is unchanged
    np.testing.assert_allclose(plain["mu_tf"](t, X), 0.05 * X, rtol=1e-14)


def test_problem_spec_average_field():
    pkg = load_pkg()
    sp = pkg.ProblemSpec()
    assert sp.average is False and list(sp.__dataclass_fields__)[-1] == "average"
    assert pkg.ProblemSpec(average=True, g="call_mean", g_cols=1).to_c().kind == 4
    assert pkg.ProblemSpec(g="call_mean").to_c().kind == 0
    with pytest.raises(ValueError, match="Heston"):
        pkg.ProblemSpec(kind="heston", average=True, g="call_mean").to_c()
    for name in ("AsianCallOption", "AsianPutOption", "AsianBasketCallOption", "AsianBasketPutOption"):
        assert name in pkg.__all__ and issubclass(getattr(pkg, name), pkg.FBSNN)
    assert issubclass(pkg.AsianPutOption, pkg.AsianCallOption) and pkg.AsianBasketPutOption.option_type == "put"
    assert pkg.AsianBasketCallOption.schedule == "corr" and pkg.AsianCallOption.schedule == "nd"
