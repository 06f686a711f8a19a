"""The geometric-average Asian problem without a GPU: geo_lg / geo_exp /
geo_row_sum and asian_step of csrc/sde.hpp, compiled as plain host C++ (g++
-ffp-contract=off, as tests/test_asian_cpu.py builds its driver), equal the
numpy chain of tests/geo_asian_reference.py bit for bit; the float64 closed
form is held to the textbook formula, to its own central differences, to
parity and to the full covariance; the restatement of dbsde_mc_value converges
to the closed form; the Python surface that needs no device."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import geo_asian_reference as gr
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
// stdout: X [M, N+1, 1 + k], then a = log G [M, N+1], then the row sums of lg [M, N]
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int M = atoi(argv[1]), N = atoi(argv[2]), k = atoi(argv[3]), D = k + 1;
  const std::vector<float> c = rdn(4);
  const std::vector<float> t = rdn(N + 1), xi = rdn((size_t)M * D), dw = rdn((size_t)M * N * k);
  std::vector<float> X((size_t)M * (N + 1) * D), as((size_t)M * (N + 1)), sums((size_t)M * N);
  for (int m = 0; m < M; ++m) {
    std::vector<float> x(xi.begin() + (size_t)m * D, xi.begin() + (size_t)(m + 1) * D);
    float a = geo_lg(x[0]);
    for (int n = 0; n <= N; ++n) {
      float* Xr = &X[((size_t)m * (N + 1) + n) * D];
      for (int d = 0; d < D; ++d) Xr[d] = x[d];
      Xr[0] = n == 0 ? x[0] : geo_exp(a);
      as[(size_t)m * (N + 1) + n] = a;
      if (n == N) break;
      const float dt = rn_sub(t[n + 1], t[n]);
      const float s = geo_row_sum(&x[1], k);
      sums[(size_t)m * N + n] = s;
      asian_step(asian_mean(s, k), dt, c[3], a);
      for (int i = 0; i < k; ++i) diag_step(c[0], c[1], c[2], dt, dw[((size_t)m * N + n) * k + i], x[1 + i]);
    }
  }
  for (float v : X) printf("%a\n", (double)v);
  for (float v : as) printf("%a\n", (double)v);
  for (float v : sums) printf("%a\n", (double)v);
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("geo_asian_step")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("k", [1, 3, 16, 17, 70])
@pytest.mark.parametrize("Tm", [1.0, 0.7])
def test_log_chain_equals_the_numpy_chain(driver, k, Tm):
    """Unequal prices, G_0 != 1, T = 0.7 (a division that rounds); k = 70 has
    lanes with 4 and with 5 terms.  Both sides round the fp64 log / exp to fp32
    once: they agree unless an argument sits within an fp64 ulp of a rounding
    boundary (no case here does; a case that did would change its seed)."""
    coef = dict(mu_a=0.05, sig_a=0.2, sig_b=0.0)
    Xi = np.concatenate([np.full((M, 1), 0.875), np.random.RandomState(k).uniform(0.5, 1.5, (M, k))], 1).astype(f32)
    dw = ph.increments(SEED, 0, 0, M, N, k, Tm)
    words = [np.asarray(a, f32).ravel() for a in ([coef["mu_a"], coef["sig_a"], coef["sig_b"], Tm],
                                                  ph.time_grid(N, Tm), Xi, dw)]
    text = " ".join(float(v).hex() for v in np.concatenate(words))
    out = subprocess.run([driver, str(M), str(N), str(k)], input=text, capture_output=True, text=True, check=True)
    vals = np.array([float.fromhex(w) for w in out.stdout.split()], np.float64)
    got = vals.astype(f32)
    assert np.array_equal(got.astype(np.float64), vals)
    nx, na = M * (N + 1) * (k + 1), M * (N + 1)
    X, a, sums = got[:nx].reshape(M, N + 1, k + 1), got[nx:nx + na].reshape(M, N + 1), got[nx + na:].reshape(M, N)
    Xr, sdw, ar_ = gr.rollout(Xi, dw, Tm, with_log=True, **coef)
    np.testing.assert_array_equal(bits(X), bits(Xr))
    np.testing.assert_array_equal(bits(a), bits(ar_))
    ref_sums = np.stack([gr.ar.row_sum(gr.lg(Xr[:, n, 1:])) for n in range(N)], 1)
    np.testing.assert_array_equal(bits(sums), bits(ref_sums))
    assert np.all(sdw[:, :, 0] == 0) and np.abs(sdw[:, :, 1:]).min() > 0
    assert np.all(Xr[:, 0, 0] == f32(0.875)) and np.abs(Xr[:, -1, 0] - f32(0.875)).min() > 1e-3     # the average moved


def test_exponential_form_in_closed_form():
    """dw = 0, mu_a = 0: S stays at Xi, so G_N = G_0 exp(mean log S); with every
    S = 1 the logs are exactly 0 and G stays at G_0 = 1 bit for bit."""
    k, Nn = 5, 4
    X, sdw = gr.rollout(gr.xi_state(k), np.zeros((2, Nn, k), f32), 1.0, mu_a=0.0, sig_a=0.2)
    assert np.all(X[:, :, 0] == 1.0) and np.all(sdw == 0)
    Xi = np.array([[1.0, 2.0, 0.5, 4.0, 1.0, 1.0]], f32)
    X, _ = gr.rollout(Xi, np.zeros((2, Nn, k), f32), 1.0, mu_a=0.0, sig_a=0.2)
    np.testing.assert_allclose(X[:, -1, 0], 4.0 ** 0.2, rtol=4 * 2.0 ** -24)


# ---------------------------------------------------------------- the closed form
CF = dict(mu=0.05, r=0.05, sigma=0.4, K=1.0)


def test_closed_form_is_the_textbook_formula_at_one_asset():
    """k = 1, L = I, t = 0, G = 1: the Black-Scholes formula with volatility
    sigma / sqrt(3) and drift (r - sigma^2 / 2) / 2 of log G_T (Kemna-Vorst)."""
    r, sig, K, Tm = 0.05, 0.4, 1.0, 1.0
    for S in (0.8, 1.0, 1.05, 1.3):
        sg = sig / math.sqrt(3.0)
        b = 0.5 * (r - 0.5 * sig * sig) + 0.5 * sg * sg          # cost of carry of the geometric average
        d1 = (math.log(S / K) + (b + 0.5 * sg * sg) * Tm) / (sg * math.sqrt(Tm))
        d2 = d1 - sg * math.sqrt(Tm)
        N_ = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))
        want = S * math.exp((b - r) * Tm) * N_(d1) - K * math.exp(-r * Tm) * N_(d2)
        got, _ = gr.closed_form(np.array([[1.0, S]]), [0.0], Tm, r, r, sig, K, 1.0, 1.0)
        print(f"S = {S}: closed form {got[0]:.12f}, textbook {want:.12f}")
        assert abs(got[0] - want) <= 1e-14


@pytest.mark.parametrize("put", [False, True], ids=["call", "put"])
def test_closed_form_deltas_are_central_differences(put):
    """Every delta column against central differences of the price at h and
    h / 2: the error falls by 4 (+-25 %) and is <= 1e-3 |delta| at h / 2."""
    k, Tm, h = 3, 0.7, 1.0 / 128
    L = gr.equicorr_L(k, 0.3)
    cbar, vbar = gr.factor_moments(L, k)
    x = np.array([[0.97, 1.0, 1.125, 0.875]])
    args = (Tm, CF["mu"], CF["r"], CF["sigma"], CF["K"], cbar, vbar, put)
    _, d = gr.closed_form(x, [0.2], *args)
    for c in range(k + 1):
        errs = []
        for hh in (h, h / 2):
            e = np.zeros((1, k + 1))
            e[0, c] = hh
            cd = (gr.closed_form(x + e, [0.2], *args)[0][0] - gr.closed_form(x - e, [0.2], *args)[0][0]) / (2 * hh)
            errs.append(abs(cd - d[0, c]))
        print(f"column {c}: delta {d[0, c]:.8f}, errors {errs[0]:.3e} {errs[1]:.3e}, ratio {errs[0] / errs[1]:.3f}")
        assert 3.0 <= errs[0] / errs[1] <= 5.0 and errs[1] <= 1e-3 * abs(d[0, c])


def test_closed_form_call_minus_put_is_the_discounted_forward():
    k, Tm = 4, 1.0
    rs = np.random.RandomState(3)
    x = np.concatenate([rs.uniform(0.8, 1.2, (16, 1)), rs.uniform(0.7, 1.4, (16, k))], 1)
    t = rs.uniform(0.0, 0.9, 16)
    cbar, vbar = gr.factor_moments(gr.equicorr_L(k, 0.3), k)
    args = (Tm, CF["mu"], CF["r"], CF["sigma"], CF["K"], cbar, vbar)
    call, dc_ = gr.closed_form(x, t, *args)
    put, dp = gr.closed_form(x, t, *args, put=True)
    Mm, V, tau = gr.closed_form_terms(x, t, *args)
    np.testing.assert_allclose(call - put, np.exp(-CF["r"] * tau) * (np.exp(Mm + 0.5 * V) - CF["K"]), rtol=0, atol=1e-14)
    assert np.all(call > 0) and np.all(put > 0) and np.all(dc_ > 0) and np.all(dp < 0)
    # tau <= 0: the payoff and its one-sided derivative in G
    x0 = np.array([[1.0, 1.1], [1.2, 0.9], [0.7, 1.0]])
    c0, d0 = gr.closed_form(x0, [1.0, 1.0, 1.5], Tm, 0.05, 0.05, 0.4, 1.0, 1.0, 1.0)
    p0, e0 = gr.closed_form(x0, [1.0, 1.0, 1.5], Tm, 0.05, 0.05, 0.4, 1.0, 1.0, 1.0, put=True)
    np.testing.assert_array_equal(c0, [0.0, x0[1, 0] - 1.0, 0.0])
    np.testing.assert_array_equal(d0, [[0.5, 0], [1, 0], [0, 0]])
    np.testing.assert_array_equal(p0, [0.0, 0.0, 1.0 - x0[2, 0]])
    np.testing.assert_array_equal(e0, [[-0.5, 0], [0, 0], [-1, 0]])


def test_closed_form_with_a_factor_is_the_full_covariance():
    """rho = 0.3, k = 5: vbar and cbar from the factor equal those of the full
    covariance matrix, and the price equals the formula evaluated with the
    variance of mean_i (L W)_i written out."""
    k, rho, Tm, t = 5, 0.3, 1.0, 0.25
    C = (1 - rho) * np.eye(k) + rho * np.ones((k, k))
    cbar, vbar = gr.factor_moments(np.linalg.cholesky(C), k)
    assert abs(cbar - 1.0) <= 1e-15 and abs(vbar - (1 + (k - 1) * rho) / k) <= 1e-15
    x = np.concatenate([[0.97], np.linspace(0.9, 1.2, k)])[None]
    got, _ = gr.closed_form(x, [t], Tm, CF["mu"], CF["r"], CF["sigma"], CF["K"], cbar, vbar)
    tau = Tm - t
    w = np.ones(k) / k
    var = CF["sigma"] ** 2 * (w @ C @ w) * tau ** 3 / (3 * Tm * Tm)
    mean = math.log(0.97) + (tau * np.mean(np.log(x[0, 1:])) + (CF["mu"] - 0.5 * CF["sigma"] ** 2 * np.mean(np.diag(C)))
                             * tau * tau / 2) / Tm
    d2 = (mean - math.log(CF["K"])) / math.sqrt(var)
    N_ = lambda z: 0.5 * math.erfc(-z / math.sqrt(2.0))
    want = math.exp(-CF["r"] * tau) * (math.exp(mean + var / 2) * N_(d2 + math.sqrt(var)) - CF["K"] * N_(d2))
    assert abs(got[0] - want) <= 1e-14


# ---------------------------------------------------------------- the restatement against the closed form
@pytest.mark.parametrize("k,t,G", gr.ARBITER["points"], ids=[f"k{k}-t{t}" for k, t, _ in gr.ARBITER["points"]])
def test_scheme_bias_shrinks_to_the_closed_form(k, t, G):
    """Strike 1, sigma = 0.4, mu = r = 0.05, mc = 2^16 Philox draws: the
    restatement's distance from the closed form at 50, 100, 200 and 400 steps
    (printed: the bias is O(dt)), within 3 stderr at 400.  The GPU arm is
    tests/test_gpu_geo_asian.py::test_mc_arbiter."""
    pkg = load_pkg()
    c = gr.ARBITER
    sp = gr.spec(pkg, "call_mean", strike=c["strike"], mu_a=c["mu_a"], sig_a=c["sig_a"])
    want = gr.arbiter_exact(k, t, G)
    x = gr.arbiter_point(k, G)[None]
    for ns in c["steps"]:
        r = gr.mc_value(sp, [t], x, T, ns, c["mc"], seed=c["seed"], L=gr.arbiter_L(k))
        diff, se = r["value"][0] - want, r["stderr"][0]
        print(f"k={k} t={t} n_steps={ns}: restatement {r['value'][0]:.6f} +- {se:.2e}, closed form {want:.6f}, "
              f"difference {diff:+.2e} = {abs(diff) / se:.2f} stderr")
    assert se > 0 and abs(diff) <= 3 * se


def test_call_minus_put_is_the_discounted_forward_in_the_restatement():
    pkg = load_pkg()
    k, n_steps, mc = 3, 6, 2048
    X, t = gr.mc_points(k)[:2], gr.MC_T_POINTS[:2]
    call = gr.mc_value(gr.spec(pkg, "call_mean"), t, X, T, n_steps, mc, seed=2)
    put = gr.mc_value(gr.spec(pkg, "put_mean"), t, X, T, n_steps, mc, seed=2)
    disc = np.exp(-float(f32(gr.R_RATE)) * (1.0 - t.astype(np.float64)))
    np.testing.assert_allclose(call["value"] - put["value"], disc * (call["mean_GT"] - 1.0), rtol=0, atol=1e-12)
    assert np.all(call["value"] > 0) and np.all(put["value"] > 0)


def test_restated_delta_is_the_derivative_of_the_restated_value():
    """Smooth payoff, common draws: the pathwise delta of every column, G
    included, against central differences of the restated value at h and
    h / 2 (exact in fp32): the error falls by 4 (+-25 %) and is <= 1e-3 |delta|
    at h / 2.  The paths are fp32, so a value carries a rounding of about 2^-24
    of itself, 1e-7 / h in the difference: far below the truncation error at
    these h."""
    pkg = load_pkg()
    k, n_steps, mc, h = 3, 6, 512, 1.0 / 16
    sp = gr.spec(pkg, "smooth_call")
    x = np.array([1.0, 1.0, 1.125, 0.875], f32)
    ref = gr.mc_value(sp, [0.5], x[None], T, n_steps, mc, seed=2, delta=True)
    assert abs(ref["mean_GT"][0] - 1.0) < 0.05
    for d in range(k + 1):
        errs = []
        for hh in (h, h / 2):
            e = np.zeros(k + 1, f32)
            e[d] = hh
            up = gr.mc_value(sp, [0.5], (x + e)[None], T, n_steps, mc, seed=2)["value"][0]
            dn = gr.mc_value(sp, [0.5], (x - e)[None], T, n_steps, mc, seed=2)["value"][0]
            errs.append(abs((up - dn) / (2 * hh) - ref["delta"][0, d]))
        print(f"column {d}: pathwise {ref['delta'][0, d]:.6f}, errors {errs[0]:.3e} {errs[1]:.3e}, "
              f"ratio {errs[0] / errs[1]:.3f}")
        assert 3.0 <= errs[0] / errs[1] <= 5.0 and errs[1] <= 1e-3 * abs(ref["delta"][0, d]), d


@pytest.mark.parametrize("case", list(gr.LOSS_CASES))
def test_loss_cases_have_rows_on_both_sides_of_the_kink(case):
    k, Mc = gr.LOSS_CASES[case][:2]
    dw = ph.increments(gr.LOSS_SEED + k, 0, 0, Mc, gr.N, k, T)
    X, _ = gr.rollout(gr.xi_state(k), dw, T, **gr.COEF)
    a = X[:, -1, 0].astype(np.float64) - gr.LOSS_STRIKE
    print(f"{case}: G_T - K in [{a.min():.4f}, {a.max():.4f}], {int((a > 0).sum())} of {Mc} in the money")
    assert (a > 1e-4).sum() >= 1 and (a < -1e-4).sum() >= 1 and np.abs(a).min() > 1e-4      # no row near the tie


def test_fp64_loss_paths_are_the_fp32_chain():
    """The fp64 autograd loss rolls out the process the numpy chain rolls out:
    X within the GPU test's bound."""
    case = "fused16_k3"
    k, Mc = gr.LOSS_CASES[case][:2]
    model, _ = gr.loss_model(case)
    dw = ph.increments(gr.LOSS_SEED + k, 0, 0, Mc, gr.N, k, T)
    prob = gr.GeoAsianProblem(k, "call_mean", gr.LOSS_STRIKE)
    ref = gr.loss_and_grads(model, prob, ph.time_grid(gr.N, T), dw, gr.xi_state(k))
    X, sdw = gr.rollout(gr.xi_state(k), dw, T, **gr.COEF)
    np.testing.assert_allclose(X, ref["X"], rtol=1e-5, atol=1e-6)
    assert np.isfinite(ref["loss"]) and np.abs(ref["grad"]).max() > 0
    assert np.abs(ref["Z"][:, -1, 1:]).max() > 1e-3


# ---------------------------------------------------------------- the Python surface without a device
def test_spec_functions_know_the_G_row():
    pkg = load_pkg()
    gen = __import__("importlib").import_module(PKG_NAME + ".generic")
    k, Tm = 4, 0.7
    sp = gr.spec(pkg, "put_mean", strike=0.9)
    with pytest.raises(ValueError, match="needs T"):
        gen.spec_functions(sp)
    f = gen.spec_functions(sp, T=Tm)
    prob = gr.GeoAsianProblem(k, "put_mean", 0.9, T=Tm)
    rs = np.random.RandomState(1)
    X = torch.tensor(np.concatenate([rs.uniform(0.5, 1.2, (6, 1)), rs.uniform(0.5, 1.5, (6, k))], 1))
    t, Y, Z = torch.zeros(6, 1), torch.ones(6, 1, dtype=X.dtype), torch.ones(6, k + 1, dtype=X.dtype)
    np.testing.assert_allclose(f["mu_tf"](t, X), prob.mu(t, X), rtol=1e-14)
    np.testing.assert_allclose(f["sigma_tf"](t, X), prob.sigma(t, X), rtol=1e-14)
    assert bool((f["sigma_tf"](t, X)[:, 0, :] == 0).all())
    np.testing.assert_allclose(f["g_tf"](X), prob.g(X), rtol=1e-14)
    arith = gen.spec_functions(gr.ar.spec(pkg, "put_mean", strike=0.9), T=Tm)     # the arithmetic row is unchanged
    np.testing.assert_allclose(arith["mu_tf"](t, X)[:, :1], X[:, 1:].mean(1, keepdim=True) / Tm, rtol=1e-14)
    assert float((arith["mu_tf"](t, X)[:, 0] - f["mu_tf"](t, X)[:, 0]).abs().min()) > 0.1


def test_problem_spec_average_field():
    pkg = load_pkg()
    sp = pkg.ProblemSpec()
    assert sp.average is False and list(sp.__dataclass_fields__)[-1] == "average"
    assert pkg._lib.PROB_GEO_ASIAN == 8 and len(pkg._lib.PROBLEM_KINDS) == 3
    assert pkg.ProblemSpec(average="geometric", g="call_mean", g_cols=1).to_c().kind == 8
    assert pkg.ProblemSpec(average="arithmetic", g="call_mean", g_cols=1).to_c().kind == 4
    assert pkg.ProblemSpec(average=True, g="call_mean", g_cols=1).to_c().kind == 4
    assert pkg.ProblemSpec(g="call_mean").to_c().kind == 0
    with pytest.raises(ValueError, match="unknown average"):
        pkg.ProblemSpec(average="harmonic", g="call_mean", g_cols=1).to_c()
    for kind in ("heston", "heston2"):
        with pytest.raises(ValueError, match="Heston"):
            pkg.ProblemSpec(kind=kind, average="geometric", g="call_mean").to_c()
    assert pkg._lib.EXACT_KINDS["geo_asian"] == 10 and pkg._lib.EXACT_KINDS["geo_asian_put"] == 11
    assert 9 not in pkg._lib.EXACT_KINDS.values()
    names = ("GeometricAsianCallOption", "GeometricAsianPutOption", "GeometricAsianBasketCallOption",
             "GeometricAsianBasketPutOption")
    for name in names:
        assert name in pkg.__all__ and issubclass(getattr(pkg, name), pkg.FBSNN)
        assert callable(getattr(pkg, name).closed_form)
    assert issubclass(pkg.GeometricAsianPutOption, pkg.GeometricAsianCallOption)
    assert pkg.GeometricAsianBasketPutOption.option_type == "put"
    assert pkg.GeometricAsianBasketCallOption.schedule == "corr" and pkg.GeometricAsianCallOption.schedule == "nd"
