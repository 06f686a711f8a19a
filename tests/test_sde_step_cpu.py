"""The Euler steps of csrc/sde.hpp, compiled as plain host C++ and run on the
oracles' increments and time grid: X and sdw equal oracle/philox.py (diagonal,
one-factor Heston) and tests/heston2_reference.py (two-factor Heston) bit for
bit.  The same functions are what every path kernel, the Monte-Carlo comparator
and the PDE residual's Heston coefficients run on the GPU.  No GPU.

The Heston states are chosen so that the oracle itself has every +-100 clamp and
the variance floor active (asserted below), N = 13 is no multiple of 4 or 8."""
import os
import subprocess

import numpy as np
import pytest

import heston2_reference as h2
import mc_reference as mr
from conftest import PKG_NAME, ROOT
from oracle import philox as ph

f32 = np.float32
CSRC = os.path.join(ROOT, PKG_NAME, "csrc")
M, N, T, SEED = 3, 13, 1.0, 5
D_DIAG, K_HESTON = 7, 5

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
static void put(const std::vector<float>& v) {
  for (float x : v) printf("%a\n", (double)x);
}

// argv: kind M N nb; stdin: the coefficients, t [N+1], Xi [M, D], dw [M, N, nb]
// stdout: X [M, N+1, D], sdw [M, N, D], and for diag the tangent J_N [M, D]
int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const bool diag = !strcmp(argv[1], "diag"), two = !strcmp(argv[1], "heston2");
  const int M = atoi(argv[2]), N = atoi(argv[3]), nb = atoi(argv[4]);
  const int k = two ? nb / 2 : nb, D = diag ? nb : 2 * k;
  const std::vector<float> c = rdn(diag ? 3 : (two ? 6 : 5));
  const std::vector<float> t = rdn(N + 1), xi = rdn((size_t)M * D), dw = rdn((size_t)M * N * nb);
  std::vector<float> X((size_t)M * (N + 1) * D), sdw((size_t)M * N * D), J((size_t)M * D, 1.0f);
  for (int m = 0; m < M; ++m) {
    std::vector<float> x(xi.begin() + (size_t)m * D, xi.begin() + (size_t)(m + 1) * D);
    for (int n = 0; n <= N; ++n) {
      float* Xr = &X[((size_t)m * (N + 1) + n) * D];
      for (int d = 0; d < D; ++d) Xr[d] = x[d];
      if (n == N) break;
      const float dt = rn_sub(t[n + 1], t[n]);
      const float* w = &dw[((size_t)m * N + n) * nb];
      float* s = &sdw[((size_t)m * N + n) * D];
      if (diag) {
        for (int d = 0; d < D; ++d) {
          s[d] = diag_step(c[0], c[1], c[2], dt, w[d], x[d]);
          diag_tangent_step(c[0], c[1], dt, w[d], J[(size_t)m * D + d]);
        }
      } else {
        for (int i = 0; i < k; ++i) {
          if (two)
            heston2_step(c[0], c[1], c[2], c[3], c[4], c[5], dt, w[i], w[k + i], x[i], x[k + i], s[i], s[k + i]);
          else
            heston_step(heston_coef(c[0], c[1], c[2], c[3], c[4], x[i], x[k + i]), dt, w[i], x[i], x[k + i], s[i],
                        s[k + i]);
        }
      }
    }
  }
  put(X);
  put(sdw);
  if (diag) put(J);
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("sde_step")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    # no HIP include path: the header must be plain C++ here
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def run(driver, kind, nb, coef, Xi, dw):
    """(X [M, N+1, D], sdw [M, N, D], rest) float32 of the compiled steps."""
    D = nb if kind == "diag" else (nb if kind == "heston2" else 2 * nb)
    words = [np.asarray(a, f32).ravel() for a in (coef, ph.time_grid(N, T), np.broadcast_to(Xi, (M, D)), dw)]
    text = " ".join(float(v).hex() for v in np.concatenate(words))
    out = subprocess.run([driver, kind, str(M), str(N), str(nb)], input=text, capture_output=True, text=True, check=True)
    vals = np.array([float.fromhex(w) for w in out.stdout.split()], np.float64)
    got = vals.astype(f32)
    assert np.array_equal(got.astype(np.float64), vals)          # every printed value is an fp32
    nx, ns = M * (N + 1) * D, M * N * D
    return got[:nx].reshape(M, N + 1, D), got[nx:nx + ns].reshape(M, N, D), got[nx + ns:]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("mu_a,sig_a,sig_b", [(0.0, 0.4, 0.0), (0.05, 0.2, 0.1)], ids=["bsb", "sig_b"])
def test_diagonal_step_and_tangent(driver, mu_a, sig_a, sig_b):
    D = D_DIAG
    Xi = np.linspace(0.5, 1.5, D).astype(f32)[None, :]
    dw = ph.increments(SEED, 0, 0, M, N, D, T)
    X, sdw, J = run(driver, "diag", D, [mu_a, sig_a, sig_b], Xi, dw)
    ref = ph.rollout(Xi, dw, T, mu_a, sig_a, sig_b)
    np.testing.assert_array_equal(bits(X), bits(ref))
    np.testing.assert_array_equal(bits(sdw), bits((f32(sig_a) * ref[:, :-1] + f32(sig_b)) * dw))   # rollout's s
    np.testing.assert_array_equal(bits(J.reshape(M, D)), bits(mr.tangent(dw, T, mu_a, sig_a)))
    assert sig_b == 0.0 or np.any(bits(sdw) != bits((f32(sig_a) * ref[:, :-1]) * dw))              # sig_b is felt


# assets: ordinary; the Sigma clamp on sv S and rho sv S; the drift clamp on mu_a S; the clamps on kappa (theta -
# v), sigma sv and its rho / rhob multiples; the variance floor
HESTON_XI = np.array([[1.0, 300.0, 3000.0, 1.0, 1.0, 0.2, 0.2, 0.2, 2e6, 1e-9]], f32)
HESTON_COEF = dict(mu_a=0.05, kappa=2.0, theta=0.2, sigma=0.3, rho=0.8)


def assert_oracle_hits_clamps_and_floor(X, second):
    """Every clamped entry exceeds 100 in magnitude somewhere on the oracle's own
    path, and the floor is active; second: the multipliers of sigma sv."""
    k = K_HESTON
    S, v = X[:, :-1, :k], X[:, :-1, k:]
    c = {n: f32(x) for n, x in HESTON_COEF.items()}
    sv = np.sqrt(np.maximum(v, f32(1e-8)))
    assert np.any(v < f32(1e-8)), "variance floor"
    assert np.any(c["mu_a"] * S > 100), "muS clamp"
    assert np.any(c["kappa"] * (c["theta"] - v) < -100), "muV clamp"
    assert np.any(sv * S > 100), "d00 clamp"
    for name, mult in second.items():
        assert np.any(mult > 100), name + " clamp"


def test_one_factor_heston_step(driver):
    k = K_HESTON
    dw = ph.increments(SEED, 0, 0, M, N, k, T)
    c = HESTON_COEF
    X, sdw, _ = run(driver, "heston", k, [c["mu_a"], c["kappa"], c["theta"], c["sigma"], c["rho"]], HESTON_XI, dw)
    Xr, sr = ph.heston_rollout(HESTON_XI, dw, T, **c)
    np.testing.assert_array_equal(bits(X), bits(Xr))
    np.testing.assert_array_equal(bits(sdw), bits(sr))
    sv = np.sqrt(np.maximum(Xr[:, :-1, k:], f32(1e-8)))
    sS, sV = sv * Xr[:, :-1, :k], f32(c["sigma"]) * sv
    assert_oracle_hits_clamps_and_floor(Xr, {"d01": f32(c["rho"]) * sV, "d10": f32(c["rho"]) * sS, "d11": sV})


def test_two_factor_heston_step(driver):
    k = K_HESTON
    dw = ph.increments(SEED, 0, 0, M, N, 2 * k, T)
    c = HESTON_COEF
    rb = h2.rhobar(c["rho"])
    X, sdw, _ = run(driver, "heston2", 2 * k, [c["mu_a"], c["kappa"], c["theta"], c["sigma"], c["rho"], rb], HESTON_XI, dw)
    Xr, sr = h2.rollout(HESTON_XI, dw, T, **c)
    np.testing.assert_array_equal(bits(X), bits(Xr))
    np.testing.assert_array_equal(bits(sdw), bits(sr))
    sV = f32(c["sigma"]) * np.sqrt(np.maximum(Xr[:, :-1, k:], f32(1e-8)))
    assert_oracle_hits_clamps_and_floor(Xr, {"d10": f32(c["rho"]) * sV, "d11": rb * sV})
