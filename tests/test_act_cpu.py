"""SiLU and Softplus on the CPU: the scalar functions of csrc/act.hpp compiled
as plain host C++ against fp64 numpy, and the reference side of
tests/test_gpu_act.py (tests/act_cases.py): every case has a tight reference,
every used parameter tensor a gradient to be compared with, the package's own
torch networks reproduce the swapped oracle's layout and initialisation, and
the saturated cases do saturate.  No GPU.

Measured when written (host build, g++ -O2 -ffp-contract=off, 420,002 grid
points of [-100, 100] plus 40,001 of [-1, 1]): max error / max(1, |ref|)
  SiLU      f 1.39e-07   f' 1.60e-07   f'' 1.35e-07
  Softplus  f 9.79e-08   f' 8.87e-08   f'' 5.43e-08
against the bound 2e-6, the project's fp32 ATOL."""
import os
import subprocess
from importlib import import_module

import numpy as np
import pytest
import torch

import act_cases as ac
import depth_cases as dc
from conftest import PKG_NAME, ROOT, load_pkg

CSRC = os.path.join(ROOT, PKG_NAME, "csrc")
ATOL = 2e-6
MARGIN = 0.05

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include "act.hpp"
#ifdef __HIPCC__
#error "this driver is the plain host C++ build of act.hpp"
#endif
using namespace dbsde;

// stdin: fp32 arguments as hex floats; stdout per argument:
// silu f f' f'' (from silu_v1 and silu_12), softplus f f' f'', and the
// single-result forms silu_f silu_1 softplus_f softplus_1
int main() {
  char b[64];
  while (scanf("%63s", b) == 1) {
    const float a = strtof(b, nullptr);
    float f, d, d1, d2, g, e, e1, e2;
    silu_v1(a, f, d);
    silu_12(a, d1, d2);
    softplus_v1(a, g, e);
    softplus_12(a, e1, e2);
    if (d != d1 || e != e1) return 3;   // one definition of f' behind both forms
    printf("%a %a %a %a %a %a %a %a %a %a\n", (double)f, (double)d1, (double)d2, (double)g, (double)e1, (double)e2,
           (double)silu_f(a), (double)silu_1(a), (double)softplus_f(a), (double)softplus_1(a));
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """(a [n] fp32, got [n, 10] fp32) of the compiled header over the grid."""
    d = tmp_path_factory.mktemp("act")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    # no HIP include path: the header must be plain C++ here
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    a = np.concatenate([np.linspace(-100.0, 100.0, 420002), np.linspace(-1.0, 1.0, 40001),
                        [0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0, 104.0, -104.0, 3e38, -3e38]]).astype(np.float32)
    text = "\n".join(float(v).hex() for v in a)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout
    vals = np.array([float.fromhex(w) for w in out.split()], np.float64).reshape(len(a), 10)
    assert np.array_equal(vals.astype(np.float32).astype(np.float64), vals)     # every printed value is an fp32
    return a, vals


def fp64_reference(a):
    """f, f', f'' of SiLU and Softplus in fp64, overflow-free."""
    a = a.astype(np.float64)
    s = np.where(a >= 0, 1.0 / (1.0 + np.exp(-np.abs(a))), np.exp(-np.abs(a)) / (1.0 + np.exp(-np.abs(a))))
    q = np.exp(-np.abs(a)) / (1.0 + np.exp(-np.abs(a))) ** 2
    return {"SiLU": (a * s, s + a * q, q * (2.0 + a * (1.0 - 2.0 * s))),
            "Softplus": (np.maximum(a, 0.0) + np.log1p(np.exp(-np.abs(a))), s, q)}


def test_fp64_reference_is_torch(table):
    """The numpy restatement above against torch's own SiLU / Softplus and
    their autograd derivatives in fp64 (Softplus with torch's threshold out of
    the way: the smooth form everywhere), and the threshold note of DESIGN
    3.10: at 20 the two differ by 2.1e-9."""
    a = torch.linspace(-100.0, 100.0, 2001, dtype=torch.float64, requires_grad=True)
    ref = fp64_reference(a.detach().numpy())
    for name, fn in (("SiLU", torch.nn.SiLU()), ("Softplus", torch.nn.Softplus(threshold=1e9))):
        f = fn(a)
        d1, = torch.autograd.grad(f.sum(), a, create_graph=True)
        d2, = torch.autograd.grad(d1.sum(), a)
        for got, want in zip(ref[name], (f, d1, d2)):
            np.testing.assert_allclose(got, want.detach().numpy(), rtol=1e-12, atol=1e-14)
    x = torch.tensor([20.0 + 1e-9], dtype=torch.float64)
    gap = float(torch.nn.Softplus(threshold=1e9)(x) - torch.nn.Softplus()(x))
    assert 2.0e-9 < gap < 2.2e-9, gap


def test_scalar_functions_against_fp64(table):
    a, got = table
    ref = fp64_reference(a)
    assert np.all(np.isfinite(got)), "a value is not finite"
    cols = {"SiLU": (0, 1, 2), "Softplus": (3, 4, 5)}
    for name, (f, d1, d2) in ref.items():
        worst = []
        for k, want in zip(cols[name], (f, d1, d2)):
            err = np.abs(got[:, k] - want) / np.maximum(1.0, np.abs(want))
            worst.append(float(err.max()))
            assert err.max() <= ATOL, (name, k, float(err.max()), float(a[err.argmax()]))
        print(f"{name}: max error / max(1, |ref|): f {worst[0]:.2e}, f' {worst[1]:.2e}, f'' {worst[2]:.2e} (bound {ATOL:.0e})")
    # the single-result forms are the same numbers
    for k, j in ((6, 0), (7, 1), (8, 3), (9, 4)):
        np.testing.assert_array_equal(got[:, k], got[:, j])
    # the tails are exact: nothing is left of e beyond |a| = 104
    hi, lo = a >= 104.0, a <= -104.0
    assert hi.any() and lo.any()
    assert np.all(got[hi | lo][:, [2, 5]] == 0.0)
    assert np.all(got[hi][:, [1, 4]] == 1.0) and np.all(got[lo][:, [0, 1, 3, 4]] == 0.0)
    np.testing.assert_array_equal(got[hi][:, 0], a[hi])
    np.testing.assert_array_equal(got[hi][:, 3], a[hi])


@pytest.mark.parametrize("case", list(ac.CASES))
def test_fp32_oracle_is_within_5_percent_of_each_bound_from_fp64(case):
    b = ac.reference(case)
    np.testing.assert_array_equal(b["ref32"]["used"], b["ref64"]["used"])
    e = dc.errors(b["ref32"], b["ref64"], b["tensors"])
    print(f"{case}: fp32 vs fp64 oracle, error / bound: " + ", ".join(
        f"{k} {v:.3g}" for k, v in e.items() if not isinstance(v, str)) + f" ({e['tensor_name']})")
    xr = np.abs(b["ref32"]["X"] - b["ref64"]["X"]).max() / np.abs(b["ref64"]["X"]).max()
    assert xr < 1e-5, xr
    for k in ("loss", "Y", "Z", "grad", "tensor"):
        assert e[k] <= MARGIN, (case, k, e[k])


@pytest.mark.parametrize("case", list(ac.CASES))
def test_every_used_tensor_has_a_gradient(case):
    b = ac.reference(case)
    K = ac.depth(case)
    unused = {f"input_layers.{K}.weight", f"input_layers.{K}.bias"} if ac.CASES[case]["mode"] == "NAIS-Net" else set()
    for ref in (b["ref32"], b["ref64"]):
        for name, off, n in b["tensors"]:
            u = ref["used"][off:off + n]
            assert u.all() or not u.any(), name
            assert (not u.any()) == (name in unused), name
            if u.all():
                assert np.abs(ref["grad"][off:off + n]).max() > 0, name
            else:
                assert np.all(ref["grad"][off:off + n] == 0), name
    assert np.isfinite(b["ref64"]["loss"]) and b["ref64"]["loss"] > 0


@pytest.mark.parametrize("case", list(ac.CASES))
def test_make_model_reproduces_the_swapped_oracle(case):
    """networks.make_model(mode, layers, "SiLU" / "Softplus"): the swapped
    oracle's state_dict keys, shapes, order and, after the same seed, values bit
    for bit; and the same function (one forward on the case's first rows)."""
    c = ac.CASES[case]
    nets = import_module(load_pkg().__name__ + ".networks")
    want_model = ac.build(case)
    torch.manual_seed(c["seed"] if c["seed"] is not None else ac.state_dim(case) + len(c["layers"]))
    got_model = nets.make_model(c["mode"], c["layers"], c["act"])
    want, got = want_model.state_dict(), got_model.state_dict()
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k], want[k]), k
    x = torch.linspace(-2.0, 2.0, 5 * c["layers"][0]).reshape(5, c["layers"][0])
    with torch.no_grad():
        assert torch.equal(got_model(x), want_model(x))
    acts = [m for m in got_model.modules() if isinstance(m, tuple(ac.TORCH_ACT.values()))]
    assert acts and all(type(m) is ac.TORCH_ACT[c["act"]] for m in acts)


@pytest.mark.parametrize("layout", ac.SAT_LAYOUTS)
@pytest.mark.parametrize("act", ac.ACTS)
def test_saturated_cases_span_60(layout, act):
    """The saturated twin's first pre-activation reaches beyond +-60 on the
    oracle, its reference stays finite, within 5 % of each bound between fp32
    and fp64, and every used tensor keeps a gradient."""
    case = f"{layout}-{act}"
    b = ac.reference(case, sat=True)
    a0 = ac.first_preactivation(b["model"], b["tt"], b["Wt"], b["Xit"], case)
    print(f"{case}: a_0 spans [{a0.min():.1f}, {a0.max():.1f}]")
    assert a0.min() <= -ac.SAT_SPAN and a0.max() >= ac.SAT_SPAN
    for ref in (b["ref32"], b["ref64"]):
        assert all(np.all(np.isfinite(ref[k])) for k in ("loss", "Y", "Z", "grad"))
    e = dc.errors(b["ref32"], b["ref64"], b["tensors"])
    print(f"{case} saturated: fp32 vs fp64 oracle, error / bound: " + ", ".join(
        f"{k} {v:.3g}" for k, v in e.items() if not isinstance(v, str)) + f" ({e['tensor_name']})")
    for k in ("loss", "Y", "Z", "grad", "tensor"):
        assert e[k] <= MARGIN, (case, k, e[k])
    for name, off, n in b["tensors"]:
        if b["ref64"]["used"][off]:
            assert np.abs(b["ref64"]["grad"][off:off + n]).max() > 0, name
