"""The reference side of tests/test_gpu_depths.py, on the CPU: every case of
tests/depth_cases.py has a tight reference (the fp32 oracle within 5 % of each
bound from its fp64 twin), every used parameter tensor has a gradient to be
compared with, and the package's own torch networks reproduce the oracle's
layout and init at every depth.  No GPU."""
from importlib import import_module

import numpy as np
import pytest
import torch

import depth_cases as dc
from conftest import load_pkg
from oracle import fbsnn_ref as fr

MARGIN = 0.05


@pytest.mark.parametrize("case", list(dc.CASES))
def test_fp32_oracle_is_within_5_percent_of_each_bound_from_fp64(case):
    b = dc.reference(case)
    np.testing.assert_array_equal(b["ref32"]["used"], b["ref64"]["used"])
    e = dc.errors(b["ref32"], b["ref64"], b["tensors"])
    print(f"{case}: fp32 vs fp64 oracle, error / bound: " + ", ".join(
        f"{k} {v:.3g}" for k, v in e.items() if not isinstance(v, str)) + f" ({e['tensor_name']})")
    xr = np.abs(b["ref32"]["X"] - b["ref64"]["X"]).max() / np.abs(b["ref64"]["X"]).max()
    assert xr < 1e-5, xr
    for k in ("loss", "Y", "Z", "grad", "tensor"):
        assert e[k] <= MARGIN, (case, k, e[k])


@pytest.mark.parametrize("case", list(dc.CASES))
def test_every_used_tensor_has_a_gradient(case):
    """Nothing is compared against a zero reference, and `used` leaves out
    exactly NAIS-Net's input_layers[K]."""
    b = dc.reference(case)
    K = dc.depth(case)
    unused = {f"input_layers.{K}.weight", f"input_layers.{K}.bias"} if dc.CASES[case]["mode"] == "NAIS-Net" else set()
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


@pytest.mark.parametrize("case", list(dc.CASES))
def test_make_model_reproduces_the_oracle_layout_and_init(case):
    """networks.make_model: the same state_dict keys, shapes and order as the
    oracle's build_model and, after the same torch.manual_seed, the same values
    bit for bit."""
    c = dc.CASES[case]
    nets = import_module(load_pkg().__name__ + ".networks")
    seed = dc.state_dim(case) + len(c["layers"])
    torch.manual_seed(seed)
    want = fr.build_model(c["mode"], c["layers"], c["act"]).state_dict()
    torch.manual_seed(seed)
    got = nets.make_model(c["mode"], c["layers"], c["act"]).state_dict()
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k], want[k]), k
