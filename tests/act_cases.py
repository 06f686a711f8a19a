"""SiLU and Softplus in every kernel family -- test infrastructure only, in
the manner of tests/depth_cases.py, whose spec_for, tensors, errors, check,
BOUNDS, batch (M = 20, N = 3: 80 rows, ragged against every row tile) and
seeding it reuses.

The oracle (oracle/fbsnn_ref.py) knows the reference's three activations.  A
case's oracle model is built with "Tanh" and its activation module swapped for
torch's nn.SiLU / nn.Softplus (beta = 1): `model.act` on ResnetRef / NaisnetRef,
the nn.Tanh entries of the FC Sequential.  The activation holds no parameters
and draws no random numbers, so layout and initialisation are the oracle's own.

LAYOUTS are the smallest layouts that select each kernel family; every layout
is a case for each of the two activations ("<layout>-SiLU", "<layout>-Softplus").
The columns fused / form are what a Tanh solver of the same layout reports
(csrc/step.hip kFused holds, for each new activation, the instances tanh has;
none was left to the chain):

  layout             network                               kernel family
  nais16_K1, _K3     NAIS-Net width 16                     fused fp32
  fc16_K2            FC width 16                           fused fp32, no x-stack
  nais110_K3         NAIS-Net [101] + 4 [110] + [1], bsb   fused split-bf16 and column-split (the headline layout)
  naisnet110_K3      Naisnet, same widths, call            fused split-bf16 and column-split
  resnet110_K3       Resnet, same widths                   fused split-bf16, no x-stack
  fc256_K3           FC [101] + 4 [256] + [1], hjb         phase2.hip (M = 16, N = 2)
  nais110_K2         NAIS-Net width 110, K = 2             per-layer chain, fp32
  fc256_K1           FC width 256, K = 1                   per-layer chain, split-bf16
  fc_d200_64_32_16   FC, D = 200                           wide Z GEMM

cs: DBSDE_CS=1 selects the column-split phase kernels at M = 20 (width 110,
K = 3).  Seeds: torch.manual_seed(D + len(layers)) as in depth_cases; a case
that missed the 5 % condition of tests/test_act_cpu.py would get another seed
here (`seed`), never another margin.  Saturation: SAT_CASES with the input
layer's weight scaled by SAT_SCALE, so that the oracle's first pre-activation
spans at least +-60 (asserted on the CPU)."""
from __future__ import annotations

import copy

import numpy as np
import torch
from torch import nn

import depth_cases as dc
from oracle import fbsnn_ref as fr

ACTS = ("SiLU", "Softplus")
TORCH_ACT = {"SiLU": nn.SiLU, "Softplus": nn.Softplus}


def _layout(mode, problem, layers, fused, tnw, form, M=dc.M, N=dc.N, cs=False, seed=None):
    return dict(mode=mode, problem=problem, layers=list(layers), fused=fused, tnw=tnw, form=form, M=M, N=N, cs=cs,
                scale0=False, seed=seed)


W110 = [101] + 4 * [110] + [1]
LAYOUTS = {
    "nais16_K1": _layout("NAIS-Net", "bsb", [15] + 2 * [16] + [1], True, True, 0),
    "nais16_K3": _layout("NAIS-Net", "bsb", [15] + 4 * [16] + [1], True, True, 0),
    "fc16_K2": _layout("FC", "bspde_test", [9] + 3 * [16] + [1], True, False, 2),
    "nais110_K3": _layout("NAIS-Net", "bsb", W110, True, True, 3, cs=True),
    "naisnet110_K3": _layout("Naisnet", "call", W110, True, True, 3, cs=True),
    "resnet110_K3": _layout("Resnet", "bsb", W110, True, False, 3, cs=True),
    "fc256_K3": _layout("FC", "hjb", [101] + 4 * [256] + [1], True, False, 3, M=16, N=2),
    "nais110_K2": _layout("NAIS-Net", "bsb", [101] + 3 * [110] + [1], False, False, 0),
    "fc256_K1": _layout("FC", "hjb", [101] + 2 * [256] + [1], False, False, 6, M=16, N=2),
    "fc_d200_64_32_16": _layout("FC", "bsb", [201, 64, 32, 16, 1], False, False, 0),
}
CASES = {f"{name}-{act}": dict(lay, act=act, layout=name) for name, lay in LAYOUTS.items() for act in ACTS}

NETU_LAYOUTS = ("nais16_K1", "nais110_K3", "fc256_K1", "fc_d200_64_32_16")
SAT_LAYOUTS = ("nais16_K1", "nais110_K3")
SAT_SPAN = 60.0
SAT_SCALE = {"nais16_K1": 40.0, "nais110_K3": 40.0}


def depth(case):
    return len(CASES[case]["layers"]) - 3


def state_dim(case):
    return CASES[case]["layers"][0] - 1


def swap_activation(model, act):
    """The oracle model with its activation module replaced (in place)."""
    new = TORCH_ACT[act]()
    if isinstance(model, nn.Sequential):
        n = 0
        for k, m in enumerate(model):
            if isinstance(m, nn.Tanh):
                model[k] = new
                n += 1
        assert n == len(model) // 2
    else:
        assert isinstance(model.act, nn.Tanh)
        model.act = new
    return model


def build(case, sat=False):
    """The case's oracle model; NAIS cases keep depth_cases' guard that no
    projected block's |W^T W|_F sits near the projection branch."""
    c = CASES[case]
    torch.manual_seed(c["seed"] if c["seed"] is not None else state_dim(case) + len(c["layers"]))
    model = swap_activation(fr.build_model(c["mode"], c["layers"], "Tanh"), c["act"])
    if c["mode"] in ("NAIS-Net", "Naisnet"):
        sd = model.state_dict()
        blocks = dc.hidden_blocks(model, c["layers"][1])
        assert len(blocks) == depth(case)
        for name in blocks:
            w = sd[name].double()
            nrm = float(torch.norm(w.t() @ w))
            assert nrm < 0.9 or nrm > 1.1, (case, name, nrm)
    if sat:
        with torch.no_grad():
            first = next(iter(model.state_dict().values()))   # the input layer's weight
            assert first.shape == (c["layers"][1], c["layers"][0])
            first.mul_(SAT_SCALE[c["layout"]])
    return model


def first_preactivation(model, t, W, Xi, case):
    """a_0 = W_in [t, X] + b_in of the oracle over the case's batch, fp64."""
    c = CASES[case]
    D = state_dim(case)
    m = copy.deepcopy(model).double()
    prob = fr.make_problem(c["problem"], D)
    X = np.asarray(fr.loss_and_grads(m, prob, t.double(), W.double(), Xi.double(), c["M"], D)["X"], np.float64)
    tt = t.double().numpy().reshape(c["M"], c["N"] + 1, 1)
    x = torch.from_numpy(np.concatenate([tt, X], axis=2).reshape(-1, D + 1))
    sd = m.state_dict()
    w, b = list(sd.values())[0], list(sd.values())[1]
    return (x @ w.t() + b).numpy()


def batch(case):
    c = CASES[case]
    D = state_dim(case)
    t, W = fr.fetch_minibatch(c["M"], c["N"], D, dc.T, rng=np.random.RandomState(7))
    return t, W, torch.ones((1, D), dtype=torch.float32)


def _run(model, case, t, W, Xi):
    c = CASES[case]
    D = state_dim(case)
    return fr.loss_and_grads(model, fr.make_problem(c["problem"], D), t, W, Xi, c["M"], D)


_REFS = {}


def reference(case, sat=False):
    """dict(model, params, tensors, t, W, Xi as numpy, ref32, ref64) of a case
    (depth_cases.reference's bundle), computed once per process; sat: the
    saturated twin."""
    key = (case, sat)
    if key not in _REFS:
        c = CASES[case]
        model = build(case, sat)
        t, W, Xi = batch(case)
        ref32 = _run(model, case, t, W, Xi)
        ref64 = _run(copy.deepcopy(model).double(), case, t.double(), W.double(), Xi.double())
        _REFS[key] = dict(model=model, params=fr.flat_params(model), tensors=dc.tensors(model), M=c["M"], N=c["N"],
                          t=t.squeeze(-1).numpy(), W=W.numpy(), Xi=Xi.numpy(), ref32=ref32, ref64=ref64,
                          tt=t, Wt=W, Xit=Xi)
    return _REFS[key]
