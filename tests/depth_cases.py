"""Networks at every supported depth (K = len(layers) - 3 hidden blocks, 1..6;
Naisnet 1..3) and FC networks with unequal hidden widths -- test
infrastructure only: the case table, and per case the oracle model
(oracle/fbsnn_ref.py), its flat parameters, one batch and the oracle's loss and
gradients in fp32 and in fp64, each computed once per process and never
changed by a test.

Depth is not a loop count in the engine; it selects kernels, buffers and
tables (csrc/net.hip build_net / build_buffers, csrc/step.hip kFused,
launch_tnw, tn_setup):

  fused     the fused phase kernels exist for K = 3 at widths 112 and 256 and
            for K = 1, 2, 3 at width 16; every other layout runs the per-layer
            chain (fp32, or split-bf16 chainx3 for uniform FC / Resnet)
  tnw       wave-owned weight-gradient tiles: NAIS layouts with Wp == Dp <= 128
            and (2K + 2) % 4 == 0, i.e. K = 1, 3, 5 with P = 4, 8, 12 problems;
            the other depths run the split-K TN GEMM (K = 6 fills its 8 problem
            slots)
  form      NativeSolver.matrix_form: bit 0 the fused phase kernels in
            split-bf16 form, bit 1 the weight-gradient tiles in split-bf16 form
            (tn_x3), bit 2 the split-bf16 chain (chainx3)
  unequal   FC hidden widths that differ select the plain fp32 chain with a
            column offset, padded width and slab shape per level; widths above
            128 pad to multiples of 128

The columns fused / tnw / form of CASES are what that code selects for the
default environment; tests/test_gpu_depths.py asserts all three on the device
(tnw through dbsde_train_step, which folds the update into the finalize only
on that layout; the DBSDE_TNW=0 variant runs the other kernel on the same
case).

M = 20, N = 3 gives 80 rows, ragged against every row tile (16, 32, 64).
Seeds: torch.manual_seed(D + len(layers)) before build_model; the batch is
fetch_minibatch(M, N, D, 1.0, rng=RandomState(7)), Xi = ones((1, D)).

ReLU is left out, as in tests/test_gpu_nais_wide.py: its kinks flip between
summation orders.  The ReLU instances of the fused kernels at K = 1, 2
therefore stay without a reference.

Bounds (tests/test_gpu_parity.py, tests/test_gpu_nais_wide.py): loss rel 1e-4,
Y / Z abs 1e-4 max(1, |ref|max), gradient abs 2e-4 max|ref grad| globally and,
per parameter tensor, abs 2e-4 max|ref grad of that tensor| -- the smallest
per-tensor maximum is 2.2e-2 of the global one (nais110 K = 6), so the global
bound alone would pass an error 45 times the per-tensor bound there.  The
reference is the fp64 oracle; tests/test_depth_reference_cpu.py holds the fp32
oracle within 5 % of each bound from it (measured: loss 1.9e-7 rel, Y 8.1e-7,
Z 4.9e-7, gradient 4.9e-7 global and 6.6e-7 per tensor, under 1 % of each).
"""
from __future__ import annotations

import copy

import numpy as np
import torch

from oracle import fbsnn_ref as fr

T = 1.0
M, N = 20, 3
BOUNDS = dict(loss=1e-4, Y=1e-4, Z=1e-4, grad=2e-4, tensor=2e-4)


def _case(mode, act, problem, layers, fused, tnw, form, M=M, N=N, scale0=False):
    return dict(mode=mode, act=act, problem=problem, layers=list(layers), fused=fused, tnw=tnw, form=form, M=M, N=N,
                scale0=scale0)


def _table():
    c = {}
    for K in range(1, 7):
        lay = (K + 1) * [16]
        # NAIS-Net width 16 (Dp = Wp = 16): fused at K <= 3, tnw at odd K; the
        # hidden weight of block 0 scaled by 0.2 at K = 2 and K = 5 so that the
        # not-projected branch occurs
        c[f"nais16_K{K}"] = _case("NAIS-Net", "Sine", "bsb", [15] + lay + [1], K <= 3, K % 2 == 1, 0,
                                  scale0=K in (2, 5))
        # FC / Resnet width 16: fused without the x-stack at K <= 3 with tn_x3
        # weight gradients, chainx3 at K >= 4
        c[f"fc16_K{K}"] = _case("FC", "Tanh", "bspde_test", [9] + lay + [1], K <= 3, False, 2 if K <= 3 else 6)
        c[f"resnet16_K{K}"] = _case("Resnet", "Sine", "bsb", [9] + lay + [1], K <= 3, False, 2 if K <= 3 else 6)
    for K in (1, 2, 5, 6):
        # fp32 chain; fp32 tnw with 7-block tiles at K = 1 (P = 4), K = 5 (P = 12)
        c[f"nais110_K{K}"] = _case("NAIS-Net", "Sine", "bsb", [101] + (K + 1) * [110] + [1], False, K % 2 == 1, 0)
    for K in (1, 2):
        c[f"naisnet110_K{K}"] = _case("Naisnet", "Tanh", "call", [101] + (K + 1) * [110] + [1], False, K % 2 == 1, 0)
    for K in (1, 2, 4, 6):
        # chainx3 at Wp = 256 (the fused width-256 kernels are K = 3 only)
        c[f"fc256_K{K}"] = _case("FC", "Sine", "hjb", [101] + (K + 1) * [256] + [1], False, False, 6, M=16, N=2)
    # FC with unequal hidden widths: the plain fp32 chain
    c["fc_48_32_16"] = _case("FC", "Tanh", "bspde_test", [9, 48, 32, 16, 1], False, False, 0)
    c["fc_16_64_32_48"] = _case("FC", "Sine", "bsb", [9, 16, 64, 32, 48, 1], False, False, 0)
    c["fc_33_20_130_7"] = _case("FC", "Tanh", "basket", [21, 33, 20, 130, 7, 1], False, False, 0)   # 130 pads to 256
    c["fc_16_to_112"] = _case("FC", "Sine", "bsb", [9, 16, 32, 48, 64, 80, 96, 112, 1], False, False, 0)   # K = 6
    c["fc_d200_64_32_16"] = _case("FC", "Sine", "bsb", [201, 64, 32, 16, 1], False, False, 0)   # Dp > 128: wide Z GEMM
    return c


CASES = _table()

# the K != 3 chunk pipeline (tests/test_gpu_depths.py): case -> (M, N)
CHUNK_CASES = {"nais16_K1": (128, 3), "fc16_K2": (128, 3)}
# net_u, net_u_xvjp and net_u_jet
NETU_CASES = ("nais16_K1", "nais16_K6", "nais110_K5", "fc256_K1", "fc_33_20_130_7", "fc_16_to_112")


def depth(case):
    return len(CASES[case]["layers"]) - 3


def state_dim(case):
    return CASES[case]["layers"][0] - 1


def spec_for(pkg, problem, D):
    """The ProblemSpec of an oracle problem (tests/test_gpu_parity.py spec_for)."""
    S = pkg.ProblemSpec
    return {
        "bsb": S(sig_a=0.4, phi_r=0.05, phi_c=1.0, g="sumsq"),
        "bspde_test": S(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=1.0, g="sumsq"),
        "call": S(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=1.0, g="call_sum", strike=1.0 * D),
        "basket": S(mu_a=0.05, sig_a=0.2, phi_r=0.05, phi_c=0.0, g="call_mean", strike=1.0),
        "hjb": S(sig_b=float(np.sqrt(2.0)), phi_zz=1.0, g="log"),
    }[problem]


def hidden_blocks(model, L):
    """Names of the projected L x L hidden weights, in state_dict order."""
    return [n for n, p in model.state_dict().items()
            if n.endswith(".weight") and "input" not in n and tuple(p.shape) == (L, L)]


def tensors(model):
    """(name, offset, numel) of every parameter tensor in the flat vector."""
    out, off = [], 0
    for name, p in model.state_dict().items():
        out.append((name, off, p.numel()))
        off += p.numel()
    return out


def build(case):
    """The case's oracle model.  NAIS cases assert that no projected block's
    |W^T W|_F sits near the projection branch (0.98): below 0.9 or above 1.1."""
    c = CASES[case]
    torch.manual_seed(state_dim(case) + len(c["layers"]))
    model = fr.build_model(c["mode"], c["layers"], c["act"])
    if c["mode"] in ("NAIS-Net", "Naisnet"):
        sd = model.state_dict()
        blocks = hidden_blocks(model, c["layers"][1])
        assert len(blocks) == depth(case)
        with torch.no_grad():
            for k, name in enumerate(blocks):
                if k == 0 and c["scale0"]:
                    sd[name].mul_(0.2)
                w = sd[name].double()
                nrm = float(torch.norm(w.t() @ w))
                assert nrm < 0.9 or nrm > 1.1, (case, name, nrm)
                if c["scale0"]:
                    assert (nrm < 0.9) == (k == 0), (case, name, nrm)
    return model


def batch(case, M=None, N=None):
    """(t [M, N+1, 1], W [M, N+1, D], Xi [1, D]) as torch float32."""
    c = CASES[case]
    D = state_dim(case)
    t, W = fr.fetch_minibatch(M or c["M"], N or c["N"], D, T, rng=np.random.RandomState(7))
    return t, W, torch.ones((1, D), dtype=torch.float32)


def _run(model, case, t, W, Xi, M):
    D = state_dim(case)
    return fr.loss_and_grads(model, fr.make_problem(CASES[case]["problem"], D), t, W, Xi, M, D)


_REFS = {}


def reference(case, M=None, N=None):
    """dict(model, params, tensors, t, W, Xi as numpy, ref32, ref64) of a case
    at its own (M, N) or the given one; ref64 is the oracle on
    copy.deepcopy(model).double() with double t, W, Xi."""
    c = CASES[case]
    M, N = M or c["M"], N or c["N"]
    key = (case, M, N)
    if key not in _REFS:
        model = build(case)
        t, W, Xi = batch(case, M, N)
        ref32 = _run(model, case, t, W, Xi, M)
        ref64 = _run(copy.deepcopy(model).double(), case, t.double(), W.double(), Xi.double(), M)
        _REFS[key] = dict(model=model, params=fr.flat_params(model), tensors=tensors(model), M=M, N=N,
                          t=t.squeeze(-1).numpy(), W=W.numpy(), Xi=Xi.numpy(), ref32=ref32, ref64=ref64)
    return _REFS[key]


def errors(got, ref, tens):
    """Each checked quantity's max error divided by its bound: loss, Y, Z,
    grad (global) and tensor (the worst parameter tensor, with its name)."""
    out = {}
    out["loss"] = abs(float(np.ravel(got["loss"])[0]) - ref["loss"]) / (BOUNDS["loss"] * abs(ref["loss"]))
    for k in ("Y", "Z"):
        a, b = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        out[k] = float(np.abs(a - b).max()) / (BOUNDS[k] * max(1.0, float(np.abs(b).max())))
    if "grad" in got:
        used = ref["used"]
        g, gr = np.asarray(got["grad"], np.float64), np.asarray(ref["grad"], np.float64)
        out["grad"] = float(np.abs(g - gr)[used].max()) / (BOUNDS["grad"] * float(np.abs(gr).max()))
        worst, who = 0.0, None
        for name, off, n in tens:
            if not used[off]:
                continue
            top = float(np.abs(gr[off:off + n]).max())
            assert top > 0, name
            e = float(np.abs(g[off:off + n] - gr[off:off + n]).max()) / (BOUNDS["tensor"] * top)
            if who is None or e > worst:
                worst, who = e, name
        out["tensor"], out["tensor_name"] = worst, who
    return out


def check(got, b, what=""):
    """got against the fp64 oracle of bundle b with BOUNDS; X bit-equal to the
    fp32 oracle's; unused gradient elements exactly 0; everything finite.
    Prints each quantity's max error over its bound and returns them."""
    ref = b["ref64"]
    for k in ("loss", "X", "Y", "Z", "grad"):
        if k in got:
            assert np.all(np.isfinite(got[k])), f"{what}: {k} is not finite"
    e = errors(got, ref, b["tensors"])
    print(f"{what}: error / bound: " + ", ".join(
        f"{k} {v:.3g}" if not isinstance(v, str) else f"({v})" for k, v in e.items()))
    np.testing.assert_array_equal(got["X"], b["ref32"]["X"])
    if "grad" in got:
        assert np.all(got["grad"][~ref["used"]] == 0), f"{what}: unused gradient elements are not 0"
    for k in ("loss", "Y", "Z", "grad", "tensor"):
        if k in e:
            assert e[k] <= 1.0, f"{what}: {k} is {e[k]:.3g} of its bound" + (f" ({e['tensor_name']})" if k == "tensor" else "")
    return e
