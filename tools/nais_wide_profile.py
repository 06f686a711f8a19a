"""Step timings of NAIS-Net at hidden widths up to 1024 (the wide projection
kernels of csrc/projw.hip), with the Resnet step at the same shape as the
yardstick: the same per-layer chain without projection or V layers.  Needs a
GPU.

  * workload: BSB, depth 4, Sine, M = 1024, N = 50, Adam, device mode, at
    (D, L) in {(100, 128), (256, 272), (512, 528), (1022, 1024)} -- the
    reference sizes its networks as D + 10 or so; L = 128 is the last width of
    the narrow projection kernels;
  * medians of event-timed steps after warm-up, then the per-kernel table of a
    profiled pass (dbsde_profile_*);
  * for rtr(_wide) and proj_backward(_wide): the achieved algorithmic TFLOP/s
    (2 L^3 per block and product) against the fp32 matrix peak, their share of
    the step's kernel time, and the share by FLOP count, about 3 L / (14 R).
    python tools/nais_wide_profile.py [out.json] [commit]   (default profiles/nais_wide_times.json)"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nais_wide_times.json")
COMMIT = (sys.argv[2] if len(sys.argv) > 2 else None) or None
pkg = importlib.import_module("deep-neural-network-solutions-for-partial-differential-equations_amd")
dev = torch.device("cuda:0")
M, N, WARM, STEPS, PROF = 1024, 50, 5, 20, 5
MFMA_F32 = 157.3e12
SHAPES = ((100, 128), (256, 272), (512, 528), (1022, 1024))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def step_case(mode, D, L):
    torch.manual_seed(0)
    m = pkg.BlackScholesBarenblatt(np.ones((1, D)), 1.0, M, N, D, [D + 1] + 4 * [L] + [1], mode, "Sine", device=dev)
    opt = m.new_optimizer_state("Adam", 1e-3)
    it = [0]

    def step():
        m.device_step(opt, seed=it[0], next_seed=it[0] + 1)
        it[0] += 1

    for _ in range(WARM):
        step()
    torch.cuda.synchronize()
    ms = [timed(step) for _ in range(STEPS)]
    m.solver.prefetch_drop()
    m.solver.profile(True)
    m.solver.profile_reset()
    for _ in range(PROF):
        m.device_step(opt, seed=it[0])
        it[0] += 1
    torch.cuda.synchronize()
    prof = m.solver.profile_read()
    m.solver.profile(False)
    kern = {k: dict(us=1e3 * v["ms"] / v["launches"], gflop=v["flops"] / v["launches"] / 1e9)
            for k, v in prof.items() if v["launches"]}
    # per step: a kernel launched several times a step counts every launch
    per_step = {k: 1e3 * v["ms"] / PROF for k, v in prof.items() if v["launches"]}
    loss = float(m._gradbuf[-1])
    return dict(mode=mode, D=D, L=L, matrix_form=m.solver.matrix_form, ms_median=float(np.median(ms)),
                ms_min=float(np.min(ms)), ms_max=float(np.max(ms)), path_steps_per_s=M * N / (np.median(ms) * 1e-3),
                last_loss=loss, finite=bool(np.isfinite(loss)), kernels_us_per_step=per_step,
                kernel_sum_us=float(sum(per_step.values()))), kern


def projection(case, kern):
    """The two projection launches of a NAIS row."""
    R = M * (N + 1)
    out = {}
    total = case["kernel_sum_us"]
    for base in ("rtr", "proj_backward"):
        name = base + "_wide" if base + "_wide" in kern else base
        row = kern[name]
        fl = row["gflop"] * 1e9 / (row["us"] * 1e-6)
        out[name] = dict(us=row["us"], tflop_per_s=fl / 1e12, mfma_f32_fraction=fl / MFMA_F32,
                         share_of_step_kernel_time=row["us"] / total)
    out["share_of_step_kernel_time"] = sum(v["us"] for v in out.values()) / total
    out["share_by_flop_count"] = 3.0 * case["L"] / (14.0 * R)
    return out


res = {"commit": COMMIT,
       "shape": dict(M=M, N=N, layers="[D+1, L, L, L, L, 1]", activation="Sine", problem="bsb", optimizer="Adam",
                     warmups=WARM, steps=STEPS, profiled_steps=PROF),
       "peaks": dict(mfma_f32_flop_per_s=MFMA_F32), "rows": []}
for D, L in SHAPES:
    nais, kern = step_case("NAIS-Net", D, L)
    nais["projection"] = projection(nais, kern)
    resnet, _ = step_case("Resnet", D, L)
    res["rows"].append(dict(D=D, L=L, nais=nais, resnet=resnet, nais_over_resnet=nais["ms_median"] / resnet["ms_median"]))
    print(f"D={D} L={L}: NAIS-Net {nais['ms_median']:.3f} ms, Resnet {resnet['ms_median']:.3f} ms, projection "
          f"{nais['projection']}", file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)       # after every row: a partial table survives a time limit
print(json.dumps(res, indent=1))
