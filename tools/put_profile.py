"""One BasketPutOption training step beside one BasketCallOption step at the
basket workload's shape of bench.py (100 assets, Naisnet-ReLU [101, 110 x 4, 1],
M = 4096, N = 50, the Q10 correlation matrix, Adam, device mode, prefetched), in
one session: medians of 20 event-timed device steps after 5 warm-ups, and the
launches of one profiled step of each -- a put step must launch exactly the
kernels of the call step.  Recorded, not gated.  Needs a GPU.

    python tools/put_profile.py OUT.json [commit]

OUT.json is created or, when it exists (tools/bench_ab.py's result), gains the
key "put_against_call"."""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1]
COMMIT = sys.argv[2] if len(sys.argv) > 2 else None
D, M, N, WARM, STEPS = 100, 4096, 50, 5, 20

pkg = importlib.import_module("deep-neural-network-solutions-for-partial-differential-equations_amd")
dev = torch.device("cuda:0")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def arm(cls):
    torch.manual_seed(0)
    np.random.seed(0)                      # the Q10 correlation matrix draw
    m = cls(np.ones((1, D)), 1.0, M, N, D, None, [D + 1] + 4 * [110] + [1], "Naisnet", "ReLU", "random_correlation",
            device=dev)
    opt = m.new_optimizer_state("Adam", 1e-3)
    it = [0]

    def step():
        m.device_step(opt, 1e-3, seed=it[0], next_seed=it[0] + 1)
        it[0] += 1

    for _ in range(WARM):
        step()
    torch.cuda.synchronize()
    ms = [timed(step) for _ in range(STEPS)]
    m.solver.profile(True)
    m.solver.profile_reset()
    step()
    torch.cuda.synchronize()
    prof = m.solver.profile_read()
    m.solver.profile(False)
    m.solver.prefetch_drop()
    loss = float(m._gradbuf[-1])
    return dict(g=m.spec.g, matrix_form=m.solver.matrix_form, ms_median=float(np.median(ms)), ms_min=float(np.min(ms)),
                ms_max=float(np.max(ms)), last_loss=loss, finite=bool(np.isfinite(loss)),
                launches={n: int(v["launches"]) for n, v in sorted(prof.items())})


res = {"what": "one device-mode training step of BasketPutOption beside BasketCallOption at bench.py's basket shape, "
               f"medians of {STEPS} event-timed steps after {WARM} warm-ups in one session, and the launches of one "
               "profiled step of each",
       "commit": COMMIT, "shape": dict(D=D, M=M, N=N, layers="[101, 110, 110, 110, 110, 1]", mode="Naisnet",
                                       activation="ReLU", correlation="random_correlation", optimizer="Adam")}
# call, put, put, call: neither arm always runs first
runs = [arm(c) for c in (pkg.BasketCallOption, pkg.BasketPutOption, pkg.BasketPutOption, pkg.BasketCallOption)]
res["call"], res["put"] = [runs[0], runs[3]], [runs[1], runs[2]]
res["same_launches"] = all(r["launches"] == runs[0]["launches"] for r in runs)
res["median_ms"] = dict(call=float(np.median([r["ms_median"] for r in res["call"]])),
                        put=float(np.median([r["ms_median"] for r in res["put"]])))
full = json.load(open(OUT)) if os.path.exists(OUT) else {}
full["put_against_call"] = res
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(full, open(OUT, "w"), indent=1)
print(json.dumps(res, indent=1))
