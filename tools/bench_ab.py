"""No-regression A/B of bench.py between the parent commit's library and this
tree's, in one session on one GPU (profiles/heston2_bench_ab.json,
profiles/heston_corr_bench_ab.json have this format).  Needs a GPU.

    python tools/bench_ab.py PARENT_LIB OUT.json [PARENT_COMMIT] [REPEATS] [WORKLOADS]

PARENT_LIB is a libdbsde.so built from the parent commit; each run selects its
library through DBSDE_LIB (the in-tree one when unset).  When a change alters a
struct of the C ABI (dbsde_problem gained a member), this tree's binding cannot
drive the parent's library: PARENT_LIB is then a directory, a built checkout of
the parent commit, and the parent arm runs that checkout's own bench.py.  Per workload (WORKLOADS,
comma-separated names of bench.py's --workload; default bsb,heston): `python
bench.py --gpus 1 --steps 50 --warmup 10`, parent and this change alternating
REPEATS (5) times, the order inside each pair alternating too; then
--dump-outputs of both, compared bitwise.  Recorded: every ms/step, the medians, the parent's own spread
(max - min) and whether the medians differ by less than it."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_LIB, OUT = os.path.abspath(sys.argv[1]), sys.argv[2]
PARENT_COMMIT = sys.argv[3] if len(sys.argv) > 3 else None
REPEATS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
WORKLOADS = tuple(sys.argv[5].split(",")) if len(sys.argv) > 5 else ("bsb", "heston")
DUMPS = os.path.join(ROOT, "bench_out", "bench_ab")


def bench(arm, workload, dump=None):
    env = dict(os.environ)
    env.pop("DBSDE_LIB", None)
    root = ROOT
    if arm == "parent" and os.path.isdir(PARENT_LIB):
        root = PARENT_LIB
    elif arm == "parent":
        env["DBSDE_LIB"] = PARENT_LIB
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "10"]
    if workload != "bsb":
        cmd += ["--workload", workload]
    if dump:
        cmd += ["--dump-outputs", dump]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=root)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(f"bench.py failed on the {arm} library (exit {r.returncode}); nothing further is started")
    return json.loads(r.stdout.strip().split("\n")[-1])


res = {"what": f"python bench.py --gpus 1 --steps 50 --warmup 10 (--workload {', '.join(WORKLOADS)}) on the parent "
               f"commit's library and on this change's, alternating {REPEATS} times each in one session on one MI355X "
               "(the order inside each pair alternates too); then --dump-outputs of both",
       "parent_commit": PARENT_COMMIT, "workloads": {}}
for workload in WORKLOADS:
    runs = {"parent": [], "this": []}
    for i in range(REPEATS):
        for arm in (("parent", "this") if i % 2 == 0 else ("this", "parent")):
            runs[arm].append(bench(arm, workload))
            print(f"{workload} {arm} {i}: {runs[arm][-1]['ms_per_step']:.4f} ms/step", file=sys.stderr, flush=True)
    ms = {a: [r["ms_per_step"] for r in runs[a]] for a in runs}
    med = {a: float(np.median(ms[a])) for a in ms}
    spread = float(max(ms["parent"]) - min(ms["parent"]))
    same = {}
    for arm in ("parent", "this"):
        bench(arm, workload, dump=os.path.join(DUMPS, workload, arm))
    for name in sorted(os.listdir(os.path.join(DUMPS, workload, "parent"))):
        if name.endswith(".npy"):
            a = np.load(os.path.join(DUMPS, workload, "parent", name))
            b = np.load(os.path.join(DUMPS, workload, "this", name))
            same[name] = bool(a.shape == b.shape and a.tobytes() == b.tobytes())
    res["workloads"][workload] = {
        "ms_per_step": ms, "median_ms": med, "parent_spread_ms": spread,
        "median_difference_ms": med["this"] - med["parent"],
        "within_parent_spread": bool(abs(med["this"] - med["parent"]) <= spread),
        "final_loss": {a: [r.get("final_loss") for r in runs[a]] for a in runs},
        "dump_outputs_bitwise_equal": same}
    print(f"{workload}: median parent {med['parent']:.4f} this {med['this']:.4f} ms/step, parent spread {spread:.4f}, "
          f"bitwise {same}", file=sys.stderr, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(res, open(OUT, "w"), indent=1)
print(json.dumps(res, indent=1))
