#!/bin/bash
# A/B of library environment switches on the bench (one GPU box call):
#   tools/ab_env.sh "DBSDE_CHUNKS=1" "DBSDE_CHUNKS=2" ...
# Each variant runs bench.py --full --steps 30 --warmup 5 --no-cpu-baseline under
# its own time limit; one summary line per variant in $R/ab.txt (R = $RESULTS_DIR,
# default bench_out).
R=${RESULTS_DIR:-bench_out}
mkdir -p $R
: > $R/ab.txt
for v in "$@"; do
  env $v timeout -k 10 240 python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline > $R/ab_run.log 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "$v rc=$rc" | tee -a $R/ab.txt; tail -5 $R/ab_run.log; exit $rc; fi
  python - "$v" $R/ab_run.log >> $R/ab.txt <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
print(sys.argv[1], "ms/step %.4f" % d["ms_per_step"], "frac %.3f" % d["roofline"]["frac"], json.dumps(d["step_kernel_ms"]))
PY
done
cat $R/ab.txt
