#!/bin/bash
# A/B of environment switches with extra bench arguments (one GPU box call):
#   tools/ab_args.sh "<bench args>" "ENV=1" "ENV=2" ...
# Results under $RESULTS_DIR (default bench_out).
R=${RESULTS_DIR:-bench_out}
mkdir -p $R
: > $R/ab.txt
args=$1; shift
for v in "$@"; do
  env $v timeout -k 10 240 python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline $args > $R/ab_run.log 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "$v rc=$rc" | tee -a $R/ab.txt; tail -5 $R/ab_run.log; exit $rc; fi
  python - "$v" $R/ab_run.log >> $R/ab.txt <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
print(sys.argv[1], "ms/step %.4f" % d["ms_per_step"], json.dumps(d["step_kernel_ms"]))
PY
done
cat $R/ab.txt
