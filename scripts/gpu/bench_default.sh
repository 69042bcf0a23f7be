#!/bin/bash
# The multi-GPU bench tests (shared-device gloo rehearsals, strong legs) and the default
# bench line (N = 1, every leg).
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
mkdir -p gpurun_out
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests/test_gpu_multigpu.py -m gpu -x -v --timeout 600 --timeout-method thread \
  -p no:cacheprovider -k "bench" > gpurun_out/t_bench.log 2>&1 || { tail -40 gpurun_out/t_bench.log; exit 1; }
tail -3 gpurun_out/t_bench.log
OUT=${BENCH_OUT:-bench_out}  # the line and its stderr land here
mkdir -p "$OUT"
timeout -k 10 900 python3 bench.py --full > "$OUT/default_bench.json" 2> "$OUT/default_bench.err" \
  || { tail -30 "$OUT/default_bench.err"; exit 1; }
python3 -c "import json,sys;d=json.load(open(sys.argv[1]));print(d['value'],d['ms_per_step']);print(json.dumps(d['strong_scaling'],indent=1))" "$OUT/default_bench.json"
