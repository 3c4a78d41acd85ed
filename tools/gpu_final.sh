#!/bin/bash
# final validation on the GPU machine, two calls (each under 20 minutes): `bash tools/gpu_final.sh tests` -- smoke() and
# the full GPU suite; `bash tools/gpu_final.sh bench` -- the bench line with everything --full adds (audit, CPU
# baseline, every companion).  Logs under $OUT/final_* (default bench_out/).
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
if [ "$1" = tests ]; then
  timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke()" > "$OUT/final_smoke.log" 2>&1; s=$?
  echo "smoke=$s"; tail -2 "$OUT/final_smoke.log"; [ $s -eq 0 ] || exit $s
  timeout -k 10 1080 python3 -u -m pytest tests -m gpu -v -x -p no:cacheprovider --timeout 300 --timeout-method thread \
    > "$OUT/final_tests.log" 2>&1; s=$?
  echo "tests=$s"; grep -cE "PASSED" "$OUT/final_tests.log"; tail -3 "$OUT/final_tests.log"; exit $s
fi
if [ "$1" = bench ]; then
  timeout -k 10 900 python3 -u bench.py --full > "$OUT/final_bench.json" 2> "$OUT/final_bench.err"; s=$?
  echo "bench=$s"; tail -2 "$OUT/final_bench.err"; [ $s -eq 0 ] || exit $s
  python3 -c "import json, sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d['audit_flips'], d['spotted_digest'], d['roofline']['frac'], d['cpu_baseline'].get('value'))" "$OUT/final_bench.json"
  exit 0
fi
echo "usage: bash tools/gpu_final.sh tests|bench"; exit 2
