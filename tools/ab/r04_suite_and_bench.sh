O=${1:?usage: bash tools/ab/r04_suite_and_bench.sh OUT_DIR}; mkdir -p "$O"
timeout -k 10 600 python -m pytest tests/ -x -q -m gpu > "$O/gpu_tests_5.txt" 2>&1; rc=$?
tail -3 "$O/gpu_tests_5.txt"
[ $rc -eq 0 ] || exit 1
for i in 1 2; do timeout -k 10 200 python bench.py --full --steps 100 --warmup 10 --no-cpu-baseline --no-latency --no-compare --no-host-leg > "$O/bench_silu4_$i.json" 2>/dev/null || exit 1; done
python - <<PY
import json
for i in (1,2):
    d=json.loads(open("$O/bench_silu4_%d.json"%i).read().strip().splitlines()[-1]); print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["conv_kernels_ms_eager"], d["roofline"].get("in_kernel_clock",{}).get("ghz_mean"))
PY
