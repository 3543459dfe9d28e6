#!/bin/bash
# whole gpu suite (no -x), then the default bench line:  gpurun --timeout 2400 -- bash tools/gpu_suite_and_bench.sh
R=${GRAFT_REPO_ROOT:-/root/repo}
cd $R; mkdir -p gpurun_out
timeout 1800 python -m pytest tests -m gpu -q -rf --no-header -p no:cacheprovider 2>&1 | grep -v amdgpu.ids | tail -40 | tee gpurun_out/pytest_gpu.log
mkdir -p runs; timeout 900 python bench.py --full > runs/bench_default.out 2> runs/bench_default.err; echo "bench rc=$?"; tail -3 runs/bench_default.err
python - <<'PY'
import json
d=json.load(open('runs/bench_extras.json'))     # bench.py --full's whole record
print('headline', d['value'], d['ms_per_step'], d['region_ms_per_step'])
for x in d['extra_configs']:
    print(x.get('key'), x.get('value'), x.get('error'))
PY
