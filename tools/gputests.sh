#!/bin/bash
# GPU box: the whole -m gpu suite + smoke + the default bench line (what the driver runs at round end)
export TMPDIR=/tmp
mkdir -p gpurun_out
timeout 1500 python -m pytest tests -q -m gpu -x 2>&1 | tail -15
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
BENCH_LINE=$(timeout 600 python bench.py --full 2>/dev/null | tail -1) python - <<'PY'
import json, os
j = json.loads(os.environ["BENCH_LINE"])
print({k: j[k] for k in ("metric", "value", "ms_per_step")}, j["roofline"], j.get("cpu_baseline"))
PY
