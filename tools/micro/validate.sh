#!/bin/bash
# The round-end check in one go: the whole -m gpu suite, smoke(), the full bench line (--full: every leg).
# usage: tools/micro/validate.sh OUTDIR      (run from the repository root; logs and the bench line land in OUTDIR)
set -o pipefail
OUT=${1:?usage: tools/micro/validate.sh OUTDIR}
mkdir -p "$OUT"
timeout -k 10 1000 python -m pytest tests -m gpu -x -q > "$OUT/validate_tests.log" 2>&1; echo "pytest rc=$?" | tee -a "$OUT/validate_tests.log"
tail -3 "$OUT/validate_tests.log"
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
timeout -k 10 600 python bench.py --gpus 1 --steps 20 --warmup 5 --full > "$OUT/validate_bench.json" 2> "$OUT/validate_bench.err"; echo "bench rc=$?"
python3 - "$OUT/validate_bench.json" <<'EOF'
import json, sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1])
r = d['roofline']
print('value', d['value'], 'ms/step', d['ms_per_step'], 'sustained', d['sustained']['value'], 'serial', d['pipeline']['serial']['value'], 'check', d['pipeline']['check'])
print('roofline', r['kernel'], r['achieved'], r['frac'], 'alone', r['kernel_alone']['frac'], 'chip', r['chip_level']['frac'], 'traffic', r['traffic'], 'busy', r['mfma_busy'])
print('cpu', d['cpu_baseline']['value'], d['cpu_baseline']['variants'])
EOF
