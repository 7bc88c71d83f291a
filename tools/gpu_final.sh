#!/bin/bash
# Final-tree evidence: GPU tests, smoke, the full bench line, rocprofv3 kernel trace of the
# ring points of the bench, FETCH / WRITE / SQ counter passes (ring) and FETCH / WRITE (C4 ORSet, C5).
# Results go to $OUT (default bench_out/).
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${1:-fin}
timeout -k 10 900 python -u -m pytest tests -x -q -m gpu --timeout 280 --timeout-method thread > $OUT/${TAG}_pytest.log 2>&1 || { echo "pytest failed"; tail -40 $OUT/${TAG}_pytest.log; exit 1; }
tail -1 $OUT/${TAG}_pytest.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || { echo "smoke failed"; tail -20 $OUT/${TAG}_smoke.log; exit 1; }
tail -1 $OUT/${TAG}_smoke.log
timeout -k 10 900 python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { echo "bench failed"; tail -30 $OUT/${TAG}_bench.err; exit 1; }
python3 -c "import json; d=json.loads(open('$OUT/${TAG}_bench.json').read().strip().splitlines()[-1]); print(json.dumps(d['summary'])); print(json.dumps(d['roofline']))"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o run -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-configs > $OUT/${TAG}_prof.log 2>&1 || { echo "rocprof failed"; tail -20 $OUT/${TAG}_prof.log; exit 1; }
echo "rocprof ok"
bash tools/gpu_pmc_r03.sh pmc3 || exit 1
