#!/bin/bash
# final check of the in-tree library: GPU suite, smoke, the full bench line (traffic from
# the committed PMC record of this build); logs go to $O (default build/check)
set -o pipefail
cd "$(dirname "$0")/.."; O=${O:-build/check}; mkdir -p "$O"
timeout -k 10 900 python -u -m pytest -q --timeout 300 --timeout-method thread tests -m gpu > "$O/final_t.log" 2>&1 || { tail -5 "$O/final_t.log"; exit 1; }
tail -1 "$O/final_t.log"
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$O/final_smoke.log" 2>&1 || { tail -5 "$O/final_smoke.log"; exit 1; }
tail -1 "$O/final_smoke.log"
timeout -k 10 300 python -u bench.py --full > "$O/final_bench.log" 2>&1 || { tail -5 "$O/final_bench.log"; exit 1; }
tail -1 "$O/final_bench.log" | cut -c1-400; grep -o '"roofline": {[^}]*}' "$O/final_bench.log" | cut -c1-200
