#!/bin/bash
# per-launch table of the decode Linears, bf16 route and fp8 route, from one rocprofv3 kernel trace of tools/bench_decode_w8.py profile (one sequence, the default)
# or batched_profile (B = 8 on the matrix-pipe chain: `batched` as the second argument)
# usage: tools/prof_decode_w8.sh <output directory> [batched]   (linears.md, stats.md and run.log are left in it)
set -eo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "${1:?usage: tools/prof_decode_w8.sh <output directory> [batched]}"
OUT=$(cd "$1" && pwd)
PRE=""
[ "${2:-}" = "batched" ] && PRE="batched_"
cd /tmp && export TMPDIR=/tmp
NEW=${NEW:-17} rocprofv3 --kernel-trace --stats -d "$OUT" -o dec -- python "$ROOT/tools/bench_decode_w8.py" ${PRE}profile > "$OUT/run.log" 2>&1
DB=$(find "$OUT" -name "*.db" | head -1)
python "$ROOT/tools/bench_decode_w8.py" ${PRE}table "$DB" "$OUT/linears.md"
python "$ROOT/tools/rocpd_stats.py" "$DB" "$OUT/stats.md" > /dev/null 2>&1
rm -f "$DB"
