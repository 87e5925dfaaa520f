#!/bin/bash
# usage (GPU box): tools/ab_bench.sh <tag> [ENV=1 ...] -- <bench.py args>   one bench line under the given switches
tag=$1; shift
envs=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do envs+=("$1"); shift; done
shift
cd "$(dirname "$0")/.."
out=${OUT:-out}; mkdir -p $out  # (where the lines go: $OUT, default out/ in the repository)
env "${envs[@]}" python bench.py --full --no-cpu-baseline --no-other-configs --no-live-traffic "$@" > $out/ab_$tag.json 2> $out/ab_$tag.err
python - $out/ab_$tag.json $tag <<'PY'
import json, sys
try:
    d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
    r = d.get("roofline", {})
    print("%-28s ms_per_step %.3f  frac %.3f" % (sys.argv[2], d["ms_per_step"], r.get("frac", 0.0)))
except Exception as e:
    print(sys.argv[2], "FAILED", e)
PY
