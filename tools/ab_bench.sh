#!/bin/bash
# usage (on the GPU box): tools/ab_bench.sh <tag>=<lib.so> [<tag>=<lib.so> ...] [-- extra bench args]
# Runs the default bench (config 2, --full for the kernel-event roofline, no secondary / CPU legs) once per library on the SAME
# box and prints one line each; the JSON lines and stderr go to $AB_OUT (default: $TMPDIR/ab_bench).
O=${AB_OUT:-${TMPDIR:-/tmp}/ab_bench}; mkdir -p "$O"
libs=(); extra=()
while [ $# -gt 0 ]; do
  if [ "$1" == "--" ]; then shift; extra=("$@"); break; fi
  libs+=("$1"); shift
done
for spec in "${libs[@]}"; do
  tag=${spec%%=*}; lib=${spec#*=}
  ENSLAM_LIB=$lib ENSLAM_LIB_ALLOW_MISSING=1 python bench.py --steps 300 --warmup 30 --full --no-cpu-baseline --no-secondary "${extra[@]}" > "$O/ab_$tag.json" 2> "$O/ab_$tag.err" || { echo "$tag FAILED"; tail -3 "$O/ab_$tag.err"; continue; }
  python - "$tag" "$O/ab_$tag.json" <<'PY'
import json, sys
tag = sys.argv[1]
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
r = d.get("roofline", {})
print(f"{tag:14s} {d['ms_per_step']*1e3:8.1f} us/step  {d['value']/1e6:6.3f} Mrays/s  bwd {r.get('avg_launch_us', 0):7.1f} us (dense {r.get('avg_launch_us_dense', 0):7.1f})  frac {r.get('frac', 0):.3f} dense {r.get('frac_dense', 0):.3f} step_frac {r.get('step_frac', 0):.3f} loss {d['loss']:.6f}")
PY
done
