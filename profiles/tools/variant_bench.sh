#!/bin/bash
# runs bench.py --full --lean with every library variant under scratch/variants and prints the blend_bwd time
# (per-variant JSON under $VARIANT_OUT, default /tmp/variant_bench)
cd $GRAFT_REPO_ROOT
out=${VARIANT_OUT:-/tmp/variant_bench}
mkdir -p "$out"
for f in scratch/variants/lib_*.so; do
  n=$(basename $f .so)
  MGS_LIB_PATH=$PWD/$f python bench.py --full --lean --steps 50 --warmup 10 > $out/var_$n.json 2> $out/var_$n.err
  python - <<PY
import json
try:
    d=json.loads([l for l in open("$out/var_$n.json") if l.startswith("{")][-1])
    print("$n", "fps", d["value"], "kernels", d["kernels_us"])
except Exception as e:
    print("$n", "FAILED", e)
PY
done
