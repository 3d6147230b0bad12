#!/bin/bash
# A/B of environment-selected variants on the PnP bench step: bash tools/ab_pnp_split.sh <tag> NAME=ENV[,ENV...] ...
tag=$1; shift
out=bench_out/$tag
mkdir -p $out
for spec in "$@"; do
  name=${spec%%=*}; envs=${spec#*=}
  env $(echo "$envs" | tr ',' ' ') timeout -k 10 120 python bench.py --estimator pnp --steps 100 --warmup 10 --no-extras --no-cpu-baseline --full > $out/$name.log 2> $out/$name.err
  python - "$out/$name.log" "$name" <<'PY'
import json,sys
log,name=sys.argv[1:3]
for line in open(log):
    if line.startswith('{'):
        j=json.loads(line); k=j['kernel_ms_per_step']
        print("%-14s value %.2f M  ms/step %.4f  chain %.4f  match %.4f  ok %s" % (name, j['value']/1e6, j['ms_per_step'], k.get('k_verify_fused',0), k.get('k_match_global',0), j['check']['decisions_matching_ground_truth']))
PY
done
