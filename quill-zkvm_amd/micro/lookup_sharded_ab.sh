#!/bin/bash
# The lookup measurements of profiles/lookup_sharded.json in one visit:
#   lookup_sharded_ab.sh <parent libquill_gpu.so> [rounds] [output directory]
# 1. micro/lookup_mult_cost.py's measurement on the parent's build and on the
#    in-tree build, alternating, <rounds> times each (single_<lib>_<i>.json);
# 2. the materialiser cost and the sharded per-rank split on the in-tree build;
# 3. everything merged into <output directory>/lookup_sharded.json
#    (default bench_out, which git ignores).
set -o pipefail
parent=$1; rounds=${2:-2}; top=${3:-bench_out}
out=$top/lookup_sharded; mkdir -p $out
py=quill-zkvm_amd/micro/lookup_sharded_cost.py
files=()
for i in $(seq "$rounds"); do
  for v in parent branch; do
    lib=quill-zkvm_amd/libquill_gpu.so; [ "$v" = branch ] || lib=$parent
    QG_LIB=$lib timeout -k 10 240 python3 $py --part single --out $out/single_${v}_$i.json \
      > $out/single_${v}_$i.log 2>&1 || exit 1
    files+=($out/single_${v}_$i.json)
  done
done
timeout -k 10 240 python3 $py --part materialiser --out $out/materialiser.json > $out/materialiser.log 2>&1 || exit 1
timeout -k 10 300 python3 $py --part sharded --out $out/sharded.json > $out/sharded.log 2>&1 || exit 1
python3 $py --merge "${files[@]}" $out/materialiser.json $out/sharded.json --out $top/lookup_sharded.json > /dev/null
