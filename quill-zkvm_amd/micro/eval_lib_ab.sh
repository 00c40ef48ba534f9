#!/bin/bash
# Evaluation-region timings of library variants (micro/ab_<name>/libquill_gpu.so,
# "." = in-tree, named "result"; "parent", the parent commit's build, is the
# yardstick), one process per variant and round, alternating, then the summary:
# eval_lib_ab.sh <rounds> <out.json> lib...   (the processes' own files go to
# the directory <out>.d)
set -o pipefail
rounds=$1; out=$2; shift 2
dir=${out%.json}.d
mkdir -p "$dir"
py=quill-zkvm_amd/micro/eval_unify_cost.py
for i in $(seq "$rounds"); do
  for v in "$@"; do
    lib=quill-zkvm_amd/libquill_gpu.so; name=result
    [ "$v" = "." ] || { lib=quill-zkvm_amd/micro/ab_$v/libquill_gpu.so; name=$v; }
    QG_LIB=$lib timeout -k 10 200 python3 $py --out $dir/${name}_$i.json || exit 1
  done
done
python3 $py --summarize $dir --out "$out"
