#!/bin/bash
# full GPU suite + default bench line (arg: tag)
set -o pipefail
export TMPDIR=/tmp
tag=$1
out=${OUT:-bench_out}  # where the logs and reports go
mkdir -p "$out"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread \
  > $out/${tag}_gpu_tests.log 2>&1 || exit 1
timeout -k 10 900 python -u bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err || exit 1
