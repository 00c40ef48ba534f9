#!/bin/bash
# Round evidence on the GPU box: full -m gpu suite, the default bench line (the
# driver's command), and the same bench under rocprofv3 --kernel-trace --stats
# (kernel averages per bench leg, from the qg_trace_marker markers, that the
# bench's HIP-event figures must agree with), plus the per-kernel PMC HBM table
# of the bench's probe.  Usage: round_end.sh <tag> [skip-tests]
set -o pipefail
export TMPDIR=/tmp
tag=${1:-r04}
out=${OUT:-bench_out}  # where the logs and reports go
mkdir -p "$out"
if [ "$2" != "skip-tests" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread \
    > $out/${tag}_gpu_tests.log 2>&1 || exit 1
fi
timeout -k 10 900 python -u bench.py --full --steps 20 --warmup 5 --detail-out $out/${tag}_detail.json \
  > $out/${tag}_bench.json 2> $out/${tag}_bench.err || exit 1
python3 profiles/pmc_table.py $out/${tag}_detail.json > $out/${tag}_pmc_hbm_table.txt
python3 profiles/pmc_table.py $out/${tag}_detail.json --shapes >> $out/${tag}_pmc_hbm_table.txt
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d $out/prof_${tag} -o run -- \
  python3 -u bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-traffic \
  --detail-out $out/${tag}_detail_rocprof.json > $out/${tag}_bench_under_rocprof.json \
  2> $out/${tag}_bench_under_rocprof.err || exit 1
python3 profiles/kstats.py $out/prof_${tag} --legs > $out/${tag}_kernel_stats_legs.txt
