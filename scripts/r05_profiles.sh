#!/bin/bash
# round 5: the four rocprofv3 passes of the bench command for C3 and C2 (scripts/gpu_profile.sh), then the default bench line
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
out=${1:?usage: r05_profiles.sh <output directory>}; mkdir -p "$out"
bash scripts/gpu_profile.sh r05_c3 c3 || exit 1
bash scripts/gpu_profile.sh r05_c2 c2 || exit 1
timeout -k 10 600 python bench.py --full --no-build > "$out"/r05_bench_default_line.json 2> "$out"/r05_bench_default.err || exit 1
cut -c1-300 "$out"/r05_bench_default_line.json
