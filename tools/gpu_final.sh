#!/bin/bash
# Round-end evidence in one GPU call: C3 steady-state kernel trace + PMC
# traffic passes, the default bench line of a --full run (with the CPU
# baseline), and the C5 steady-state kernel trace.  The bench line goes to
# $KMC_OUT_DIR/<tag> (default: prof_out/<tag> in the repository).
#   tools/gpu_final.sh <tag> [pmc|sq|all]   (PMC passes of the C3 profile, default pmc)
set -euo pipefail
tag=$1
root=${GRAFT_REPO_ROOT:-$(pwd)}
out=${KMC_OUT_DIR:-$root/prof_out}/$tag
mkdir -p "$out"
cd "$root"
bash tools/gpu_steady_profile.sh "${tag}_C3" C3 "${2:-pmc}"
cd "$root"
timeout -k 10 400 python bench.py --full > "$out/bench.json" 2> "$out/bench.err"
bash tools/gpu_steady_profile.sh "${tag}_C5" C5
echo "final $tag done"
