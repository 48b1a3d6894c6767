#!/bin/bash
# The measurements of DESIGN section 4.7d on one MI355X: the fused evaluation rollout against the by-hand path (the gate:
# exit status of the first step), then the chunk time of the training loop with and without evaluation.
#   tools/gpu_ddpg_eval.sh [OUT_DIR]     (default profiles/ddpg_eval)
# Each GPU step runs under its own time limit; nothing runs after a step that failed.
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/ddpg_eval}
mkdir -p "$OUT"
timeout -k 10 300 python tools/exp_ddpg_eval.py percall --out "$OUT" 2>&1 | tee "$OUT/percall.log" &&
timeout -k 10 300 python tools/exp_ddpg_eval.py chunk --out "$OUT" 2>&1 | tee "$OUT/chunk.log"
