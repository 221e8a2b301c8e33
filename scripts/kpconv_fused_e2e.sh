#!/bin/bash
# End-to-end effect of the fused KPConv forward: scripts/predator_stacked_rate.py (8 pairs stacked per forward, and the
# one-pair loop) with APR_KPCONV_FUSED=0 and 2, alternated twice.  Every GPU step under its own time limit, chained: a step
# that fails or hangs ends the script.
set -o pipefail
cd "$(dirname "$0")/.."
step() { echo "APR_KPCONV_FUSED=$1"; APR_KPCONV_FUSED=$1 timeout -k 10 "${STEP_LIMIT:-240}" python scripts/predator_stacked_rate.py; }
step 0 && step 2 && step 0 && step 2
