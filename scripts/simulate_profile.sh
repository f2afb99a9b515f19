#!/bin/bash
# The simulator's performance record: call times, a kernel trace (device time per call against the byte and instruction
# models) and two counter passes of their own over the first case's subtree walk.  Usage: scripts/simulate_profile.sh OUT_DIR
set -o pipefail
OUT=${1:?output directory}
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$OUT"
S="python3 $R/scripts/simulate_scale.py"
one="--cases balanced20_f81_k64 --iters 1"
timeout -k 10 600 $S --iters 20 > "$OUT/calls.txt" &&
timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d "$OUT/trace" -o run -- $S --iters 3 > /dev/null 2> "$OUT/trace.err" &&
timeout -k 10 600 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR GRBM_GUI_ACTIVE \
    --output-format csv -d "$OUT/pmc_a" -o run -- $S $one > /dev/null 2> "$OUT/pmc_a.err" &&
timeout -k 10 600 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE \
    --output-format csv -d "$OUT/pmc_b" -o run -- $S $one > /dev/null 2> "$OUT/pmc_b.err" &&
{
    echo "== calls (HIP events around Engine.simulate_states, median of 20; includes the copy of the states to the host)"
    cat "$OUT/calls.txt"
    echo "== device time per call (rocprofv3 --kernel-trace, median of 3 calls after 2 warm-up calls)"
    $S --iters 3 --trace "$(find "$OUT/trace" -name '*kernel_trace.csv' | head -1)"
    echo "== SQ counters of the subtree walk of balanced20_f81_k64 (two --pmc passes of their own)"
    $S --pmc "$(find "$OUT/pmc_a" -name '*counter_collection.csv' | head -1)" "$(find "$OUT/pmc_b" -name '*counter_collection.csv' | head -1)"
} > "$OUT/record.txt"
