#!/bin/bash
# Negative control of tests/test_gpu_dirty_memory.py::test_result_slices_on_poisoned_memory: the same test against a build
# that skips the clear of the results outside a komb_truss_run_slice rank's slice (-DKOMB_TEST_SKIP_SLICE_ZERO, ktruss.hip)
# must FAIL.  That clear only feeds values (the trussness / support words copied out), never an index, address or loop bound.
# Run on the GPU box; prints "negative control ok" only when the poisoned slice test ends with failed assertions (pytest exit
# status 1).  Any other status of either GPU step -- a crash, an abort, a fault, a time-limit kill, a collection or usage
# error -- ends the script at once with a nonzero status, and nothing more is started on the GPU.
#
# The existing tests/test_gpu_parity.py::test_result_slices runs against the same build first, for the record: it starts
# from whatever the context's pool holds, so whether it notices depends on the call history.  On an MI355X it FAILS too
# (its earlier whole-graph run leaves nonzero trussness in the block the slice run gets back), but only by luck of that
# history; the poisoned test fails on the first rank of its first graph.
cd "$(dirname "$0")/../.."
LOG="${TMPDIR:-/tmp}/slice_zero_negative_control.$$"
make -s -j8 -C komb_amd/csrc OUT=../libv/slicezero EXTRA=-DKOMB_TEST_SKIP_SLICE_ZERO ../libv/slicezero/libkomb_accel.so || exit 2
LIB=komb_amd/libv/slicezero/libkomb_accel.so

# run_step <log> <pytest args...>: sets STATUS to pytest's exit status; 0 (passed) and 1 (a failed assertion) are the only outcomes
# after which the script goes on
run_step() {
    local log=$1; shift
    KOMB_ACCEL_LIB=$LIB timeout -k 10 900 python -m pytest "$@" > "$log" 2>&1
    STATUS=$?
    if [ "$STATUS" -ne 0 ] && [ "$STATUS" -ne 1 ]; then
        echo "negative control ABORTED: pytest $* ended with status $STATUS (not a test failure)"; tail -15 "$log"; exit 3
    fi
    if [ "$STATUS" -eq 1 ] && ! grep -q "AssertionError" "$log"; then      # (a library error raised in a test is no result)
        echo "negative control ABORTED: pytest $* failed without a failed assertion"; tail -15 "$log"; exit 3
    fi
}

run_step "$LOG.old" tests/test_gpu_parity.py -q -m gpu -k test_result_slices
if [ "$STATUS" -eq 0 ]; then echo "existing test_result_slices: passes on the build without the clear"
else echo "existing test_result_slices: fails on the build without the clear"; fi

run_step "$LOG" tests/test_gpu_dirty_memory.py -x -q -m gpu -k slice
if [ "$STATUS" -eq 0 ]; then
    echo "negative control FAILED: the poisoned slice test passed without the clear"; tail -5 "$LOG"; exit 1
fi
if ! grep -q "outside the slice" "$LOG"; then
    echo "negative control FAILED: the poisoned slice test failed, but not on the zeros outside the slice"; tail -15 "$LOG"; exit 1
fi
grep -E "outside the slice" "$LOG" | head -3
echo "negative control ok: the skipped clear is caught"
