"""The workgroup-split planner of the decoder launches (csrc/nsk_split.h) without a GPU: host/test/split_test.cpp, built by a plain host compiler
under AddressSanitizer + UBSan, checks the worked examples of the planner's comments and recomputes every row of tests/golden/wg_splits.txt,
the splits recorded from the functions as they stood inside nsk.hip; then it sweeps plan_fwd / plan_bwd at the extremes of the tuning keys (costs 1 and
100 000, frozen_mid_pct 10 and 1000, dead_tile_pct 0 and 100; 1 .. 3000 tiles, both wave counts) and asserts properties: every role in [1, cap],
the role ranges strictly increasing, the trainable role within its num_cu - (n - 1) gradient slabs."""
import re
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
TABLE = os.path.join(ROOT, "tests", "golden", "wg_splits.txt")


def test_the_split_planner_reproduces_its_recorded_table():
    subprocess.check_call(["make", "-s", "-C", HOST, "split_test"])
    r = subprocess.run([os.path.join(HOST, "split_test"), TABLE], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1"))
    with open(TABLE) as f:
        rows = sum(1 for line in f if line.strip() and not line.startswith("#"))
    assert rows > 5000                # (the sweep in the table's header)
    assert r.returncode == 0 and "split_test: %d rows, 0 failures" % rows in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    m = re.search(r"split_test: knob sweep (\d+) plans, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 100000, r.stdout[-1500:] + r.stderr[-3000:]
    # which backward launch goes out and which median form runs in front of it (bwd_form, bwd_deal_role, bwd_grid, median_form): every combination of
    # the boolean inputs, the four stages' role sets x trainable subsets, N in {1, 200, 1024, 1025}, num_cu in {50, 256}, against the properties
    # the launch code states (exactly one kernel; what the Tracker's launch, the frozen kernel, the dead-tile skip, dealing and the scan rider need)
    m = re.search(r"split_test: form sweep (\d+) forms, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 50000, r.stdout[-1500:] + r.stderr[-3000:]
