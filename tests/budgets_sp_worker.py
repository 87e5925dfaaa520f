"""FP32 flavour of the budget kernels (libx3d2_hip_sp.so), in a process of its own like tests/stats_sp_worker.py (the real
kind is chosen when x3d2_amd is imported): parity, determinism and p = NULL of tests/test_hip_budgets.py on every shape of
that file, plus 1030 x 3 x 2 -- a 16-byte load holds four 4-byte points, so the lane loop's second trip starts at 1024.
Prints the rows (error, bound) for the parent to assert on; the bound is the FP64 one."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_hip_budgets as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
cases = []
for dims, ybc, dir_keep in t.SHAPES + [((1030, 3, 2), t.PER, 2)]:
    rows, _, _ = t.parity_case(dims, ybc, dir_keep)  # (asserts that the sums formed twice agree bit for bit)
    zero, same = t.no_pressure_case(dims, ybc, dir_keep)
    cases.append({"id": "%dx%dx%d-keep%d" % (tuple(dims) + (dir_keep,)), "rows": rows, "zero": zero, "same": same})
print("BUDGETSRESULT " + json.dumps({"dtype": str(np.dtype(_lib.NP_REAL)), "cases": cases}))
