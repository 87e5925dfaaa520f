"""FP32 flavour of the snapshot pack kernel (libx3d2_hip_sp.so), in a process of its own like tests/stats_sp_worker.py
(the real kind is chosen when x3d2_amd is imported): the COPY and the VORT / QCRIT checks of tests/test_hip_snapshot.py
on 17 x 6 x 5; prints the results for the parent to assert on."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import test_hip_snapshot as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
dims = (17, 6, 5)
checks, rows = 0, []
for stride in ((1, 1, 1), (2, 3, 2)):
    for first in t.FIRSTS:
        checks += t.copy_case(dims, t.PER, stride, first)
    for first in t.FIRSTS[:2]:
        rows += t.derived_case(dims, t.PER, stride, first, against_existing=(stride == (1, 1, 1) and first == (0, 0, 0)))
print("SNAPRESULT " + json.dumps({"eps": t.eps_real(), "copy_checks": checks, "derived": rows}))
