"""FP32 flavour of the running-sum RK stages (libx3d2_hip_sp.so), in a process of its own like tests/stats_sp_worker.py (the
real kind is chosen when x3d2_amd is imported): the whole-step comparison of tests/test_rk_running_sum.py, default against
X3D_NO_RK_RUNSUM=1, on both pencil lengths; prints the rows for the parent to assert on."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_rk_running_sum as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
rows = []
for dims in t.STEP_DIMS:
    for time_intg in ("RK3", "RK4"):
        new, cn = t.run_steps(dims, time_intg, 2)
        old, co = t.run_steps(dims, time_intg, 2, X3D_NO_RK_RUNSUM="1")
        rows.append({"dims": dims, "time_intg": time_intg, "dtype": str(new[0].dtype), "nstage": cn["nstage"],
                     "finite": bool(all(np.isfinite(a).all() for a in new)),
                     "in_transeq_new": cn["in_transeq"], "in_transeq_old": co["in_transeq"],
                     "equal": [bool(np.array_equal(a, b)) for a, b in zip(new, old)]})
print("RUNSUMRESULT " + json.dumps(rows))
