"""FP32 flavour of the active-scalar kernels (libx3d2_hip_sp.so), in a process of its own like tests/particles_sp_worker.py (the
real kind is chosen when x3d2_amd is imported): test 1 of tests/test_hip_scalars.py on its three meshes with the bound
2^-23 |want| plus the FP64 bound, the plane sums, and test 4's stretched case at the FP32 step tolerance (fields
2e-5 max(|ref|, 1)).  The restatement stays in double; the checks assert in here."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_hip_scalars as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
res = {"dtype": str(np.dtype(_lib.NP_REAL))}
for name in ("box", "channel", "tail"):
    res["couple_" + name] = t.check_couple(name)
res["sums"] = t.check_profile_sums("tail", 3, 2)
for fused in (True, False):
    res["steps_fused" if fused else "steps_op"] = t.check_steps("top-bottom", "RK3", fused)
print("SCALARSRESULT " + json.dumps(res))
