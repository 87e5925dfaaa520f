"""FP32 flavour of the statistics kernels (libx3d2_hip_sp.so), in a process of its own like tests/sp_worker.py (the real
kind is chosen when x3d2_amd is imported): the 3-D update of tests/test_hip_stats.py on 64 x 33 x 48 and the profile
along y; prints the rows (error, bound) for the parent to assert on."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_hip_stats as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
dims, n = (64, 33, 48), 3
rows, _, _, _ = t.update_case(dims, t.WALL)
prof = t.profile_case(dims, t.WALL, 2, n=n)
eps = t.eps_real()
P = dims[0] * dims[2]
# (the bound without the P of the summation: err, (n + 4 + P) eps vmax -> + (n + 4) eps vmax)
prof = [(name, err, bound, bound * (n + 4) / (n + 4 + P)) for name, err, bound in prof]
print("STATSRESULT " + json.dumps({"eps": eps, "update": rows, "profile": prof, "dtype": str(np.dtype(_lib.NP_REAL))}))
