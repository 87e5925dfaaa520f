"""FP32 flavour of the loads and probes kernels (libx3d2_hip_sp.so), in a process of its own like tests/ibm_sp_worker.py (the
real kind is chosen when x3d2_amd is imported): the cases of tests/test_hip_loads.py at 65 x 12 x 6 for every mask (field
bits against x3d_ibm_body, rows against numpy on the float32 values), the uniform flow, and the probes at 33 x 16 x 8 (files
under the prefix named on the command line).  The parent applies the same checks and bounds as in FP64."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_hip_loads as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
body = {kind: t.body_loads_case((65, 12, 6), t.tib.DIR, kind) for kind in t.tib.MASKS}
res = {"dtype": str(np.dtype(_lib.NP_REAL)), "body": body, "uniform": t.uniform_flow_case(),
       "probes": t.probes_case((33, 16, 8), sys.argv[1])}
print("LOADSRESULT " + json.dumps(res))
