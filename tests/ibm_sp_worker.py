"""FP32 flavour of the immersed-boundary kernels (libx3d2_hip_sp.so), in a process of its own like tests/sp_worker.py (the
real kind is chosen when x3d2_amd is imported): the body kernel of tests/test_hip_ibm.py at 65 x 12 x 6 for every mask, and
one AB3 step of the cylinder case at 33 x 16 x 8 whose fields go to the .npz named on the command line for the parent to
compare with its FP64 run."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_hip_ibm as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
body = {kind: t.body_case((65, 12, 6), t.DIR, kind) for kind in t.MASKS}
case, _, _ = t.cylinder_pair("AB3", False, with_ref=False)
case.step(1)
u, v, w = t.fields_of(case)
np.savez(sys.argv[1], u=u, v=v, w=w)
print("IBMRESULT " + json.dumps({"dtype": str(np.dtype(_lib.NP_REAL)), "body": body}))
