"""FP32 flavour of the particle kernels (libx3d2_hip_sp.so), in a process of its own like tests/loads_sp_worker.py (the real kind
is chosen when x3d2_amd is imported): tests 1 and 2 of tests/test_hip_particles.py on the channel.  The restatement takes the
float32 fields widened to double; the parent applies the FP64 bounds."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_hip_particles as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
tracers, _, _ = t.update_rows("channel", fused=True)
inertial, _, _ = t.update_rows("channel", inertial=True, fused=True)
res = {"dtype": str(np.dtype(_lib.NP_REAL)), "interpolation": t.interpolation_rows("channel"), "tracers": tracers,
       "inertial": inertial}
print("PARTICLESRESULT " + json.dumps(res))
