"""FP32 flavour of the band forcing (libx3d2_hip_sp.so), in a process of its own like tests/scalars_sp_worker.py (the real kind
is chosen when x3d2_amd is imported): the kernel cases of tests/test_hip_forcing.py on its four shapes against the restatement
run in FP64 on the same float32 inputs -- the coefficients and the row at 1e-12 (the accumulators are double: only the inputs are
rounded), the derivative blocks within 2 * 2^-24 max|d_after| (one rounding at the store) -- and the two forced steps at the
FP32 step tolerance 2e-5.  The checks assert in here."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_hip_forcing as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
res = {"dtype": str(np.dtype(_lib.NP_REAL))}
for name in ("20x12x18", "33x10x9", "64x16x16", "16x96x90"):
    res["kernels_" + name] = t.check_kernels(name)["blocks"]
res["kernels_M4"] = t.check_kernels("20x20x20", k_hi=4.5, solenoidal=False)["blocks"]
for fused in (True, False):
    res["steps_fused" if fused else "steps_op"] = t.check_steps("RK3", fused)
print("FORCINGRESULT " + json.dumps(res))
