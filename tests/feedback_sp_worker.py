"""FP32 flavour of the two-way coupling (libx3d2_hip_sp.so), in a process of its own like tests/forcing_sp_worker.py (the real
kind is chosen when x3d2_amd is imported): the kernel cases of tests/test_hip_feedback.py against the restatement -- the records
are FP64 in both flavours, f and the blocks are held to 8 * 2^-24 max(|before| + sum |contributions|), a vertex taking at most
eight rounded adds -- and the coupled steps at the FP32 step tolerance 2e-5.  The checks assert in here."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_hip_feedback as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
res = {"dtype": str(np.dtype(_lib.NP_REAL))}
for name in ("box", "channel"):
    res["field_" + name] = t.check_field(name)
    res["add_" + name] = t.check_add(name)
t.test_bit_identity_of_builds_and_slot_orders()
for fused in (True, False):
    res["steps_fused" if fused else "steps_op"] = t.check_steps("RK3", fused)
print("FEEDBACKRESULT " + json.dumps(res))
