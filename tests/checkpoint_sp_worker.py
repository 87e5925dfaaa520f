"""FP32 flavour of the checkpoint kernels (libx3d2_hip_sp.so), in a process of its own like tests/snapshot_sp_worker.py
(the real kind is chosen when x3d2_amd is imported): the kernel checks of tests/test_hip_checkpoint.py at (17, 6, 5) and
(64, 5, 3) and one AB3 resume; prints the results for the parent to assert on."""
import json
import os
import pathlib
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import test_hip_checkpoint as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
checks = 0
for dims in ((17, 6, 5), (64, 5, 3)):
    for nblock in t.NBLOCKS:
        checks += t.kernel_case(dims, t.PER, nblock)
a, c = t.run_pair("tgv", pathlib.Path(sys.argv[1]), time_intg="AB3", fused=True)
t.assert_same_run(a, c)
print("CKPTRESULT " + json.dumps({"real_bytes": t.real_dtype().itemsize, "kernel_checks": checks, "resume": True}))
