"""FP32 flavour of the spectra (libx3d2_hip_sp.so), in a process of its own like tests/stats_sp_worker.py (the real kind is
chosen when x3d2_amd is imported): the shell cases and the two plane cases of tests/test_hip_spectra.py; prints the rows
(name, error, bound) for the parent to assert on."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_hip_spectra as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
shell = []
for dims, L, dk in t.SHELL_CASES:
    rows, _ = t.shell_rows(dims, L, dk)
    shell += rows
plane, _ = t.plane_rows(t.channel_fields((32, 17, 16)), (32, 17, 16))
more, _ = t.plane_rows(t.periodic_fields((40, 24, 12), t.BOX, poisson=False), (40, 24, 12))
print("SPECTRARESULT " + json.dumps({"eps": t.eps_real(), "shell": shell, "plane": plane + more,
                                     "dtype": str(np.dtype(_lib.NP_REAL))}))
