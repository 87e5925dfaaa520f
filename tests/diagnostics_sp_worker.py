"""FP32 flavour of the diagnostics reduction (libx3d2_hip_sp.so), in a process of its own like tests/sp_worker.py (the
real kind is chosen when x3d2_amd is imported): the synthetic case of tests/test_hip_diagnostics.py at (64, 9, 8) and
(17, 33, 10); prints the rows (slot, error, bound) for the parent to assert on."""
import json
import os
import sys
import tempfile

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_hip_diagnostics as t  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
rows = []
with tempfile.TemporaryDirectory() as tmp:
    for dims in ((64, 9, 8), (17, 33, 10)):
        rows += [(name, float(err), float(bound)) for name, err, bound in t.synthetic_rows(dims, os.path.join(tmp, "d"))]
    b = t.make_backend((64, 9, 8))
    dg = t.diagnostics_of(t.Fields(b), os.path.join(tmp, "e"), divergence=False)
    blocks = t.poisoned_blocks(b, t.random_arrays((64, 9, 8), 1))
    row_dtype = str(dg.reduce(blocks[0], blocks[1], blocks[2], blocks[3:]).cpu().numpy().dtype)
print("DIAGRESULT " + json.dumps({"eps": t.eps_real(), "rows": rows, "dtype": str(np.dtype(_lib.NP_REAL)),
                                  "row_dtype": row_dtype}))
