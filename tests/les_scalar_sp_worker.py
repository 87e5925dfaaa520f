"""FP32 flavour of the LES eddy diffusivity (libx3d2_hip_sp.so), in a process of its own like tests/les_sp_worker.py (the real
kind is chosen when x3d2_amd is imported):

  kernel        the synthetic cases of tests/test_hip_les_scalar.py with 2^-24 |ref| (one rounding of a double result) on top
                of the double bound, their rows, and the species' term against the dense restatement
  step <out>    one fused channel step with WALE and one species; the fields go to <out> for the parent to compare with the
                FP64 library's

Prints one line "LESRESULT <json>"."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import test_hip_les_scalar as ts  # noqa: E402
import util  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")


if __name__ == "__main__":
    what = sys.argv[1]
    res = {"dtype": str(np.dtype(_lib.NP_REAL))}
    if what == "kernel":
        rows = []
        one_rounding = lambda ref: np.asarray(np.abs(ref), dtype=np.float64) * 2.0 ** -24
        for idx in range(len(ts.SHAPES)):
            for ns in (1, 2):
                r = ts.kernel_case(idx, ns)
                tag = "%s ns=%d " % (ts.IDS[idx], ns)
                rows += [(tag + n, float(e), float(bd)) for n, e, bd in ts.pointwise_rows(r, extra=one_rounding)]
                rows += [(tag + n, float(e), float(bd)) for n, e, bd in ts.row_rows(r)]
                res["row_dtype"] = str(r["row"].dtype)
        term = {}
        for kind in ("box", "wall"):
            got, _, (sgs, _, _), _ = ts.device_term(kind, "smagorinsky")
            term[kind] = util.relerr(got, sgs)
        res["rows"], res["term"] = rows, term
    elif what == "step":
        from x3d2_amd.les import LesConfig
        _, case = ts.stepped("channel", "RK3", True, LesConfig(model="wale", prt=ts.PRT[0]), nsteps=1)
        s = case.solver
        got = [s.backend.get_field_data(f) for f in (s.u, s.v, s.w, s.species[0])]
        assert all(a.dtype == np.float32 for a in got)
        np.savez(sys.argv[2], u=got[0], v=got[1], w=got[2], phi=got[3])
    print("LESRESULT " + json.dumps(res))
