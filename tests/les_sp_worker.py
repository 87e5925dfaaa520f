"""FP32 flavour of the explicit LES (libx3d2_hip_sp.so), in a process of its own like tests/sp_worker.py (the real kind is
chosen when x3d2_amd is imported):

  kernel        the synthetic cases of tests/test_hip_les.py with 2^-24 |ref| (one rounding of a double result) on top of
                the double bound, their scalars, and the whole term against the dense restatement
  step <out>    one fused channel step with WALE attached; the fields go to <out> for the parent to compare with the FP64
                library's

Prints one line "LESRESULT <json>"."""
import json
import os
import sys

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import les_ref  # noqa: E402
import test_hip_les as t  # noqa: E402
import util  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")


def term_errors():
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.les import Les, LesConfig
    out = {}
    for kind in ("box", "wall"):
        for model, c2 in t.MODELS:
            case, dims = t.small_case(kind, dims=(40, 40, 40))
            s = case.solver
            b, m = s.backend, s.mesh
            u, v, w = (a.astype(np.float32).astype(np.float64) for a in t.set_noisy(case, dims))
            les = Les(s, LesConfig(model=model))
            d = [b.allocator.get_block(DIR_X, VERT) for _ in range(3)]
            for f in d:
                f.fill(0.0)
            les.add(*d)
            got = [b.get_field_data(f).astype(np.float64) for f in d]
            deltas = [float(x) for x in m.d]
            ops = les_ref.dense_der1st(dims, deltas, [tuple(m.BCs_global[k]) for k in range(3)])
            tables = [np.full(n, h ** (2.0 / 3.0)) for n, h in zip(dims, deltas)]
            sgs, _, _ = les_ref.dense_term(u, v, w, ops, tables, model, c2)
            out["%s-%s" % (kind, model)] = max(util.relerr(g, r) for g, r in zip(got, sgs))
    return out


if __name__ == "__main__":
    what = sys.argv[1]
    res = {"dtype": str(np.dtype(_lib.NP_REAL))}
    if what == "kernel":
        rows = []
        for idx in range(len(t.SHAPES)):
            for model, c2 in t.MODELS:
                r = t.kernel_case(idx, model)
                tag = "%s %s " % (t.IDS[idx], model)
                one_rounding = lambda ref: np.asarray(np.abs(ref), dtype=np.float64) * 2.0 ** -24
                rows += [(tag + n, float(e), float(bd)) for n, e, bd in t.pointwise_rows(r, model, c2, extra=one_rounding)]
                rows += [(tag + n, float(e), float(bd)) for n, e, bd in t.scalar_rows(r, model, c2)]
                res["row_dtype"] = str(r["row"].dtype)
        res["rows"], res["term"] = rows, term_errors()
    elif what == "step":
        from x3d2_amd.les import LesConfig
        fields, _, _, case = t.stepped("channel", "RK3", True, LesConfig(model="wale"), nsteps=1)
        got = [case.solver.backend.get_field_data(f) for f in (case.solver.u, case.solver.v, case.solver.w)]
        assert all(a.dtype == np.float32 for a in got)
        np.savez(sys.argv[2], u=got[0], v=got[1], w=got[2])
    print("LESRESULT " + json.dumps(res))
