"""FP32 flavour of the library (libx3d2_hip_sp.so = every source compiled with -DX3D_SINGLE_PREC, the reference's
-DSINGLE_PREC of src/common.f90:6-12), run in a process of its own (X3D_SINGLE_PREC is read when x3d2_amd is imported):
  (1) every operator of the reference's periodic fixture (ref_p000_rk3.npz: der1st / der2nd / interpolations / staggered
      derivatives in x, y, z, transeq) against the reference's FP64 vectors, tolerance 1e-5 relative (max norm);
  (2) the Dirichlet + stretched fixture (ref_c010_rk3.npz) likewise (general kernels, stretching tables);
  (3) TGV 64^3, RK3, FFT Poisson, 20 steps, fused driver and the deferred layer: enstrophy against the FP64 trace fixture
      (1e-5 relative), max |div u| at FP32 round-off;
  (4) a 512^3 fused step (the bench's kernels: tile kernels, z-first Poisson solve) against the same step at 1e-4 of the
      field maximum after ONE step from the analytic initial field (FP64 result computed by the FP64 library in the parent)."""
import json
import os
import sys

import numpy as np

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import util  # noqa: E402
from x3d2_amd import _lib, make_tgv  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
out = {}
what = sys.argv[1]
if what == "operators":
    from test_hip_parity import make_solver, set_inputs
    from util import OPNAMES, load_golden, relerr
    from x3d2_amd.common import DIR_X, DIR_Z, VERT, move_data_loc
    for fx in sys.argv[2].split(","):
        g = load_golden(fx)
        s = make_solver(g)
        set_inputs(s, g)
        b, al = s.backend, s.backend.allocator
        worst = {}
        for d, (dn, dp) in enumerate(zip("xyz", (s.xdirps, s.ydirps, s.zdirps)), 1):
            for op in OPNAMES:
                src = al.get_block(DIR_X, VERT)
                b.veccopy(src, s.u)
                if op.endswith("p2v"):
                    src.set_data_loc(move_data_loc(VERT, d, 1))
                a, o = al.get_block(d), al.get_block(d)
                if d == 1:
                    b.veccopy(a, src)
                    a.set_data_loc(src.data_loc)
                else:
                    b.reorder(a, src, 10 + d)
                b.tds_solve(o, a, getattr(dp, op))
                worst["tds.%s.%s" % (dn, op)] = float(relerr(b.get_field_data(o), g["tds.%s.%s" % (dn, op)]))
                for f in (src, a, o):
                    al.release_block(f)
        rhs = [al.get_block(DIR_X) for _ in range(3)]
        s.transeq(rhs, [s.u, s.v, s.w])
        for f, k in zip(rhs, ("du", "dv", "dw")):
            worst["transeq." + k] = float(relerr(b.get_field_data(f), g["transeq." + k]))
        div_u = al.get_block(DIR_Z)
        s.divergence_v2p(div_u, s.u, s.v, s.w)
        worst["div"] = float(relerr(b.get_field_data(div_u), g["div.div_u"]))
        s.gradient_p2v(*rhs, div_u)
        for f, k in zip(rhs, ("dpdx", "dpdy", "dpdz")):
            worst["grad." + k] = float(relerr(b.get_field_data(f), g["grad." + k]))
        for f in rhs:
            f.set_data_loc(VERT)
        s.curl(*rhs, s.u, s.v, s.w)
        for f, k in zip(rhs, "ijk"):
            worst["curl." + k] = float(relerr(b.get_field_data(f), g["curl." + k]))
        ens = 0.5 * sum(b.scalar_product(f, f) for f in rhs) / s.ngrid
        worst["enstrophy"] = float(abs(ens - g["curl.enstrophy"][0]) / abs(g["curl.enstrophy"][0]))
        out[fx] = {"max": max(worst.values()), "argmax": max(worst, key=worst.get), "all": worst}
elif what == "trace":
    fx = util.read_trace_fixture()
    for driver in ("fused", "lazy"):
        case = make_tgv(64, fused=(driver == "fused"), lazy=(driver == "lazy"))
        case.solver.n_output = 10
        rows = case.run(n_iters=20)
        out[driver] = {"enstrophy_rel": [abs(r[1] - f[1]) / f[1] for r, f in zip(rows, fx)],
                       "div_max": [float(r[2]) for r in rows]}
elif what == "step512":
    case = make_tgv(512, fused=True)
    case.step(1)
    s = case.solver
    fields = [s.backend.get_field_data(f) for f in (s.u, s.v, s.w)]
    np.savez(sys.argv[2], u=fields[0], v=fields[1], w=fields[2])
    row = case.postprocess(1, 1e-3)
    out = {"enstrophy": float(row[1]), "div_max": float(row[2]), "dtype": str(fields[0].dtype), "n_zfirst": int(s.n_zfirst)}
elif what == "wide":
    # the wide-stencil kernels (tests/test_hip_wide_stencils.py) on 4-byte reals: every operator and the direction's
    # transeq against the FP64 dense solve; 'optimised' interpolation, then hyperviscous der2nd
    from test_hip_wide_stencils import _dense
    from util import OPNAMES, dense_apply, dense_transeq, hyperviscous_der2nd, relerr
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.common import DIR_X, VERT, move_data_loc
    from x3d2_amd.solver import Solver, SolverConfig
    per, wall = ("periodic",) * 2, ("dirichlet",) * 2
    for tag, dims, d, bcs in (("x512", (512, 12, 10), 1, [per] * 3), ("x1024", (1024, 12, 10), 1, [per] * 3),
                              ("y512", (32, 512, 8), 2, [per] * 3), ("z257", (64, 8, 257), 3, [per, per, wall])):
        for interpl, hyper in (("optimised", False), ("classic", True)):
            mesh = Mesh(dims, (1, 1, 1), (2.0, 3.0, 2.5), *bcs)
            s = Solver(HipBackend(mesh), mesh, SolverConfig(poisson_solver_type="CG", fused=True, interpl_scheme=interpl))
            b, al = s.backend, s.backend.allocator
            dp = (s.xdirps, s.ydirps, s.zdirps)[d - 1]
            if hyper:
                hyperviscous_der2nd(dp, mesh, b.alloc_tdsops)
            dense = _dense(mesh, d, interpl, hyper)
            rng = np.random.default_rng(d)
            arrays = [rng.standard_normal((dims[2], dims[1], dims[0])) for _ in range(3)]
            for f, a in zip((s.u, s.v, s.w), arrays):
                f.set_data_loc(VERT)
                b.set_field_data(f, a)
            worst = {}
            for op in OPNAMES:
                t = getattr(dp, op)
                loc = move_data_loc(VERT, d, 1) if op.endswith("p2v") else VERT
                src, o = al.get_block(DIR_X, VERT), al.get_block(DIR_X)
                b.veccopy(src, s.u)
                src.set_data_loc(loc)
                b.tds_apply(o, src, t, d)
                o.set_data_loc(move_data_loc(loc, d, t.move))
                worst[op] = float(relerr(b.get_field_data(o).astype(np.float64), dense_apply(dense[op], arrays[0], 3 - d)))
                for f in (src, o):
                    al.release_block(f)
            rhs = [al.get_block(DIR_X) for _ in range(3)]
            b.transeq_dir(d, *rhs, s.u, s.v, s.w, s.nu, dp, accumulate=False)
            for k, (f, want) in enumerate(zip(rhs, dense_transeq(dense, *arrays, s.nu, 3 - d))):
                worst["transeq." + "uvw"[k]] = float(relerr(b.get_field_data(f, VERT).astype(np.float64), want))
            out["%s.%s" % (tag, "hyperviscous" if hyper else interpl)] = worst
print("SPRESULT " + json.dumps(out))
