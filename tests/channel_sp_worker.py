"""FP32 flavour of the library on the channel case (make_channel: the 010 Poisson solve, stretched wall-normal pencils, wall
stamping, the bulk-velocity integral, the device noise generator), in a process of its own (tests/test_hip_single_prec.py):

  small <stretching> <beta> <fused 0|1>   tests/test_hip_poisson_010.py::_channel_steps' recipe at 24 x 33 x 16, two steps,
                                          against the oracle: the figures the parent asserts on
  bench                                   one fused step at 1024 x 257 x 16 against the oracle's signatures
                                          (channel1024x257x16.*, of the oracle's step here), with the FP64 test's
                                          evidence of the kernels taken
  noise <out.npz>                         one fused step with wall noise on (seeded): fields and wall planes saved, the parent
                                          compares with the FP64 library's from the same seed

Prints one line "SPRESULT <json>"."""
import json
import os
import sys

import numpy as np

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from fp32_ref import noise_step  # noqa: E402
from util import assert_signature, signature_of  # noqa: E402
from x3d2_amd import _lib, make_channel  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")


def perturbation(m):
    """_channel_steps' smooth perturbation: all three components active, no Nyquist mode"""
    X = 2 * np.pi * m.vert_coords[0][None, None, :] / m.L[0]
    Y = np.pi * m.vert_coords[1][None, :, None] / m.L[1]
    Z = 2 * np.pi * m.vert_coords[2][:, None, None] / m.L[2]
    return (0.05 * np.sin(X) * np.sin(Y) ** 2 * np.cos(Z), 0.04 * np.cos(X) * np.sin(Y) ** 2 * np.sin(Z),
            0.03 * np.sin(2 * X) * np.sin(Y) ** 2 * np.cos(Z))


def min_spacing(m):
    return float(min(np.min(np.diff(np.asarray(m.vert_coords[d], dtype=np.float64))) for d in range(3)))


if __name__ == "__main__":
    what = sys.argv[1]
    out = {}
    if what == "small":
        from test_hip_poisson_010 import oracle_solver
        stretching, beta, fused = sys.argv[2], float(sys.argv[3]), sys.argv[4] == "1"
        dims, nsteps = (24, 33, 16), 2
        case = make_channel(dims, stretching=stretching, beta=beta, fused=fused, rotation=True, omega_rot=0.12, n_rotate=2)
        o = oracle_solver(dims, stretching, beta)
        o.init_channel(rotation=True, omega_rot=0.12, n_rotate=2)
        s = case.solver
        for (fo, fp), d in zip(((o.u, s.u), (o.v, s.v), (o.w, s.w)), perturbation(o.mesh)):
            a = o.backend.get_field_data(fo) + d
            o.backend.set_field_data(fo, a)
            s.backend.set_field_data(fp, a)
        for it in range(1, nsteps + 1):
            o.step_channel(it)
            case.step(it)
        err, vmax, got32 = {}, 0.0, []
        for fo, fp, nm in ((o.u, s.u, "u"), (o.v, s.v, "v"), (o.w, s.w, "w")):
            ref, got = o.backend.get_field_data(fo), s.backend.get_field_data(fp)
            assert got.dtype == np.float32
            err[nm] = float(np.max(np.abs(got.astype(np.float64) - ref)) / max(np.max(np.abs(ref)), 1.0))
            vmax = max(vmax, float(np.max(np.abs(ref))))
            got32.append(got.astype(np.float64))
        _, ens, dmax, _ = case.postprocess(nsteps, 0.01)
        eo = o.monitor()
        # where an enstrophy difference comes from: the oracle's FP64 curl and sum on the FP32 library's fields
        for fo, a in zip((o.u, o.v, o.w), got32):
            o.backend.set_field_data(fo, a)
        e32 = o.monitor()[0]
        out = {"err": err, "enstrophy_rel": float(abs(ens - eo[0]) / abs(eo[0])), "div_max": float(dmax),
               "enstrophy_rel_of_the_fields": float(abs(e32 - eo[0]) / abs(eo[0])),
               "enstrophy_rel_of_the_evaluation": float(abs(ens - e32) / abs(eo[0])), "enstrophy": float(eo[0]),
               "div_max_oracle": float(eo[1]), "min_spacing": min_spacing(o.mesh), "vmax": vmax}
    elif what == "bench":
        dims, key = (1024, 257, 16), "channel1024x257x16"
        # no signatures of this shape are stored: the oracle's step here, as the FP64 twin pays it, signed the same way
        from test_hip_poisson_010 import oracle_solver
        from util import field_signature
        o = oracle_solver(dims, "top-bottom", 0.259065151)
        o.init_channel(rotation=True, omega_rot=0.12, n_rotate=2)
        for fo, d in zip((o.u, o.v, o.w), perturbation(o.mesh)):
            o.backend.set_field_data(fo, o.backend.get_field_data(fo) + d)
        o.step_channel(1)
        fix = {key + ".enstrophy": o.monitor()[0]}
        for fo, nm in ((o.u, "u"), (o.v, "v"), (o.w, "w")):
            for k, v in field_signature(o.backend.get_field_data(fo)).items():
                fix["%s.%s.%s" % (key, nm, k)] = v
        del o
        case = make_channel(dims, stretching="top-bottom", beta=0.259065151, fused=True, rotation=True, omega_rot=0.12, n_rotate=2)
        s = case.solver
        for fp, d in zip((s.u, s.v, s.w), perturbation(s.mesh)):
            s.backend.set_field_data(fp, s.backend.get_field_data(fp).astype(np.float64) + d)
        case.step(1)
        _, ens, dmax, _ = case.postprocess(1, 0.01)
        lib = _lib.load()
        out = {"enstrophy_rel": float(abs(ens - float(fix[key + ".enstrophy"])) / abs(float(fix[key + ".enstrophy"]))),
               "div_max": float(dmax), "min_spacing": min_spacing(s.mesh), "three_in_one": int(lib.x3d_backend_counter(s.backend.h, 0)),
               "n_rot_fused": int(s.n_rot_fused), "n_interleaved": int(s.n_interleaved), "sample_err": {}}
        fields = {nm: s.backend.get_field_data(fp) for fp, nm in ((s.u, "u"), (s.v, "v"), (s.w, "w"))}
        for nm, a in fields.items():
            sg = signature_of(fix, key + "." + nm)
            iz, iy, ix = [np.unique(np.linspace(0, n - 1, min(n, 24)).astype(np.int64)) for n in a.shape]
            out["sample_err"][nm] = float(np.max(np.abs(a[np.ix_(iz, iy, ix)] - sg["sample"])) / max(float(sg["absmax"]), 1.0))
        print("SPFIGURES " + json.dumps(out), flush=True)
        for nm, a in fields.items():
            sg = signature_of(fix, key + "." + nm)
            assert a.dtype == np.float32
            assert_signature(a, sg, 2e-5, nm, scale=max(float(sg["absmax"]), 1.0))
    elif what == "noise":
        case, fields, walls = noise_step()
        assert all(a.dtype == np.float32 for a in fields + walls)
        np.savez(sys.argv[2], u=fields[0], v=fields[1], w=fields[2], wall0=walls[0], wall1=walls[1], wall2=walls[2])
        _, ens, dmax, _ = case.postprocess(1, 0.005)
        out = {"enstrophy": float(ens), "div_max": float(dmax), "min_spacing": min_spacing(case.solver.mesh)}
    print("SPRESULT " + json.dumps(out))
