"""FP32 flavour of the library, every Poisson path on a broadband right-hand side (tests/test_hip_single_prec.py), in a
process of its own per environment (the switches are read once per process):

  paths <environment> <out.npz>   every case of the environment (ENVIRONMENTS below): hip_poisson_solve's recipe
                                  (solve_poisson on a DIR_C / CELL block) on fp32_ref.rhs_of(case) -- float32,
                                  default_rng, zero mean -- against the oracle's FP64 solve of the same values; the
                                  yardstick of the case (fp32_ref.yardstick) computed next to it; the evidence that the
                                  intended path ran; the solutions of the cases in KEEP saved for the comparisons in bits
  full512 <out.npy ...>           512^3: solve_zfirst and the x-first poisson_000 (k_r2c512), or -- with
                                  X3D_FORCE_PENCIL_FFT=yslab -- the y-slab solver's poisson_000; solutions saved
  chan010 <out.npy> <out.npy>     1024 x 257 x 512 top-bottom: solve_interleaved and solve_interleaved_zfirst
                                  (the FP64 reference of the two full-size cases is the FP64 library's, in the parent)

Prints one line "SPRESULT <json>"; every case's measured error, yardstick and ratio are in it."""
import json
import os
import sys

import numpy as np

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import fp32_ref  # noqa: E402
from fp32_ref import hip_poisson_solve, product_solver  # noqa: E402
from x3d2_amd import _lib  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")

_Y256 = ["010.32x257x16." + s for s in ("top-bottom", "centred", "bottom")]
_SLAB = ["000.24x512x40", "000.512x512x8", "000.24x512x512"]
# environment -> (the variables the parent sets, the cases)
ENVIRONMENTS = {
    "default": ({}, [t for t in fp32_ref.CASES if t not in _SLAB]),
    "split": ({"X3D_Y010_FORM": "split"}, [_Y256[0], _Y256[2]]),
    "staged": ({"X3D_Y010_FORM": "staged"}, [_Y256[0], _Y256[2]]),
    # (all three stretchings: every y-last case above has its 3-D-transform form to differ from in bits)
    "no_y010": ({"X3D_NO_Y010": "1"}, _Y256),
    "no_fft512": ({"X3D_NO_FFT512": "1"}, ["000.20x512x512"]),
    "no_rwt": ({"X3D_NO_RWT": "1"}, ["000.20x512x512"]),
    "slab": ({"X3D_FORCE_PENCIL_FFT": "slab"}, _SLAB),
    "pencil3": ({"X3D_FORCE_PENCIL_FFT": "1", "X3D_PENCIL_PARTS": "3"}, ["000.34x40x24"]),
}
KEEP = set(_Y256) | {"000.20x512x512"}


def evidence(pf):
    return {"type": type(pf).__name__, "case": pf.case, "zfirst_ok": bool(pf.zfirst_ok()),
            "stretched_y": bool(pf.stretched_y), "stretched_y_sym": bool(getattr(pf, "stretched_y_sym", False)),
            "parts": int(getattr(pf, "parts", 0))}


what = sys.argv[1]
out = {}
if what == "paths":
    name, path = sys.argv[2], sys.argv[3]
    envs, tags = ENVIRONMENTS[name]
    for k in ("X3D_Y010_FORM", "X3D_NO_Y010", "X3D_NO_FFT512", "X3D_NO_RWT", "X3D_FORCE_PENCIL_FFT", "X3D_PENCIL_PARTS"):
        assert os.environ.get(k) == envs.get(k), (k, os.environ.get(k), envs.get(k))
    keep = {}
    for tag in tags:
        f = fp32_ref.rhs_of(tag)
        s = product_solver(tag)
        got = hip_poisson_solve(s, f)
        opf = fp32_ref.oracle_poisson(tag)
        yard, ref = fp32_ref.yardstick(opf, f)
        err = fp32_ref.errors(got, ref)
        out[tag] = {"l2": err[0], "max": err[1], "yard_l2": yard[0], "yard_max": yard[1], "ratio_l2": err[0] / yard[0],
                    "ratio_max": err[1] / yard[1], "finite": bool(np.all(np.isfinite(got))), **evidence(s.backend.poisson_fft)}
        print("%-10s %-30s l2 %.3e / %.3e = %5.2f   max %.3e / %.3e = %5.2f   %s" % (
            name, tag, err[0], yard[0], err[0] / yard[0], err[1], yard[1], err[1] / yard[1], type(s.backend.poisson_fft).__name__),
            flush=True)
        if tag in KEEP:
            keep[tag] = got
        del s, opf
    np.savez(path, **keep)
elif what == "full512":
    tag = "000.512x512x512"
    f = fp32_ref.rhs_of(tag)
    s = product_solver(tag)
    pf = s.backend.poisson_fft
    out = evidence(pf)
    if os.environ.get("X3D_FORCE_PENCIL_FFT") == "yslab":
        np.save(sys.argv[2], hip_poisson_solve(s, f))
    else:
        np.save(sys.argv[2], hip_poisson_solve(s, f, "solve_zfirst"))
        np.save(sys.argv[3], hip_poisson_solve(s, f))  # poisson_000, x first: k_r2c512, own y pass, fused z pass
elif what == "chan010":
    tag = "010.1024x257x512.top-bottom"
    f = fp32_ref.rhs_of(tag)
    s = product_solver(tag)
    out = evidence(s.backend.poisson_fft)
    np.save(sys.argv[2], hip_poisson_solve(s, f, "solve_interleaved"))
    np.save(sys.argv[3], hip_poisson_solve(s, f, "solve_interleaved_zfirst"))
print("SPRESULT " + json.dumps(out))
