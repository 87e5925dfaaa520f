"""The compact operators of the FP32 library (libx3d2_hip_sp.so), kernel family by kernel family, in a process of its own with
exactly the switches the caller set: ops_sp_worker.py <environment name> <tag,tag,...> (tags of fp32_ops_ref.CASES).
Per case, on the case's float32 inputs: the eight operators through tds_apply, plain and accumulating; transeq_dir plain and
accumulating; Solver.transeq; tds_pair in both modes for both pairs; on x also tds_lincomb against lincomb + tds_apply (bits)
and the three-in-one counter across transeq_x.  Every result's error against the oracle in FP64 on the same inputs, the
yardstick of the same check (tests/fp32_ops_ref.py) and their ratios, L2 and max norm, are printed as one FP32OP line each --
before anything is asserted on them; the worst result of the case in either norm is appended, as one line, to the file named
by X3D_FP32_OPS_PROFILE when it is set."""
import hashlib
import json
import os
import sys

import numpy as np

os.environ["X3D_SINGLE_PREC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import fp32_ops_ref as ops_ref  # noqa: E402
from util import OPNAMES  # noqa: E402
from x3d2_amd import _lib  # noqa: E402
from x3d2_amd.common import DIR_X, VERT, move_data_loc  # noqa: E402

assert _lib.SINGLE and _lib.LIB_PATH.endswith("_sp.so")
environment, tags = sys.argv[1], sys.argv[2].split(",")
profile = os.environ.get("X3D_FP32_OPS_PROFILE")


def run_case(tag):
    p = ops_ref.Pipeline(tag)
    yard = p.yardsticks()
    ref = ops_ref.oracle_results(p)
    s = ops_ref.product_solver(tag)
    b, al, d = s.backend, s.backend.allocator, p.d
    dp = (s.xdirps, s.ydirps, s.zdirps)[d - 1]
    for f, a in zip((s.u, s.v, s.w), (p.u, p.v, p.w)):
        f.set_data_loc(VERT)
        b.set_field_data(f, a)
    got, extra = {}, {}
    src, src2, o1, o2 = (al.get_block(DIR_X, VERT) for _ in range(4))
    sc = ops_ref.ACC_SCALE[d]
    for op in OPNAMES:
        t = getattr(dp, op)
        loc = move_data_loc(VERT, d, 1) if op.endswith("p2v") else VERT
        out_loc = move_data_loc(loc, d, t.move)
        b.veccopy(src, s.u)
        src.set_data_loc(loc)
        b.tds_apply(o1, src, t, d)
        o1.set_data_loc(out_loc)
        got["tds." + op] = b.get_field_data(o1)
        b.veccopy(o2, s.v)  # the accumulating form adds to another field
        b.tds_apply(o2, src, t, d, accumulate=True, scale=sc)
        o2.set_data_loc(out_loc)
        got["acc." + op] = b.get_field_data(o2)
    for opa, opb in ops_ref.PAIRS:
        ta, tb = getattr(dp, opa), getattr(dp, opb)
        loc = VERT if opa.endswith("v2p") else move_data_loc(VERT, d, 1)
        for f, g in ((src, s.u), (src2, s.v)):
            b.veccopy(f, g)
            f.set_data_loc(loc)
        b.tds_pair(0, o1, None, src, src2, ta, tb, d)
        o1.set_data_loc(move_data_loc(loc, d, ta.move))
        got["pair0.%s+%s" % (opa, opb)] = b.get_field_data(o1)
        b.tds_pair(1, o1, o2, src, None, ta, tb, d)
        o1.set_data_loc(move_data_loc(loc, d, ta.move))
        o2.set_data_loc(move_data_loc(loc, d, tb.move))
        got["pair1.%s.A" % opa] = b.get_field_data(o1)
        got["pair1.%s.B" % opb] = b.get_field_data(o2)
    rhs = [al.get_block(DIR_X) for _ in range(3)]
    b.transeq_dir(d, *rhs, s.u, s.v, s.w, s.nu, dp, accumulate=False)
    for k, f in enumerate(rhs):
        got["transeq_dir." + "uvw"[k]] = b.get_field_data(f, VERT)
    for f, prev in zip(rhs, (s.w, s.u, s.v)):
        b.veccopy(f, prev)
    b.transeq_dir(d, *rhs, s.u, s.v, s.w, s.nu, dp, accumulate=True)
    for k, f in enumerate(rhs):
        got["transeq_dir_acc." + "uvw"[k]] = b.get_field_data(f, VERT)
    s.transeq(rhs, [s.u, s.v, s.w])
    for k, f in enumerate(rhs):
        got["transeq." + "uvw"[k]] = b.get_field_data(f, VERT)
    if d == 1:
        # the RK stage's linear combination as the prologue of an x operator: the bits of lincomb followed by tds_apply
        coefs = [0.3, -1.7, 0.01]
        for f in (src, src2, o1, o2):
            f.set_data_loc(VERT)
        b.lincomb(src, s.u, coefs, [s.v, s.w, s.u])
        b.tds_apply(o1, src, dp.stagder_v2p, DIR_X)
        b.tds_lincomb(o2, dp.stagder_v2p, DIR_X, src2, s.u, coefs, [s.v, s.w, s.u])
        for f in (o1, o2):  # (the rows the operator writes: one fewer than vertices on a walled pencil)
            f.set_data_loc(move_data_loc(VERT, 1, 1))
        extra["lincomb_bits_equal"] = bool(np.array_equal(b.get_field_data(src), b.get_field_data(src2))
                                           and np.array_equal(b.get_field_data(o1), b.get_field_data(o2)))
        n3 = int(b.lib.x3d_backend_counter(b.h, 0))
        b.transeq_x(*rhs, s.u, s.v, s.w, s.nu, dp)
        extra["three_in_one"] = int(b.lib.x3d_backend_counter(b.h, 0)) - n3
    res = {}
    for name, g in got.items():
        finite = bool(g.dtype == np.float32 and g.shape == ref[name].shape and np.all(np.isfinite(g)))
        e = ops_ref.errors(g, ref[name]) if g.shape == ref[name].shape else (float("inf"),) * 2
        y = yard[name]
        res[name] = {"l2": e[0], "yard_l2": y[0], "ratio_l2": e[0] / y[0], "max": e[1], "yard_max": y[1],
                     "ratio_max": e[1] / y[1], "finite": finite, "bits": hashlib.sha1(g.tobytes()).hexdigest()[:16]}
        print("FP32OP " + json.dumps(dict({"environment": environment, "case": tag, "op": name},
                                          **{k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in res[name].items()})))
    # the profile keeps one line per environment and case: the worst result in either norm (every result is printed above)
    w2, wm = max(res, key=lambda k: res[k]["ratio_l2"]), max(res, key=lambda k: res[k]["ratio_max"])
    line = {"environment": environment, "case": tag, "results": len(res), "finite": all(e["finite"] for e in res.values()),
            "worst_l2": dict(op=w2, **{k: float("%.4g" % res[w2][k]) for k in ("l2", "yard_l2", "ratio_l2")}),
            "worst_max": dict(op=wm, **{k: float("%.4g" % res[wm][k]) for k in ("max", "yard_max", "ratio_max")}),
            "largest_yard_max": float("%.4g" % max(e["yard_max"] for e in res.values()))}
    if profile:
        with open(profile, "a") as fh:
            fh.write(json.dumps(line) + "\n")
    print("FP32OPX " + json.dumps(dict({"environment": environment, "case": tag}, **extra)))
    return {"ops": res, "extra": extra}


out = {tag: run_case(tag) for tag in tags}
print("SPRESULT " + json.dumps(out))
