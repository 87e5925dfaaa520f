"""The FP32 yardstick of the compact operators: the dense operators of tests/util.py (dense_dirps: A the tridiagonal
left-hand side, B the right-hand side stencils, result = solve(A, B @ u)) run as a correctly rounded FP32 pipeline would run
them, on the host.
  * A, B and the input are rounded to float32;
  * B32 @ u32 and np.linalg.solve(A32, .) stay in float32 (LAPACK's sgesv: the dtypes are asserted);
  * on a stretched direction the result is multiplied by the operator's `stretch` table rounded to float32, which is what
    tds_solve does (oracle/x3d_oracle.c, der_univ_subs); the tables are the oracle's own operators';
  * transeq32 combines du, dud and d2u as the oracle does (der_univ_fused_subs): du s, dud s, d2u s2 + du s cor, every table
    and nu rounded to float32, every product and sum in float32;
  * accumulate: float32(prev + float32(scale) * apply32(..)); pair mode 0: apply32(A)(f) + apply32(B)(g) in float32.

The yardstick of a check = the error of this pipeline against the same dense pipeline in FP64 on the same
float32-representable inputs, as two numbers: L2-relative, and max norm relative to the reference's maximum (util.relerr).
An FP32 kernel is accepted at BOUND (fp32_ref's 8) x the yardstick of its check, L2 against L2 and max norm against max norm;
the kernel's own error is taken against the oracle in FP64 on the same inputs, which the dense FP64 pipeline equals to 1e-12
(tests/test_fp32_ops_ref_host.py).  Solver.transeq adds the three directions' pipelines in float32; its other two directions
are short periodic pencils (8 .. 16 points) where the dense solve is the exact periodic solve and the oracle the truncated
distributed one, so the dense FP64 sum is no reference of the kernel there -- the oracle is -- but the distance between the two
dense pipelines still is the FP32 rounding of that sum."""
import numpy as np

import fp32_ref
import util

BOUND = fp32_ref.BOUND  # acceptance: error <= BOUND x yardstick, per norm, per operator, per case
CAP = 4e-6              # a check whose yardstick alone exceeds this in max norm is a badly chosen input (Dirichlet der2nd: 1.4e-6)
OLD_TOL = {"tight": 2e-5, "loose": 5e-4}  # tests/sp_worker.py's tolerances; loose: der2nd*, transeq*
TWOPI = 6.283185307179586
_LX, _LYZ = (TWOPI, 2.0, 3.0), (2.0, 3.0, 2.5)  # the lengths of the FP64 twins of each case (tests/test_hip_parity.py)
PAIRS = (("interpl_v2p", "stagder_v2p"), ("interpl_p2v", "stagder_p2v"))
ACC_SCALE = {1: -0.5, 2: 0.25, 3: 0.25}  # the scale of the accumulating forms, by direction

# tag -> (dims, direction, boundary condition of that direction, its stretching, beta, L, seed)
CASES = {}


def _case(dims, d, bc="periodic", stretching="uniform", beta=1.0):
    tag = "%s.%dx%dx%d.%s.%s" % ("xyz"[d - 1], *dims, bc, stretching)
    CASES[tag] = (tuple(dims), d, bc, stretching, beta, _LX if d == 1 else _LYZ, 61 + len(CASES))
    return tag


X_PERIODIC = [_case((nx, 12, 10), 1) for nx in (128, 192, 256, 500, 512, 1024)]
X_NEUMANN = _case((512, 12, 10), 1, "neumann")
NPW2 = [_case(dims, d) for dims, d in (((32, 512, 8), 2), ((64, 8, 512), 3), ((32, 256, 8), 2), ((64, 8, 256), 3),
                                       ((128, 256, 8), 2))]
NPW1 = [_case((48, 512, 8), 2), _case((48, 8, 256), 3)]
NON_TILE = _case((40, 256, 9), 2)
WALLS = [_case((32, 257, 8), 2, "dirichlet", "top-bottom", 0.259065151), _case((48, 130, 8), 2, "neumann"),
         _case((64, 8, 257), 3, "dirichlet"), _case((32, 384, 8), 2, "dirichlet", "centred", 1.3),
         _case((16, 500, 8), 2, "dirichlet", "bottom", 1.3), _case((32, 320, 8), 2, "dirichlet", "top-bottom", 0.259065151),
         _case((16, 8, 321), 3, "neumann")]
# the groups the switched runs take
CIRC = [t for t in X_PERIODIC if t.split(".")[1].split("x")[0] in ("256", "512", "1024")] + [t for t in NPW2 + NPW1]
XCIRC = ["x.512x12x10.periodic.uniform"]
UNIFORM = ["y.32x512x8.periodic.uniform", "z.64x8x256.periodic.uniform"]
DIRECT = ["y.32x257x8.dirichlet.top-bottom", "z.64x8x257.dirichlet.uniform", "y.32x320x8.dirichlet.top-bottom"]
Q5 = ["y.32x320x8.dirichlet.top-bottom"]
assert all(t in CASES for t in CIRC + XCIRC + UNIFORM + DIRECT + Q5)
# pencil and tile counts that leave a tail: a persistent loop takes more than one trip and its last trip is short, or the
# count is odd, or the last workgroup holds a lone pencil (tests/test_hip_work_counts.py has the arithmetic of each case).
# After every other case: the seeds are 61 + the position
COUNTS_X = [_case(dims, 1) for dims in ((256, 65, 64), (512, 9, 9), (1024, 9, 9), (1024, 46, 45))]
COUNTS_TILE = [_case((128, 256, 66), 2), _case((64, 66, 512), 3), _case((48, 512, 87), 2)]
COUNTS_WALLS = [_case(dims, 2, "dirichlet", "top-bottom", 0.259065151)
                for dims in ((64, 257, 65), (32, 257, 9), (48, 257, 87), (32, 320, 9))]
COUNTS = COUNTS_X + COUNTS_TILE + COUNTS_WALLS
assert len(COUNTS) == 11 and [CASES[t][-1] for t in COUNTS] == list(range(83, 94))

errors = fp32_ref.errors


def bcs_of(tag):
    """the three pairs of boundary conditions of a case"""
    _, d, bc, *_ = CASES[tag]
    return [(bc,) * 2 if k == d - 1 else ("periodic",) * 2 for k in range(3)]


def stretching_of(tag):
    _, d, _, stretching, beta, *_ = CASES[tag]
    return (tuple(stretching if k == d - 1 else "uniform" for k in range(3)),
            tuple(beta if k == d - 1 else 1.0 for k in range(3)))


def inputs_of(tag):
    """u, v, w [nz, ny, nx]: default_rng(seed).standard_normal rounded to float32; the oracle and the library both receive
    these exact values"""
    dims, *_, seed = CASES[tag]
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(dims[::-1]).astype(np.float32) for _ in range(3)]


def oracle_solver(tag):
    from oracle import x3d_oracle as orc
    dims, _, _, _, _, L, _ = CASES[tag]
    strs, beta = stretching_of(tag)
    om = orc.Mesh(list(dims), [1, 1, 1], list(L), *[list(b) for b in bcs_of(tag)], stretching=strs, beta=beta)
    return orc.Solver(om, poisson="CG")


def product_solver(tag):
    """the library's fused solver of a case, in the flavour (FP64 / FP32) this process loaded"""
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.solver import Solver, SolverConfig
    dims, _, _, _, _, L, _ = CASES[tag]
    strs, beta = stretching_of(tag)
    mesh = Mesh(dims, (1, 1, 1), L, *bcs_of(tag), strs, beta)
    return Solver(HipBackend(mesh), mesh, SolverConfig(poisson_solver_type="CG", fused=True))


# ---------------------------------------------------------------- the pipeline, in either precision
def _apply(op, a, stretch, axis, dt):
    A, B = (np.asarray(m, dtype=dt) for m in op)
    assert a.dtype == dt, (a.dtype, dt)
    u = np.moveaxis(a, axis, -1)[..., :B.shape[1]]
    r = B @ np.ascontiguousarray(u.reshape(-1, B.shape[1]).T)
    assert r.dtype == dt, r.dtype
    x = np.linalg.solve(A, r)
    assert x.dtype == dt, x.dtype  # (float32 in: LAPACK's single-precision solve)
    x = x.T.reshape(u.shape[:-1] + (A.shape[0],))
    if stretch is not None:
        x = x * np.asarray(stretch, dtype=dt)[:A.shape[0]]
    assert x.dtype == dt, x.dtype
    return np.moveaxis(x, -1, axis)


def apply32(op, a32, stretch=None, axis=-1):
    """solve(A32, B32 @ u32) [* stretch32] along `axis`, float32 throughout"""
    return _apply(op, a32, stretch, axis, np.float32)


def apply64(op, a, stretch=None, axis=-1):
    """the same pipeline in FP64: the reference of the yardstick"""
    return _apply(op, np.asarray(a, dtype=np.float64), stretch, axis, np.float64)


def _transeq(ops, u, v, w, nu, axis, tables, dt):
    conv = (u, v, w)[2 - axis]
    nu = dt(nu)
    out = []
    for f in (u, v, w):
        own = f is conv
        t1, t2, t3 = ("der1st", "der2nd", "der1st_sym") if own else ("der1st_sym", "der2nd_sym", "der1st")
        s1, s2, s3, cor = (None,) * 4 if tables is None else (tables[t1][0], tables[t2][0], tables[t3][0], tables[t2][1])
        du = _apply(ops[t1], f, s1, axis, dt)
        dud = _apply(ops[t3], conv * f, s3, axis, dt)
        d2u = _apply(ops[t2], f, s2, axis, dt)
        if cor is not None:
            shape = [1, 1, 1]
            shape[axis] = -1
            d2u = d2u + du * np.asarray(cor, dtype=dt).reshape(shape)
        r = dt(-0.5) * (conv * du + dud) + nu * d2u
        assert r.dtype == dt, r.dtype
        out.append(r)
    return out


def transeq32(ops, u, v, w, nu, axis, tables=None):
    """the float32 form of util.dense_transeq; tables: {operator: (stretch, stretch_correct)} of a stretched direction"""
    assert all(f.dtype == np.float32 for f in (u, v, w))
    return _transeq(ops, u, v, w, nu, axis, tables, np.float32)


def transeq64(ops, u, v, w, nu, axis, tables=None):
    return _transeq(ops, *[np.asarray(f, dtype=np.float64) for f in (u, v, w)], nu, axis, tables, np.float64)


def accumulate32(prev32, scale, r32):
    assert prev32.dtype == np.float32 and r32.dtype == np.float32
    out = prev32 + np.float32(scale) * r32
    assert out.dtype == np.float32
    return out


class Pipeline:
    """one case's dense operators, tables and inputs, and every check of the case in both precisions.
    checks() -> {name: (float32 result, FP64 result)}; the names are those tests/ops_sp_worker.py gives the kernels' results"""

    def __init__(self, tag, defect=None):
        """defect: None, "A" (every off-diagonal of A x (1 + 1e-5)) or "B" (the largest coefficient of row 1 of B
        x (1 + 1e-5)), applied to the float32 side only"""
        self.tag = tag
        self.dims, self.d, *_ = CASES[tag]
        self.axis = 3 - self.d
        self.o = oracle_solver(tag)
        m = self.o.mesh
        self.nu = self.o.nu
        self.dirps = [util.dense_dirps(int(m.vert_dims[k]), float(m.d[k]), int(m.BCs[k, 0]), int(m.BCs[k, 1])) for k in range(3)]
        self.ops = self.dirps[self.d - 1]
        odp = (self.o.xdirps, self.o.ydirps, self.o.zdirps)[self.d - 1]
        self.stretched = bool(m.stretched[self.d - 1])
        self.tables = {k: (getattr(odp, k).stretch.copy(), getattr(odp, k).stretch_correct.copy()) for k in util.OPNAMES} \
            if self.stretched else None
        self.ops32 = {k: defective(v, defect) for k, v in self.ops.items()}
        self.u, self.v, self.w = inputs_of(tag)
        self._memo = {}

    def stretch(self, op):
        return None if self.tables is None else self.tables[op][0]

    def both(self, op, which):
        """(apply32, apply64) of operator `op` on input field `which` ("u" / "v"), computed once"""
        if (op, which) not in self._memo:
            a = getattr(self, which)
            self._memo[op, which] = (apply32(self.ops32[op], a, self.stretch(op), self.axis),
                                     apply64(self.ops[op], a, self.stretch(op), self.axis))
        return self._memo[op, which]

    def cut(self, a, like):
        """a on the extent of `like` (an operator that moves to the cells of a walled direction returns one row fewer)"""
        n = like.shape[self.axis]
        return np.moveaxis(np.moveaxis(a, self.axis, -1)[..., :n], -1, self.axis)

    def checks(self, operators=True, transeq=True, solver_transeq=True):
        out = {}
        sc = ACC_SCALE[self.d]
        if operators:
            for op in util.OPNAMES:
                r32, r64 = self.both(op, "u")
                out["tds." + op] = (r32, r64)
                prev = self.cut(self.v, r32)  # (the accumulating form adds to another field, not to its own result)
                out["acc." + op] = (accumulate32(prev, sc, r32), prev.astype(np.float64) + sc * r64)
            for opa, opb in PAIRS:
                (a32, a64), (b32, b64), (c32, c64) = self.both(opa, "u"), self.both(opb, "v"), self.both(opb, "u")
                out["pair0.%s+%s" % (opa, opb)] = (a32 + b32, a64 + b64)
                out["pair1.%s.A" % opa] = (a32, a64)
                out["pair1.%s.B" % opb] = (c32, c64)
        if transeq:
            t32 = transeq32(self.ops32, self.u, self.v, self.w, self.nu, self.axis, self.tables)
            t64 = transeq64(self.ops, self.u, self.v, self.w, self.nu, self.axis, self.tables)
            for k, (a, b, prev) in enumerate(zip(t32, t64, (self.w, self.u, self.v))):
                out["transeq_dir." + "uvw"[k]] = (a, b)
                out["transeq_dir_acc." + "uvw"[k]] = (prev + a, prev.astype(np.float64) + b)
            if solver_transeq:
                s32, s64 = None, None
                for d in (1, 2, 3):  # x writes, y and z accumulate
                    if d == self.d:
                        a, b = t32, t64
                    else:
                        a = transeq32(self.dirps[d - 1], self.u, self.v, self.w, self.nu, 3 - d)
                        b = transeq64(self.dirps[d - 1], self.u, self.v, self.w, self.nu, 3 - d)
                    s32 = a if s32 is None else [x + y for x, y in zip(s32, a)]
                    s64 = b if s64 is None else [x + y for x, y in zip(s64, b)]
                for k in range(3):
                    assert s32[k].dtype == np.float32
                    out["transeq." + "uvw"[k]] = (s32[k], s64[k])
        return out

    def yardsticks(self, **kw):
        """{name: ((l2, max) of the float32 pipeline against the FP64 one)}"""
        return {k: errors(a, b) for k, (a, b) in self.checks(**kw).items()}


def oracle_results(p, operators=True, transeq=True):
    """the oracle in FP64 on the inputs of Pipeline p: {name: result} under the names of Pipeline.checks() -- the reference
    the kernels' errors are taken against"""
    from oracle import x3d_oracle as orc
    o, d = p.o, p.d
    b = o.backend
    fields = dict(u=o.u, v=o.v, w=o.w)
    for k, f in fields.items():
        f.data_loc = orc.VERT
        b.set_field_data(f, getattr(p, k).astype(np.float64))
    odp = (o.xdirps, o.ydirps, o.zdirps)[d - 1]
    memo = {}

    def one(op, which):
        if (op, which) not in memo:
            src = b.get_block(orc.DIR_X, orc.VERT)
            src.data[...] = fields[which].data
            src.data_loc = orc.move_data_loc(orc.VERT, d, 1) if op.endswith("p2v") else orc.VERT
            res = b.get_block(d)
            if d == 1:
                b.tds_solve(res, src, getattr(odp, op))
            else:
                a = b.get_block(d)
                b.reorder(a, src, 10 + d)
                b.tds_solve(res, a, getattr(odp, op))
            memo[op, which] = b.get_field_data(res)
        return memo[op, which]

    out = {}
    sc = ACC_SCALE[d]
    if operators:
        for op in util.OPNAMES:
            r = one(op, "u")
            out["tds." + op] = r
            out["acc." + op] = p.cut(p.v, r).astype(np.float64) + sc * r
        for opa, opb in PAIRS:
            out["pair0.%s+%s" % (opa, opb)] = one(opa, "u") + one(opb, "v")
            out["pair1.%s.A" % opa] = one(opa, "u")
            out["pair1.%s.B" % opb] = one(opb, "u")
    if transeq:
        rhs = [b.get_block(orc.DIR_X) for _ in range(3)]
        if d == 1:
            b.transeq_x(*rhs, o.u, o.v, o.w, o.nu, o.xdirps)
            got = [b.get_field_data(f, orc.VERT) for f in rhs]
        else:
            ins, outs = [b.get_block(d) for _ in range(3)], [b.get_block(d) for _ in range(3)]
            for a, f in zip(ins, (o.u, o.v, o.w)):
                b.reorder(a, f, 10 + d)
            (b.transeq_y if d == 2 else b.transeq_z)(*outs, *ins, o.nu, odp)
            got = [b.get_field_data(f, orc.VERT) for f in outs]
        for k, (r, prev) in enumerate(zip(got, (p.w, p.u, p.v))):
            out["transeq_dir." + "uvw"[k]] = r
            out["transeq_dir_acc." + "uvw"[k]] = prev.astype(np.float64) + r
        o.transeq(rhs, [o.u, o.v, o.w])
        for k, f in enumerate(rhs):
            out["transeq." + "uvw"[k]] = b.get_field_data(f, orc.VERT)
    return out


def defective(op, defect):
    """(A, B) with a relative 1e-5 defect: "A" -- every off-diagonal entry of A; "B" -- the largest coefficient of row 1 of B"""
    A, B = op
    if defect is None:
        return op
    if defect == "A":
        A = np.where(np.eye(A.shape[0], dtype=bool), A, A * (1.0 + 1e-5))
    elif defect == "B":
        B = B.copy()
        B[1, np.argmax(np.abs(B[1]))] *= 1.0 + 1e-5
    else:
        raise ValueError(defect)
    return A, B


def old_tolerance(name):
    """the tolerance tests/sp_worker.py holds the operator of this name to"""
    return OLD_TOL["loose" if ("der2nd" in name or name.startswith("transeq")) else "tight"]


def accepted(err, yard):
    return err[0] <= BOUND * yard[0] and err[1] <= BOUND * yard[1]
