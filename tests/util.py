"""helpers shared by the test modules"""
import io
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPNAMES = ["der1st", "der1st_sym", "der2nd", "der2nd_sym", "stagder_v2p", "stagder_p2v", "interpl_v2p",
           "interpl_p2v"]


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, f"ref_{name}.npz")))


def read_csv(name):
    with open(os.path.join(GOLDEN, f"ref_{name}.csv")) as f:
        rows = [l for l in f if not l.startswith("#")]
    return np.loadtxt(io.StringIO("".join(rows)), delimiter=",")


def read_trace_fixture(name="oracle_tgv64_rk3_fft"):
    """rows (time, enstrophy, div_u_max, div_u_mean, survey_enstrophy, survey_div_u_max) of a fixture written
    by oracle/gen_trace_fixture.py"""
    with open(os.path.join(GOLDEN, name + ".csv")) as f:
        rows = [l for l in f if not l.startswith("#")]
    return np.loadtxt(io.StringIO("".join(rows)), delimiter=",")


def namelist(g):
    """parse the namelist text stored in a fixture"""
    txt = bytes(g["cfg.namelist"]).decode()

    def get(key):
        return re.search(rf"^{key}\s*=\s*(.*)$", txt, re.M).group(1).strip()

    def nums(key, f=float):
        return [f(x.replace("d", "e")) for x in get(key).split(",")]

    def strs(key):
        return [x.strip().strip("'") for x in get(key).split(",")]

    return dict(dims=nums("dims_global", int), nproc=nums("nproc_dir", int), L=nums("L_global"),
                bcx=strs("BC_x"), bcy=strs("BC_y"), bcz=strs("BC_z"), stretching=strs("stretching"),
                beta=nums("beta"), Re=nums("Re")[0], dt=nums("dt")[0],
                time_intg=get("time_intg").strip("'"), interpl=get("interpl_scheme").strip("'"),
                der2nd=get("der2nd_scheme").strip("'"))


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def product_mesh(c, rank=0):
    from x3d2_amd.mesh import Mesh
    return Mesh(c["dims"], c["nproc"], c["L"], c["bcx"], c["bcy"], c["bcz"], c["stretching"], c["beta"],
                nrank=rank)


class ThreadComm:
    """lock-step exchange between oracle solvers that run as threads of this process (the oracle's comm
    interface: sendrecv / allreduce).  send_s goes to prev (arrives as its recv_e), send_e to next."""

    def __init__(self, rank, size, shared):
        self.rank, self.size, self.sh = rank, size, shared

    @staticmethod
    def shared(size):
        import threading
        return {"barrier": threading.Barrier(size), "box": {}}

    def sendrecv(self, send_s, send_e, prev, nxt):
        box, bar = self.sh["box"], self.sh["barrier"]
        box[(self.rank, "s")], box[(self.rank, "e")] = send_s, send_e
        bar.wait()
        recv_s, recv_e = box[(int(prev), "e")].copy(), box[(int(nxt), "s")].copy()
        bar.wait()
        return recv_s, recv_e

    def allreduce(self, x, op="sum"):
        box, bar = self.sh["box"], self.sh["barrier"]
        box[(self.rank, "r")] = x
        bar.wait()
        vals = [box[(r, "r")] for r in range(self.size)]  # fixed order: every rank gets the same bits
        bar.wait()
        return max(vals) if op == "max" else sum(vals)


def run_rank_threads(size, body):
    """body(rank, comm) -> result, one thread per rank; returns the list of results (exceptions re-raised)"""
    import threading
    sh = ThreadComm.shared(size)
    out, err = [None] * size, [None] * size

    def run(r):
        try:
            out[r] = body(r, ThreadComm(r, size, sh))
        except BaseException as e:  # noqa: BLE001 -- re-raised in the parent
            err[r] = e
            sh["barrier"].abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(size)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for e in err:
        if e is not None and not isinstance(e, __import__("threading").BrokenBarrierError):
            raise e
    for e in err:
        if e is not None:
            raise e
    return out


def stitch_ranks(parts, offsets, name):
    """assemble rank-local [k, j, i] arrays into the global one by their n_offset (x, y, z)"""
    ext = [max(int(o[d]) + p[name].shape[2 - d] for p, o in zip(parts, offsets)) for d in range(3)]
    full = np.zeros((ext[2], ext[1], ext[0]))
    for p, o in zip(parts, offsets):
        a = p[name]
        ox, oy, oz = (int(v) for v in o)
        full[oz:oz + a.shape[0], oy:oy + a.shape[1], ox:ox + a.shape[2]] = a
    return full


def BATTERY_FIELDS(dn):
    """dn: the decomposed direction(s), "y", "z" or "yz" (a 2-D pencil split runs the operators of both)"""
    return [f"tds.{d}.{op}" for d in dn for op in OPNAMES] + ["transeq.du", "transeq.dv", "transeq.dw", "div.div_u", "grad.dpdx",
            "grad.dpdy", "grad.dpdz", "curl.i", "curl.j", "curl.k", "step2.u", "step2.v", "step2.w"]


def oracle_battery(g, nranks):
    """the operator sequence oracle/ref/drivers/dump_golden.f90 drives the reference with, on the ORACLE with
    nranks ranks (threads exchanging in lock step) decomposed as the namelist in g says; inputs g["in.*"] are
    global arrays.  Returns (dict of stitched global fields, list of per-rank dicts)."""
    from oracle import x3d_oracle as orc
    c = namelist(g)
    ds = [k + 1 for k, p in enumerate(c["nproc"]) if int(p) > 1]  # every decomposed direction ([1, py, pz]: y and z)
    dn = "".join("xyz"[d - 1] for d in ds)

    def local(key, mesh):
        ox, oy, oz = (int(v) for v in mesh.n_offset)
        nx, ny, nz = (int(v) for v in mesh.vert_dims)
        return g[key][oz:oz + nz, oy:oy + ny, ox:ox + nx]

    def body(rank, comm):
        mesh = orc.Mesh(c["dims"], c["nproc"], c["L"], c["bcx"], c["bcy"], c["bcz"], c["stretching"], c["beta"],
                        rank=rank)
        s = orc.Solver(mesh, Re=c["Re"], dt=c["dt"], time_intg=c["time_intg"], poisson="CG", comm=comm,
                       interpl=c["interpl"], der2nd=c["der2nd"])
        if int(g.get("cfg.hyperviscous", [0])[0]):
            for dp in (s.xdirps, s.ydirps, s.zdirps):
                hyperviscous_der2nd(dp, mesh, orc.Tdsops)
        b = s.backend
        out = {}
        for f, k in ((s.u, "in.u"), (s.v, "in.v"), (s.w, "in.w")):
            f.data_loc = orc.VERT
            b.set_field_data(f, local(k, s.mesh))
        for d in ds:
            dp = (s.xdirps, s.ydirps, s.zdirps)[d - 1]
            for op in OPNAMES:
                src = b.get_block(orc.DIR_X, orc.VERT)
                b.veccopy(src, s.u)
                if op.endswith("p2v"):
                    src.data_loc = orc.move_data_loc(orc.VERT, d, 1)
                a, o = b.get_block(d), b.get_block(d)
                b.reorder(a, src, orc.RDR[(1, d)])
                b.tds_solve(o, a, getattr(dp, op))
                out[f"tds.{'xyz'[d - 1]}.{op}"] = b.get_field_data(o)
        rhs = [b.get_block(orc.DIR_X) for _ in range(3)]
        s.transeq(rhs, [s.u, s.v, s.w])
        for f, k in zip(rhs, ("du", "dv", "dw")):
            out["transeq." + k] = b.get_field_data(f)
        spec = b.get_block(orc.DIR_X, orc.VERT)
        b.set_field_data(spec, local("in.s", s.mesh))
        srhs = b.get_block(orc.DIR_X)
        s.transeq_species([srhs], [s.u, s.v, s.w, spec], [0.37 * s.nu])
        out["species.rhs"] = b.get_field_data(srhs, orc.VERT)
        div_u = b.get_block(orc.DIR_Z)
        s.divergence_v2p(div_u, s.u, s.v, s.w)
        out["div.div_u"] = b.get_field_data(div_u)
        out["div.maxmean"] = np.array(b.field_max_mean(div_u))
        s.gradient_p2v(*rhs, div_u)
        for f, k in zip(rhs, ("dpdx", "dpdy", "dpdz")):
            out["grad." + k] = b.get_field_data(f)
        for f in rhs:
            f.data_loc = orc.VERT
        s.curl(*rhs, s.u, s.v, s.w)
        for f, k in zip(rhs, "ijk"):
            out["curl." + k] = b.get_field_data(f)
        out["curl.enstrophy"] = np.array([0.5 * sum(b.scalar_product(f, f) for f in rhs) / s.ngrid])
        for it in range(2 * s.time_integrator.nstage):
            r3 = [b.get_block(orc.DIR_X) for _ in range(3)]
            s.transeq(r3, [s.u, s.v, s.w])
            s.time_integrator.step([s.u, s.v, s.w], r3, s.dt)
        for f, k in ((s.u, "u"), (s.v, "v"), (s.w, "w")):
            out["step2." + k] = b.get_field_data(f)
        return out, s.mesh.n_offset.copy()

    res = run_rank_threads(nranks, body)
    parts, offs = [r[0] for r in res], [r[1] for r in res]
    full = {k: stitch_ranks(parts, offs, k) for k in BATTERY_FIELDS(dn) + ["species.rhs"]}
    return full, parts


NML = """&domain_settings
flow_case_name = 'tgv'
L_global = 6.283185307179586d0, 6.283185307179586d0, 6.283185307179586d0
dims_global = {dims}
nproc_dir = {nproc}
BC_x = 'periodic', 'periodic'
BC_y = 'periodic', 'periodic'
BC_z = 'periodic', 'periodic'
stretching = 'uniform', 'uniform', 'uniform'
beta = 1d0, 1d0, 1d0
/End
&solver_params
Re = 1600d0
time_intg = 'RK3'
dt = 0.001d0
interpl_scheme = 'classic'
der2nd_scheme = 'compact6'
/End
"""


def synthetic_case(dims, nproc, seed=7, interpl="classic", hyperviscous=False):
    """a fixture-shaped dict (namelist + global inputs) for the operator battery: smooth fields + 10 % noise.
    hyperviscous: "cfg.hyperviscous" = 1, which the battery (tests/mp_fixture_worker.py) and oracle_battery honour by
    swapping der2nd / der2nd_sym for compact6-hyperviscous ones (hyperviscous_der2nd): the namelist has no c_nu"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    x = np.arange(nx)[None, None, :] * (2 * np.pi / nx)
    y = np.arange(ny)[None, :, None] * (2 * np.pi / ny)
    z = np.arange(nz)[:, None, None] * (2 * np.pi / nz)
    nml = NML.format(dims=", ".join(map(str, dims)), nproc=", ".join(map(str, nproc)))
    nml = nml.replace("interpl_scheme = 'classic'", f"interpl_scheme = '{interpl}'")
    g = {"cfg.namelist": np.frombuffer(nml.encode(), dtype=np.uint8)}
    if hyperviscous:
        g["cfg.hyperviscous"] = np.array([1])
    for k, (a, b_, c) in zip(("in.u", "in.v", "in.w", "in.s"), ((1, 2, 1), (2, 1, 3), (1, 1, 2), (3, 2, 1))):
        g[k] = np.sin(a * x + 0.3) * np.cos(b_ * y) * np.cos(c * z + 0.1) + 0.1 * rng.standard_normal((nz, ny, nx))
    return g


def hash_noise(gi, gj, gk, salt):
    """deterministic pseudo-noise in [-0.5, 0.5) from GLOBAL grid indices (broadcastable integer arrays): every rank
    of a decomposed run and the single-rank oracle evaluate the same expression on the same host, so they get the same
    bits without anybody holding the global array"""
    t = np.sin(gi * 12.9898 + gj * 78.233 + gk * 37.719 + salt * 0.618) * 43758.5453
    return t - np.floor(t) - 0.5


def noisy_tgv(dims, offset, local_dims, amp=0.1):
    """Taylor-Green velocity + amp * hash noise on the box [offset, offset + local_dims) of a 2 pi periodic grid of
    `dims` vertices; arrays [k, j, i]"""
    ox, oy, oz = (int(v) for v in offset)
    nx, ny, nz = (int(v) for v in local_dims)
    gi = np.arange(ox, ox + nx)[None, None, :]
    gj = np.arange(oy, oy + ny)[None, :, None]
    gk = np.arange(oz, oz + nz)[:, None, None]
    twopi = 6.283185307179586
    x, y, z = gi * (twopi / dims[0]), gj * (twopi / dims[1]), gk * (twopi / dims[2])
    u = np.sin(x) * np.cos(y) * np.cos(z) + amp * hash_noise(gi, gj, gk, 1)
    v = -np.cos(x) * np.sin(y) * np.cos(z) + amp * hash_noise(gi, gj, gk, 2)
    w = amp * hash_noise(gi, gj, gk, 3) + 0.0 * x * y
    return u, v, w


# ---- signatures of large fields (round 6): the 512^3 / 1024 x 257 x 512 oracle runs of the GPU suite (25 s ... 60 s of host
# time each on the GPU box) are paid ONCE, by oracle/gen_step_fixtures.py, which stores these signatures of the oracle's
# fields under tests/golden/oracle_big_steps.npz; the GPU tests then compare the HIP fields' signatures with them
def _sig_axes(shape):
    return [np.unique(np.linspace(0, n - 1, min(n, 24)).astype(np.int64)) for n in shape]


def _sig_weights(shape):
    """integer-hash weights in [-1, 1): a permutation of rows or planes changes the weighted sum"""
    nz, ny, nx = shape
    gk = np.arange(nz, dtype=np.int64)[:, None, None]
    gj = np.arange(ny, dtype=np.int64)[None, :, None]
    gi = np.arange(nx, dtype=np.int64)[None, None, :]
    return (((gi * 7 + gj * 13 + gk * 29 + (gi * gj + gk) * 3) % 64) - 31.5) / 32.0


def field_signature(a):
    """a: [nz, ny, nx] -> {sample (a 24^3 lattice incl. the corners), sum, sumabs, sumsq, wsum, absmax}"""
    a = np.asarray(a, dtype=np.float64)
    iz, iy, ix = _sig_axes(a.shape)
    return {"sample": a[np.ix_(iz, iy, ix)].copy(), "sum": np.float64(a.sum()), "sumabs": np.float64(np.abs(a).sum()),
            "sumsq": np.float64(np.vdot(a, a)), "wsum": np.float64((a * _sig_weights(a.shape)).sum()),
            "absmax": np.float64(np.abs(a).max())}


def assert_signature(a, sig, rel, what="", scale=None):
    """the field a against a stored signature: every sampled point within rel * absmax; the plain and the hash-weighted
    sums within 50 sqrt(n) rel absmax (round-off differences of up to rel * absmax per point add up like a random walk; a
    coherent deviation of a tenth of that per point is caught); the sum of squares within 2 rel absmax sum|a|"""
    got = field_signature(a)
    scale = max(float(sig["absmax"]), 1e-300) if scale is None else float(scale)  # (scale given: an absolute tolerance)
    assert got["sample"].shape == sig["sample"].shape, what
    assert np.max(np.abs(got["sample"] - sig["sample"])) <= rel * scale, (what, "sample", float(np.max(np.abs(got["sample"] - sig["sample"]))))
    n = a.size
    for k in ("sum", "wsum"):
        assert abs(got[k] - float(sig[k])) <= 50.0 * np.sqrt(n) * rel * scale, (what, k, float(got[k]), float(sig[k]))
    assert abs(got["sumsq"] - float(sig["sumsq"])) <= 2.0 * rel * scale * float(sig["sumabs"]) + 1e-300, (what, "sumsq")
    assert abs(got["absmax"] - float(sig["absmax"])) <= rel * scale, (what, "absmax")


def load_big_steps():
    p = os.path.join(GOLDEN, "oracle_big_steps.npz")
    return dict(np.load(p)) if os.path.exists(p) else None


def signature_of(fix, prefix):
    return {k: fix[prefix + "." + k] for k in ("sample", "sum", "sumabs", "sumsq", "wsum", "absmax")}


# ---- dense float64 references of the compact operators (uniform grids)
def dense_operator(n, delta, operation, scheme, bc_s, bc_e, from_to=None, sym=None, c_nu=None, nu0_nu=None):
    """(A, B) of one compact operator as dense float64 matrices, result = solve(A, B @ u): A the tridiagonal left-hand
    side before its factorisation (dist_b on the diagonal, dist_sa below, dist_sc above, corners when periodic), B the
    right-hand side stencils (coeffs_s for rows 0..3, coeffs_e for the last 4 rows of n_rhs, coeffs in between; row j reads
    input j + m - 4; periodic operators wrap, others drop what falls outside [0, n_rhs)).  A is n x n, B is n x n_rhs.
    Stretch factors are not applied: uniform grids only.  Valid as a reference of the distributed algorithm (truncated
    2 x 2 coupling) only where rho^n of the solve is negligible."""
    from x3d2_amd.tdsops import Tdsops

    class _Raw(Tdsops):
        def _preprocess_dist(self, b):
            self.raw = (np.array(b[:self.n_tds]), self.dist_sa[:self.n_tds].copy(), self.dist_sc[:self.n_tds].copy())
            super()._preprocess_dist(b)

    t = _Raw(n, delta, operation, scheme, bc_s, bc_e, from_to=from_to, sym=sym, c_nu=c_nu, nu0_nu=nu0_nu)
    diag, sa, sc = t.raw
    A = np.diag(diag) + np.diag(sa[1:], -1) + np.diag(sc[:-1], 1)
    if t.periodic:
        A[0, n - 1] += sa[0]
        A[n - 1, 0] += sc[n - 1]
    n_in = t.n_rhs
    B = np.zeros((n, n_in))
    for j in range(n):
        c = t.coeffs_s[j] if j < 4 else (t.coeffs_e[j - (n_in - 4)] if j >= n_in - 4 else t.coeffs)
        for m in range(9):
            i = j + m - 4
            if t.periodic:
                i %= n_in
            elif not 0 <= i < n_in:
                continue
            B[j, i] += c[m]
    return A, B


def dense_dirps(n_vert, delta, bc_s, bc_e, interpl="classic", der2nd="compact6", c_nu=None, nu0_nu=None):
    """{operator name: (A, B)} of one direction, with the schemes and end conditions allocate_tdsops gives them (Dirichlet
    ends -> Neumann for the midpoint operators)"""
    from x3d2_amd.common import BC_DIRICHLET, BC_NEUMANN, BC_PERIODIC
    mp_s = BC_NEUMANN if bc_s == BC_DIRICHLET else bc_s
    mp_e = BC_NEUMANN if bc_e == BC_DIRICHLET else bc_e
    n_cell = n_vert if bc_s == BC_PERIODIC and bc_e == BC_PERIODIC else n_vert - 1
    d2 = dict(c_nu=c_nu, nu0_nu=nu0_nu)
    return {"der1st": dense_operator(n_vert, delta, "first-deriv", "compact6", bc_s, bc_e),
            "der1st_sym": dense_operator(n_vert, delta, "first-deriv", "compact6", bc_s, bc_e, sym=True),
            "der2nd": dense_operator(n_vert, delta, "second-deriv", der2nd, bc_s, bc_e, **d2),
            "der2nd_sym": dense_operator(n_vert, delta, "second-deriv", der2nd, bc_s, bc_e, sym=True, **d2),
            "stagder_v2p": dense_operator(n_cell, delta, "stag-deriv", "compact6", mp_s, mp_e, from_to="v2p"),
            "stagder_p2v": dense_operator(n_vert, delta, "stag-deriv", "compact6", mp_s, mp_e, from_to="p2v"),
            "interpl_v2p": dense_operator(n_cell, delta, "interpolate", interpl, mp_s, mp_e, from_to="v2p"),
            "interpl_p2v": dense_operator(n_vert, delta, "interpolate", interpl, mp_s, mp_e, from_to="p2v")}


def dense_apply(op, a, axis):
    """solve(A, B @ u) along `axis` of the array a (which holds at least n_rhs points along it)"""
    A, B = op
    u = np.moveaxis(np.asarray(a, dtype=np.float64), axis, -1)[..., :B.shape[1]]
    r = np.linalg.solve(A, B @ u.reshape(-1, B.shape[1]).T).T
    return np.moveaxis(r.reshape(u.shape[:-1] + (A.shape[0],)), -1, axis)


def dense_transeq(ops, u, v, w, nu, axis):
    """the convection-diffusion terms of one direction (transeq_dist_component: -1/2 (c du/dx + d(c u)/dx) + nu d2u/dx2,
    c the velocity component along `axis`) for the three components, vertex fields [k, j, i].  The component along the
    direction: der1st, der2nd and der1st_sym for c c; the others: der1st_sym, der2nd_sym and der1st for c u."""
    conv = (u, v, w)[2 - axis]
    out = []
    for f in (u, v, w):
        own = f is conv
        t1, t2, t3 = ("der1st", "der2nd", "der1st_sym") if own else ("der1st_sym", "der2nd_sym", "der1st")
        out.append(-0.5 * (conv * dense_apply(ops[t1], f, axis) + dense_apply(ops[t3], conv * f, axis))
                   + nu * dense_apply(ops[t2], f, axis))
    return out


HYPERVISCOUS = dict(c_nu=0.22, nu0_nu=63.0)  # the reference's own test values for compact6-hyperviscous


def hyperviscous_der2nd(dirps, mesh, alloc):
    """replace dirps.der2nd / der2nd_sym by compact6-hyperviscous ones (neither allocate_tdsops passes c_nu), allocated
    with the arguments allocate_tdsops gives them; alloc = HipBackend.alloc_tdsops (product mesh) or the oracle's
    Tdsops (oracle mesh)"""
    d0 = dirps.dir - 1
    bc_s, bc_e = int(mesh.BCs[d0, 0]), int(mesh.BCs[d0, 1])
    n = int(mesh.vert_dims[d0])
    vds2, vd2s = np.asarray(mesh.vert_ds2[d0])[:n], np.asarray(mesh.vert_d2s[d0])[:n]
    for k, sym in (("der2nd", False), ("der2nd_sym", True)):
        setattr(dirps, k, alloc(n, float(mesh.d[d0]), "second-deriv", "compact6-hyperviscous", bc_s, bc_e, stretch=vds2,
                                stretch_correct=vd2s, sym=sym, **HYPERVISCOUS))


# ---------------------------------------------------------------- operator batteries against the oracle (GPU tests)
# The bodies of test_hip_parity.py's test_x_direction_scan_kernels_full_size_pencils and
# test_yz_operators_on_512_row_pencils, shared with tests/test_hip_work_counts.py.  `got`, when given, collects every
# compared array of the product under the names tests/ops_sp_worker.py uses ("tds.<op>", "acc.<op>", "pair0.<a>+<b>",
# "pair1.<a>.A", "pair1.<b>.B", "transeq_dir.<c>", "transeq_dir_acc.<c>", "transeq.<c>"), and `worst` the largest relerr
# of the battery under "relerr".  full=True adds what one of the two bodies has and the other lacks, so that both give the
# same 31 results: the pairs on x; the direction's transeq on y / z; its accumulating form on all three.
def _pair_battery(s, o, d, dp_h, dp_o, tol, note):
    """operator pairs of the pressure correction (x3d_tds_solve_pair; one tile kernel for y pencils)"""
    from oracle import x3d_oracle as orc
    from x3d2_amd.common import DIR_X, VERT, move_data_loc
    b, al = s.backend, s.backend.allocator

    def oracle_op(fo, t_o):
        src_o = o.backend.get_block(orc.DIR_X, orc.VERT)
        src_o.data[...] = fo.data
        src_o.data_loc = fo.data_loc
        out_o = o.backend.get_block(d)
        if d == 1:
            o.backend.tds_solve(out_o, src_o, t_o)
        else:
            a_o = o.backend.get_block(d)
            o.backend.reorder(a_o, src_o, 10 + d)
            o.backend.tds_solve(out_o, a_o, t_o)
        return o.backend.get_field_data(out_o)
    for opa, opb in (("interpl_v2p", "stagder_v2p"), ("interpl_p2v", "stagder_p2v")):
        loc = VERT if opa.endswith("v2p") else move_data_loc(VERT, d, 1)
        ins = [al.get_block(DIR_X), al.get_block(DIR_X)]
        for f_, src in zip(ins, (s.u, s.v)):
            b.veccopy(f_, src)
            f_.set_data_loc(loc)
        for fo in (o.u, o.v):
            fo.data_loc = loc
        o1, o2 = al.get_block(DIR_X), al.get_block(DIR_X)
        ta, tb = getattr(dp_h, opa), getattr(dp_h, opb)
        ra, rb2 = oracle_op(o.u, getattr(dp_o, opa)), oracle_op(o.v, getattr(dp_o, opb))
        rb1 = oracle_op(o.u, getattr(dp_o, opb))
        b.tds_pair(0, o1, None, ins[0], ins[1], ta, tb, d)
        o1.set_data_loc(move_data_loc(loc, d, ta.move))
        assert note("pair0.%s+%s" % (opa, opb), b.get_field_data(o1), ra + rb2) < tol, (opa, opb, "mode 0")
        b.tds_pair(1, o1, o2, ins[0], None, ta, tb, d)
        o2.set_data_loc(move_data_loc(loc, d, tb.move))
        assert note("pair1.%s.A" % opa, b.get_field_data(o1), ra) < tol, (opa, opb, "mode 1 / A")
        assert note("pair1.%s.B" % opb, b.get_field_data(o2), rb1) < tol, (opa, opb, "mode 1 / B")
        for fo in (o.u, o.v):
            fo.data_loc = orc.VERT
        for f_ in ins + [o1, o2]:
            al.release_block(f_)


def _noter(got, worst):
    def note(name, a, ref):
        e = relerr(a, ref)
        if got is not None and name is not None:
            got[name] = a
        if worst is not None:
            worst["relerr"] = max(worst.get("relerr", 0.0), e)
        return e
    return note


def x_operator_battery(dims, L, seed, tol, three_in_one=None, full=False, got=None, worst=None):
    """periodic x pencils: every x operator, the lincomb prologue (bits), transeq_x and the fused driver's accumulating
    forms against the oracle.  three_in_one: True / False -- the three-components-in-one counter rises by one / stays
    across transeq_x; None: not asserted.  -> the product's solver"""
    from oracle import x3d_oracle as orc
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.common import DIR_X, VERT, move_data_loc
    from x3d2_amd.solver import Solver, SolverConfig
    nx = dims[0]
    note = _noter(got, worst)
    per = ("periodic",) * 2
    mesh = Mesh(dims, (1, 1, 1), L, per, per, per)
    s = Solver(HipBackend(mesh), mesh, SolverConfig(poisson_solver_type="CG", fused=True))
    om = orc.Mesh(list(dims), [1, 1, 1], list(L), list(per), list(per), list(per))
    o = orc.Solver(om, poisson="CG")
    rng = np.random.default_rng(seed)
    b, al = s.backend, s.backend.allocator
    fields = []
    for fo, fp in ((o.u, s.u), (o.v, s.v), (o.w, s.w)):
        a = rng.standard_normal((dims[2], dims[1], nx))
        fo.data_loc = orc.VERT
        o.backend.set_field_data(fo, a)
        fp.set_data_loc(VERT)
        b.set_field_data(fp, a)
        fields.append(a)
    # all 8 operators along x
    for op in OPNAMES:
        t_h, t_o = getattr(s.xdirps, op), getattr(o.xdirps, op)
        src_h, src_o = al.get_block(DIR_X, VERT), o.backend.get_block(orc.DIR_X, orc.VERT)
        b.veccopy(src_h, s.u)
        src_o.data[...] = o.u.data
        if op.endswith("p2v"):
            src_h.set_data_loc(move_data_loc(VERT, 1, 1))
            src_o.data_loc = orc.move_data_loc(orc.VERT, 1, 1)
        out_h, out_o = al.get_block(DIR_X), o.backend.get_block(orc.DIR_X)
        b.tds_solve(out_h, src_h, t_h)
        o.backend.tds_solve(out_o, src_o, t_o)
        ref = o.backend.get_field_data(out_o)
        assert note("tds." + op, b.get_field_data(out_h), ref) < tol, op
        # accumulating form: out += -0.5 * T(u)
        b.tds_apply(out_h, src_h, t_h, DIR_X, accumulate=True, scale=-0.5)
        assert note("acc." + op, b.get_field_data(out_h), 0.5 * ref) < tol, op + " (accumulate)"
        for f in (src_h, out_h):
            al.release_block(f)
    if full:
        _pair_battery(s, o, 1, s.xdirps, o.xdirps, tol, note)
    # the RK stage's linear combination as the prologue of an x operator (x3d_tds_solve_lincomb): same bits as
    # lincomb followed by tds_solve
    y1, y2, d1, d2 = (al.get_block(DIR_X, VERT) for _ in range(4))
    coefs = [0.3, -1.7, 0.01]
    b.lincomb(y1, s.u, coefs, [s.v, s.w, s.u])
    b.tds_apply(d1, y1, s.xdirps.stagder_v2p, DIR_X)
    b.tds_lincomb(d2, s.xdirps.stagder_v2p, DIR_X, y2, s.u, coefs, [s.v, s.w, s.u])
    for f in (d1, d2):
        f.set_data_loc(move_data_loc(VERT, 1, 1))
    assert np.array_equal(b.get_field_data(y1), b.get_field_data(y2))
    assert np.array_equal(b.get_field_data(d1), b.get_field_data(d2))
    for f in (y1, y2, d1, d2):
        al.release_block(f)
    # transeq along x only, then the whole fused right-hand side (x writes, y and z accumulate)
    rhs_h = [al.get_block(DIR_X) for _ in range(3)]
    rhs_o = [o.backend.get_block(orc.DIR_X) for _ in range(3)]
    n3 = int(b.lib.x3d_backend_counter(b.h, 0))
    b.transeq_x(*rhs_h, s.u, s.v, s.w, s.nu, s.xdirps)
    if three_in_one is not None:  # True: the three-components-in-one kernels took it
        assert int(b.lib.x3d_backend_counter(b.h, 0)) == n3 + (1 if three_in_one else 0)
    o.backend.transeq_x(*rhs_o, o.u, o.v, o.w, o.nu, o.xdirps)
    refs = [o.backend.get_field_data(fo, orc.VERT) for fo in rhs_o]
    for fh, ref, nm in zip(rhs_h, refs, "uvw"):
        assert note("transeq_dir." + nm, b.get_field_data(fh, VERT), ref) < tol, nm
    if full:
        _transeq_dir_acc(s, 1, s.xdirps, rhs_h, refs, fields, tol, note)
    s.transeq(rhs_h, [s.u, s.v, s.w])
    o.transeq(rhs_o, [o.u, o.v, o.w])
    for fh, fo, nm in zip(rhs_h, rhs_o, "uvw"):
        assert note("transeq." + nm, b.get_field_data(fh, VERT), o.backend.get_field_data(fo, orc.VERT)) < tol, nm
    return s


def _transeq_dir_acc(s, d, dp_h, rhs_h, refs, fields, tol, note):
    """the direction's transeq added to other fields (w, u, v), against those fields + the oracle's plain result"""
    from x3d2_amd.common import VERT
    b = s.backend
    prevs = (fields[2], fields[0], fields[1])
    for f, prev in zip(rhs_h, (s.w, s.u, s.v)):
        b.veccopy(f, prev)
    b.transeq_dir(d, *rhs_h, s.u, s.v, s.w, s.nu, dp_h, accumulate=True)
    for fh, ref, prev, nm in zip(rhs_h, refs, prevs, "uvw"):
        assert note("transeq_dir_acc." + nm, b.get_field_data(fh, VERT), prev + ref) < tol, nm + " (accumulate)"


def yz_operator_battery(dims, bc, stretch, tol, d=None, seed=7, full=False, got=None, worst=None):
    """y / z pencils (d: 2 / 3; None: y where dims[1] >= 128): every operator incl. accumulating forms, Solver.transeq and
    the operator pairs against the oracle.  -> the product's solver"""
    from oracle import x3d_oracle as orc
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.common import DIR_X, VERT, move_data_loc
    from x3d2_amd.solver import Solver, SolverConfig
    note = _noter(got, worst)
    L = (2.0, 3.0, 2.5)
    per = ("periodic",) * 2
    if d is None:
        d = 2 if dims[1] >= 128 else 3
    bcs = [per, (bc,) * 2 if d == 2 else per, (bc,) * 2 if d == 3 else per]
    strs = ("uniform", stretch, "uniform")
    beta = (1.0, 0.259065151 if stretch == "top-bottom" else 1.3, 1.0)
    mesh = Mesh(dims, (1, 1, 1), L, *bcs, strs, beta)
    s = Solver(HipBackend(mesh), mesh, SolverConfig(poisson_solver_type="CG", fused=True))
    om = orc.Mesh(list(dims), [1, 1, 1], list(L), *[list(x) for x in bcs], stretching=strs, beta=beta)
    o = orc.Solver(om, poisson="CG")
    rng = np.random.default_rng(seed)
    b, al = s.backend, s.backend.allocator
    fields = []
    for fo, fp in ((o.u, s.u), (o.v, s.v), (o.w, s.w)):
        a = rng.standard_normal((dims[2], dims[1], dims[0]))
        fo.data_loc = orc.VERT
        o.backend.set_field_data(fo, a)
        fp.set_data_loc(VERT)
        b.set_field_data(fp, a)
        fields.append(a)
    dp_h, dp_o = (s.ydirps, o.ydirps) if d == 2 else (s.zdirps, o.zdirps)
    for op in OPNAMES:
        t_h, t_o = getattr(dp_h, op), getattr(dp_o, op)
        loc = move_data_loc(VERT, d, 1) if op.endswith("p2v") else VERT
        src_h, src_o = al.get_block(DIR_X, VERT), o.backend.get_block(orc.DIR_X, orc.VERT)
        b.veccopy(src_h, s.u)
        src_o.data[...] = o.u.data
        src_h.set_data_loc(loc)
        src_o.data_loc = loc
        a_o, out_o = o.backend.get_block(d), o.backend.get_block(d)
        o.backend.reorder(a_o, src_o, 10 + d)
        o.backend.tds_solve(out_o, a_o, t_o)
        ref = o.backend.get_field_data(out_o)
        out_h = al.get_block(DIR_X)
        b.tds_apply(out_h, src_h, t_h, d)
        out_h.set_data_loc(out_o.data_loc)
        assert note("tds." + op, b.get_field_data(out_h), ref) < tol, op
        b.tds_apply(out_h, src_h, t_h, d, accumulate=True, scale=0.25)
        assert note("acc." + op, b.get_field_data(out_h), 1.25 * ref) < tol, op + " (accumulate)"
        for f in (src_h, out_h):
            al.release_block(f)
    rhs_h = [al.get_block(DIR_X) for _ in range(3)]
    rhs_o = [o.backend.get_block(orc.DIR_X) for _ in range(3)]
    if full:  # the direction's transeq alone, plain and accumulating
        ins, outs = [o.backend.get_block(d) for _ in range(3)], [o.backend.get_block(d) for _ in range(3)]
        for a_o, fo in zip(ins, (o.u, o.v, o.w)):
            o.backend.reorder(a_o, fo, 10 + d)
        (o.backend.transeq_y if d == 2 else o.backend.transeq_z)(*outs, *ins, o.nu, dp_o)
        refs = [o.backend.get_field_data(f, orc.VERT) for f in outs]
        b.transeq_dir(d, *rhs_h, s.u, s.v, s.w, s.nu, dp_h, accumulate=False)
        for fh, ref, nm in zip(rhs_h, refs, "uvw"):
            assert note("transeq_dir." + nm, b.get_field_data(fh, VERT), ref) < tol, nm
        _transeq_dir_acc(s, d, dp_h, rhs_h, refs, fields, tol, note)
    s.transeq(rhs_h, [s.u, s.v, s.w])
    o.transeq(rhs_o, [o.u, o.v, o.w])
    for fh, fo, nm in zip(rhs_h, rhs_o, "uvw"):
        assert note("transeq." + nm, b.get_field_data(fh, VERT), o.backend.get_field_data(fo, orc.VERT)) < tol, nm
    _pair_battery(s, o, d, dp_h, dp_o, tol, note)
    return s


def library_switch_names():
    """the names of the library's switch table (x3d2_amd/csrc/switches.hip), in its order"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "x3d2_amd", "csrc", "switches.hip")) as fh:
        txt = fh.read()
    body = txt[txt.index("g_table[] = {"):]
    return re.findall(r'"(X3D_[A-Z0-9_]+)"', body[:body.index("\n};")])

