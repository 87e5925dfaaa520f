"""The size-specialised kernels in their wide-stencil forms.  The default schemes (compact6 derivatives, classic
interpolation) reach at most two rows on either side, and every launcher then picks its NARROW instantiation; the other
schemes of the reference -- compact6-hyperviscous second derivatives (all 9 taps), optimised (taps 1..8 / 0..7) and
aggressive (2..7 / 1..6) interpolation, with slower-decaying solves -- run the NARROW = false kernels: their own tap
loops, LDS stencil slots and strip depths.  Each case compares the HIP result with the dense float64 solve of the same
operator (tests/util.py dense_operator, where rho^n of the solve is negligible: it is then the exact answer of the
distributed algorithm too) and with the oracle on the same inputs.  Random fields, 1e-12 relative (max norm)."""
import os

import numpy as np
import pytest

from util import HYPERVISCOUS, OPNAMES, dense_apply, dense_dirps, dense_transeq, hyperviscous_der2nd, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-12


def _solvers(dims, bcs, interpl, hyper, strs=("uniform",) * 3, beta=(1.0, 1.0, 1.0), L=(2.0, 3.0, 2.5)):
    """the product's fused solver and the oracle's on the same mesh and schemes; hyper: compact6-hyperviscous der2nd /
    der2nd_sym in every direction of both"""
    from oracle import x3d_oracle as orc
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.solver import Solver, SolverConfig
    mesh = Mesh(dims, (1, 1, 1), L, *bcs, strs, beta)
    s = Solver(HipBackend(mesh), mesh, SolverConfig(poisson_solver_type="CG", fused=True, interpl_scheme=interpl))
    om = orc.Mesh(list(dims), [1, 1, 1], list(L), *[list(x) for x in bcs], stretching=strs, beta=beta)
    o = orc.Solver(om, poisson="CG", interpl=interpl)
    if hyper:
        for dp in (s.xdirps, s.ydirps, s.zdirps):
            hyperviscous_der2nd(dp, mesh, s.backend.alloc_tdsops)
        for dp in (o.xdirps, o.ydirps, o.zdirps):
            hyperviscous_der2nd(dp, om, orc.Tdsops)
    return s, o, mesh


def _random_velocity(s, o, dims, seed):
    from oracle import x3d_oracle as orc
    from x3d2_amd.common import VERT
    rng = np.random.default_rng(seed)
    arrays = []
    for fo, fp in ((o.u, s.u), (o.v, s.v), (o.w, s.w)):
        a = rng.standard_normal((dims[2], dims[1], dims[0]))
        fo.data_loc = orc.VERT
        o.backend.set_field_data(fo, a)
        fp.set_data_loc(VERT)
        s.backend.set_field_data(fp, a)
        arrays.append(a)
    return arrays


def _rho(op):
    """decay rate per row of the operator's tridiagonal solve (from its bulk alpha)"""
    A = op[0]
    m = A.shape[0] // 2
    al = A[m, m + 1] / A[m, m]
    return (1.0 - np.sqrt(1.0 - 4.0 * al * al)) / (2.0 * al)


def _dense(mesh, d, interpl, hyper, uniform=True):
    """{op: (A, B)} of direction d, entries None where the dense solve is no reference (rho^n >= 1e-16); None on a
    stretched grid"""
    if not uniform:
        return None
    d0 = d - 1
    n = int(mesh.vert_dims[d0])
    kw = dict(der2nd="compact6-hyperviscous", **HYPERVISCOUS) if hyper else {}
    ops = dense_dirps(n, float(mesh.d[d0]), int(mesh.BCs[d0, 0]), int(mesh.BCs[d0, 1]), interpl=interpl, **kw)
    return {k: (v if _rho(v) ** n < 1e-16 else None) for k, v in ops.items()}


def _oracle_op(o, d, fo, t_o):
    from oracle import x3d_oracle as orc
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


def _check_operators(s, o, d, dense, arrays):
    """every operator of direction d, plain and accumulating, against the oracle and the dense solve"""
    from x3d2_amd.common import DIR_X, VERT, move_data_loc
    b, al = s.backend, s.backend.allocator
    dp_h, dp_o = (s.xdirps, s.ydirps, s.zdirps)[d - 1], (o.xdirps, o.ydirps, o.zdirps)[d - 1]
    for op in OPNAMES:
        t_h = getattr(dp_h, op)
        loc = move_data_loc(VERT, d, 1) if op.endswith("p2v") else VERT
        o.u.data_loc = loc
        ref = _oracle_op(o, d, o.u, getattr(dp_o, op))
        src_h, out_h = al.get_block(DIR_X, VERT), al.get_block(DIR_X)
        b.veccopy(src_h, s.u)
        src_h.set_data_loc(loc)
        b.tds_apply(out_h, src_h, t_h, d)
        out_h.set_data_loc(move_data_loc(loc, d, t_h.move))
        got = b.get_field_data(out_h)
        assert relerr(got, ref) < TOL, (op, relerr(got, ref))
        if dense is not None and dense[op] is not None:
            want = dense_apply(dense[op], arrays[0], 3 - d)
            assert relerr(got, want) < TOL, (op, "dense", relerr(got, want))
        b.tds_apply(out_h, src_h, t_h, d, accumulate=True, scale=0.25)
        assert relerr(b.get_field_data(out_h), 1.25 * ref) < TOL, op + " (accumulate)"
        for f in (src_h, out_h):
            al.release_block(f)
    o.u.data_loc = VERT


def _check_transeq(s, o, d, dense, arrays):
    """the convection-diffusion terms of direction d alone (plain and accumulating), then the whole right-hand side"""
    from oracle import x3d_oracle as orc
    from x3d2_amd.common import DIR_X, VERT
    b, al = s.backend, s.backend.allocator
    dp_h, dp_o = (s.xdirps, s.ydirps, s.zdirps)[d - 1], (o.xdirps, o.ydirps, o.zdirps)[d - 1]
    rhs_h = [al.get_block(DIR_X) for _ in range(3)]
    b.transeq_dir(d, *rhs_h, s.u, s.v, s.w, s.nu, dp_h, accumulate=False)
    if d == 1:
        rhs_o = [o.backend.get_block(orc.DIR_X) for _ in range(3)]
        o.backend.transeq_x(*rhs_o, o.u, o.v, o.w, o.nu, dp_o)
    else:
        vel = [o.backend.get_block(d) for _ in range(3)]
        rhs_o = [o.backend.get_block(d) for _ in range(3)]
        for fd, fo in zip(vel, (o.u, o.v, o.w)):
            o.backend.reorder(fd, fo, 10 + d)
        (o.backend.transeq_y if d == 2 else o.backend.transeq_z)(*rhs_o, *vel, o.nu, dp_o)
    refs = [o.backend.get_field_data(f, orc.VERT) for f in rhs_o]
    want = None
    if dense is not None and all(dense[k] is not None for k in ("der1st", "der1st_sym", "der2nd", "der2nd_sym")):
        want = dense_transeq(dense, *arrays, s.nu, 3 - d)
    for k, (fh, ref) in enumerate(zip(rhs_h, refs)):
        got = b.get_field_data(fh, VERT)
        assert relerr(got, ref) < TOL, ("uvw"[k], relerr(got, ref))
        if want is not None:
            assert relerr(got, want[k]) < TOL, ("uvw"[k], "dense", relerr(got, want[k]))
    b.transeq_dir(d, *rhs_h, s.u, s.v, s.w, s.nu, dp_h, accumulate=True)
    for k, (fh, ref) in enumerate(zip(rhs_h, refs)):
        assert relerr(b.get_field_data(fh, VERT), 2.0 * ref) < TOL, ("uvw"[k], "accumulate")
    rhs_o = [o.backend.get_block(orc.DIR_X) for _ in range(3)]
    s.transeq(rhs_h, [s.u, s.v, s.w])
    o.transeq(rhs_o, [o.u, o.v, o.w])
    for fh, fo, nm in zip(rhs_h, rhs_o, "uvw"):
        assert relerr(b.get_field_data(fh, VERT), o.backend.get_field_data(fo, orc.VERT)) < TOL, (nm, "Solver.transeq")
    for f in rhs_h:
        al.release_block(f)


def _check_pairs(s, o, d, dense, arrays):
    """the pressure correction's operator pairs (x3d_tds_solve_pair), modes 0 and 1"""
    from oracle import x3d_oracle as orc
    from x3d2_amd.common import DIR_X, VERT, move_data_loc
    b, al = s.backend, s.backend.allocator
    dp_h, dp_o = (s.xdirps, s.ydirps, s.zdirps)[d - 1], (o.xdirps, o.ydirps, o.zdirps)[d - 1]
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
        ra, rb2 = _oracle_op(o, d, o.u, getattr(dp_o, opa)), _oracle_op(o, d, o.v, getattr(dp_o, opb))
        rb1 = _oracle_op(o, d, o.u, getattr(dp_o, opb))
        if dense is not None and dense[opa] is not None and dense[opb] is not None:
            da = dense_apply(dense[opa], arrays[0], 3 - d)
            assert relerr(ra + rb2, da + dense_apply(dense[opb], arrays[1], 3 - d)) < TOL, (opa, "oracle vs dense")
        b.tds_pair(0, o1, None, ins[0], ins[1], ta, tb, d)
        o1.set_data_loc(move_data_loc(loc, d, ta.move))
        assert relerr(b.get_field_data(o1), ra + rb2) < TOL, (opa, opb, "mode 0")
        b.tds_pair(1, o1, o2, ins[0], None, ta, tb, d)
        o2.set_data_loc(move_data_loc(loc, d, tb.move))
        assert relerr(b.get_field_data(o1), ra) < TOL, (opa, opb, "mode 1 / A")
        assert relerr(b.get_field_data(o2), rb1) < TOL, (opa, opb, "mode 1 / B")
        for fo in (o.u, o.v):
            fo.data_loc = orc.VERT
        for f in ins + [o1, o2]:
            al.release_block(f)


X_CASES = [(nx, "periodic", interpl) for nx in (128, 192, 256, 320, 384, 500, 512, 1024) for interpl in ("optimised", "aggressive")]
X_CASES += [(nx, "neumann", interpl) for nx in (512, 1024) for interpl in ("optimised", "aggressive")]


@pytest.mark.parametrize("nx,bc,interpl", X_CASES)
def test_x_kernels_with_wide_stencils(nx, bc, interpl):
    """x pencils: 256 / 512 -> k_xscan_* FAST forms (Q = 4 / 8), 192 / 320 / 384 / 500 -> the Q = 6 and generic forms,
    128 -> the LDS-tiled kernels, 1024 -> csrc/xwide.hip (Q = 16; 'aggressive' interpolation decays too slowly for the
    compressed lane tables, rho^128 = 6e-12: its operators must decline xwide and fall back).  Hyperviscous der2nd in
    every case.  Every operator, transeq_x (three components in one launch where that applies), Solver.transeq and
    tds_lincomb (same bits as lincomb + tds_apply)."""
    from x3d2_amd.common import DIR_X, VERT, move_data_loc
    dims = (nx, 12, 10)
    per = ("periodic",) * 2
    s, o, mesh = _solvers(dims, [(bc,) * 2, per, per], interpl, True, L=(6.283185307179586, 2.0, 3.0))
    arrays = _random_velocity(s, o, dims, nx)
    dense = _dense(mesh, 1, interpl, True)
    b, al = s.backend, s.backend.allocator
    _check_operators(s, o, 1, dense, arrays)
    for op in ("interpl_v2p", "der2nd"):
        t = getattr(s.xdirps, op)
        y1, y2, d1, d2 = (al.get_block(DIR_X, VERT) for _ in range(4))
        coefs = [0.3, -1.7, 0.01]
        b.lincomb(y1, s.u, coefs, [s.v, s.w, s.u])
        b.tds_apply(d1, y1, t, DIR_X)
        b.tds_lincomb(d2, t, DIR_X, y2, s.u, coefs, [s.v, s.w, s.u])
        for f in (d1, d2):
            f.set_data_loc(move_data_loc(VERT, 1, t.move))
        assert np.array_equal(b.get_field_data(y1), b.get_field_data(y2)), op
        assert np.array_equal(b.get_field_data(d1), b.get_field_data(d2)), op
        for f in (y1, y2, d1, d2):
            al.release_block(f)
    n3 = int(b.lib.x3d_backend_counter(b.h, 0))
    rhs_h = [al.get_block(DIR_X) for _ in range(3)]
    b.transeq_x(*rhs_h, s.u, s.v, s.w, s.nu, s.xdirps)
    fallback = any(os.environ.get(k) == "1" for k in ("X3D_XDIR_GENERIC", "X3D_NO_XSCAN", "X3D_XSCAN_P1", "X3D_NO_TILE3"))
    if bc == "periodic" and nx in (256, 512, 1024) and not fallback:  # the three-components-in-one kernels took it
        assert int(b.lib.x3d_backend_counter(b.h, 0)) == n3 + 1
    for f in rhs_h:
        al.release_block(f)
    _check_transeq(s, o, 1, dense, arrays)


YZ_PERIODIC = [(dims, interpl) for dims in ((32, 256, 8), (64, 8, 256), (32, 512, 8), (64, 8, 512))
               for interpl in ("optimised", "aggressive")]


@pytest.mark.parametrize("dims,interpl", YZ_PERIODIC)
def test_periodic_yz_kernels_with_wide_stencils(dims, interpl):
    """periodic y / z pencils of 256 / 512 rows: the single-pass on-chip and tile kernels (csrc/onchip.hip, the
    k_ytile_* forms) with NARROW = false -- every operator, transeq of the direction and the whole Solver.transeq, the
    operator pairs"""
    per = ("periodic",) * 2
    d = 2 if dims[1] >= 128 else 3
    s, o, mesh = _solvers(dims, [per] * 3, interpl, True)
    arrays = _random_velocity(s, o, dims, 11)
    dense = _dense(mesh, d, interpl, True)
    _check_operators(s, o, d, dense, arrays)
    _check_transeq(s, o, d, dense, arrays)
    _check_pairs(s, o, d, dense, arrays)


YZ_WALLS = [
    # 257..320 rows: 5 rows per lane (+ the DIRECT Thomas form); 321 and up: 6; one stretched grid per length
    ((32, 257, 8), "dirichlet", "uniform", "optimised"), ((64, 8, 257), "neumann", "uniform", "aggressive"),
    ((32, 257, 8), "dirichlet", "top-bottom", "aggressive"),
    ((32, 320, 8), "neumann", "uniform", "aggressive"), ((64, 8, 320), "dirichlet", "centred", "optimised"),
    ((64, 8, 321), "dirichlet", "uniform", "optimised"), ((32, 321, 8), "dirichlet", "bottom", "aggressive"),
    ((32, 384, 8), "dirichlet", "uniform", "aggressive"), ((64, 8, 384), "dirichlet", "centred", "optimised"),
    ((64, 8, 500), "neumann", "uniform", "optimised"), ((16, 500, 8), "dirichlet", "bottom", "aggressive"),
    ((32, 512, 8), "dirichlet", "uniform", "optimised"), ((64, 8, 512), "neumann", "uniform", "aggressive"),
    ((32, 512, 8), "dirichlet", "top-bottom", "optimised")]


@pytest.mark.parametrize("dims,bc,stretch,interpl", YZ_WALLS)
def test_wall_bounded_yz_kernels_with_wide_stencils(dims, bc, stretch, interpl):
    """non-periodic y / z pencils (csrc/ygen.hip: a hyperviscous der2nd with Dirichlet / Neumann ends is what takes
    k_ygen_transeq3<NARROW1 = true, NARROW = false>); uniform grids against the dense solve and the oracle, stretched
    ones against the oracle"""
    per = ("periodic",) * 2
    d = 2 if dims[1] >= 128 else 3
    bcs = [per, (bc,) * 2 if d == 2 else per, (bc,) * 2 if d == 3 else per]
    strs = ("uniform", stretch, "uniform") if d == 2 else ("uniform", "uniform", stretch)
    beta = [1.0, 1.0, 1.0]
    beta[d - 1] = 0.259065151 if stretch == "top-bottom" else 1.3
    s, o, mesh = _solvers(dims, bcs, interpl, True, strs=strs, beta=tuple(beta))
    arrays = _random_velocity(s, o, dims, 7)
    dense = _dense(mesh, d, interpl, True, uniform=stretch == "uniform")
    _check_operators(s, o, d, dense, arrays)
    _check_transeq(s, o, d, dense, arrays)
    _check_pairs(s, o, d, dense, arrays)


@pytest.mark.parametrize("interpl", ["optimised", "aggressive"])
def test_channel_x_kernel_with_wide_interpolation(interpl):
    """1024-row x pencils, the deferred velocity correction with the channel's rotation forcing in one launch
    (x3d_transeq_x_update_rot -> k_xwide_transeq3_upd): 'optimised' interpolation runs its N = false form;
    'aggressive' has no compressed lane tables, and the launch must decline (counter 1 unchanged, nothing done).  The
    served result against the unfused sequence (correction by tds_apply, transeq_x, forcing), the oracle and the dense
    solve."""
    from oracle import x3d_oracle as orc
    from x3d2_amd.common import DIR_X, VERT, move_data_loc
    dims = (1024, 12, 10)
    per = ("periodic",) * 2
    s, o, mesh = _solvers(dims, [per] * 3, interpl, False, L=(6.283185307179586, 2.0, 3.0))
    arrays = _random_velocity(s, o, dims, 21)
    b, al, x = s.backend, s.backend.allocator, s.xdirps
    rng = np.random.default_rng(22)
    garr = [rng.standard_normal((dims[2], dims[1], dims[0])) for _ in range(3)]
    g = [al.get_block(DIR_X, VERT) for _ in range(3)]
    for f, a in zip(g, garr):
        b.set_field_data(f, a)
        f.set_data_loc(move_data_loc(VERT, 1, 1))  # (the pressure gradient's staggered location along x)
    omega, scale = 0.37, -1.0
    # the unfused sequence, on copies
    vel = [al.get_block(DIR_X, VERT) for _ in range(3)]
    for f, src in zip(vel, (s.u, s.v, s.w)):
        b.veccopy(f, src)
    for f, gc, t in zip(vel, g, (x.stagder_p2v, x.interpl_p2v, x.interpl_p2v)):
        b.tds_apply(f, gc, t, DIR_X, accumulate=True, scale=scale)
    plain = [al.get_block(DIR_X) for _ in range(3)]
    b.transeq_x(*plain, *vel, s.nu, x)
    vel_plain = [b.get_field_data(f, VERT) for f in vel]
    rhs_plain = [b.get_field_data(f, VERT) for f in plain]
    rhs_plain[0] = rhs_plain[0] - omega * vel_plain[1]
    rhs_plain[1] = rhs_plain[1] + omega * vel_plain[0]
    # the oracle: the same sequence
    gvel = []
    for fo, a, op in zip((o.u, o.v, o.w), garr, ("stagder_p2v", "interpl_p2v", "interpl_p2v")):
        src = o.backend.get_block(orc.DIR_X, orc.VERT)
        o.backend.set_field_data(src, a)
        out = o.backend.get_block(orc.DIR_X)
        o.backend.tds_solve(out, src, getattr(o.xdirps, op))
        gvel.append(o.backend.get_field_data(fo, orc.VERT) + scale * o.backend.get_field_data(out, orc.VERT))
    for fo, a in zip((o.u, o.v, o.w), gvel):
        o.backend.set_field_data(fo, a)
    rhs_o = [o.backend.get_block(orc.DIR_X) for _ in range(3)]
    o.backend.transeq_x(*rhs_o, o.u, o.v, o.w, o.nu, o.xdirps)
    ref = [o.backend.get_field_data(f, orc.VERT) for f in rhs_o]
    ref[0] = ref[0] - omega * gvel[1]
    ref[1] = ref[1] + omega * gvel[0]
    dense = _dense(mesh, 1, interpl, False)
    dvel = [a + scale * dense_apply(dense[op], ga, 2) for a, ga, op in
            zip(arrays, garr, ("stagder_p2v", "interpl_p2v", "interpl_p2v"))]
    want = dense_transeq(dense, *dvel, s.nu, 2)
    want[0] = want[0] - omega * dvel[1]
    want[1] = want[1] + omega * dvel[0]
    for k in range(3):
        assert relerr(vel_plain[k], gvel[k]) < TOL and relerr(vel_plain[k], dvel[k]) < TOL, ("uvw"[k], "corrected")
        assert relerr(rhs_plain[k], ref[k]) < TOL and relerr(rhs_plain[k], want[k]) < TOL, ("uvw"[k], "unfused")
    # the one-launch form
    rhs = [al.get_block(DIR_X) for _ in range(3)]
    n_upd = int(b.lib.x3d_backend_counter(b.h, 1))
    served = b.transeq_x_update_rot(*rhs, s.u, s.v, s.w, s.nu, x, g, x.stagder_p2v, x.interpl_p2v, scale, omega)
    wide_off = any(os.environ.get(k) == "1" for k in ("X3D_NO_XWIDE", "X3D_NO_XSCAN", "X3D_XDIR_GENERIC", "X3D_NO_XWIDE_UPD"))
    assert served == (interpl == "optimised" and not wide_off)
    assert int(b.lib.x3d_backend_counter(b.h, 1)) == n_upd + int(served)
    if not served:  # nothing was done: u, v, w as they were
        for f, a in zip((s.u, s.v, s.w), arrays):
            assert np.array_equal(b.get_field_data(f, VERT), a)
        return
    for k, (f, r) in enumerate(zip((s.u, s.v, s.w), rhs)):
        u_got, r_got = b.get_field_data(f, VERT), b.get_field_data(r, VERT)
        assert relerr(u_got, vel_plain[k]) < TOL and relerr(u_got, dvel[k]) < TOL, ("uvw"[k], "corrected, fused")
        assert relerr(r_got, rhs_plain[k]) < TOL, ("uvw"[k], "fused vs unfused")
        assert relerr(r_got, ref[k]) < TOL and relerr(r_got, want[k]) < TOL, ("uvw"[k], "fused")


# ---------------------------------------------------------------- decomposed directions: the HALO single-pass kernels
@pytest.mark.parametrize("dims,nproc,interpl,hyper", [
    ((32, 16, 512), (1, 1, 2), "aggressive", False),    # 256 rows per rank: 207 + 207 strip rows > 256 (one range)
    ((32, 16, 1024), (1, 1, 2), "aggressive", False),   # 512 rows per rank: interior planes
    ((32, 1024, 16), (1, 2, 1), "optimised", True),     # y split, hyperviscous der2nd
    ((16, 512, 512), (1, 2, 2), "optimised", False)])   # y and z split
def test_decomposed_wide_stencils_vs_oracle_on_the_same_ranks(dims, nproc, interpl, hyper, tmp_path):
    """two (four) ranks sharing the GPU, fused driver: the single-pass HALO kernels and their boundary-strip
    corrections (k_tds_halo_fix / k_transeq_halo_fix) with strips of 103 ('optimised') or 207 ('aggressive') rows,
    against the oracle decomposed the same way (its distributed form is pinned to the dense solve in
    test_oracle_vs_reference.py): every operator of each split direction, transeq + species, divergence, gradient, curl,
    two RK3 steps"""
    from test_hip_parity import _run_fixture_worker
    from util import BATTERY_FIELDS, oracle_battery, stitch_ranks, synthetic_case
    nranks = int(np.prod(nproc))
    dn = "".join("xyz"[k] for k in range(3) if nproc[k] > 1)
    g = synthetic_case(dims, nproc, interpl=interpl, hyperviscous=hyper)
    path = str(tmp_path / "case.npz")
    np.savez(path, **g)
    parts = _run_fixture_worker([path, "fused"], tmp_path, 29531, nranks=nranks)
    offs = [p["offset"] for p in parts]
    assert all(int(p["halo_launches"][0]) >= len(dn) * 8 + 7 for p in parts)  # the single-pass path did run
    full, oparts = oracle_battery(g, nranks)
    for k in BATTERY_FIELDS(dn):
        assert relerr(stitch_ranks(parts, offs, k), full[k]) < TOL, k
    for p, o in zip(parts, oparts):
        assert relerr(p["species.rhs"], o["species.rhs"]) < TOL
        assert abs(p["curl.enstrophy"][0] - o["curl.enstrophy"][0]) <= 1e-12 * o["curl.enstrophy"][0]


# ---------------------------------------------------------------- FP32
def test_single_precision_wide_stencils_against_the_dense_solve():
    """libx3d2_hip_sp.so (tests/sp_worker.py, a process of its own): x 512 and 1024, y 512 periodic, z 257 Dirichlet,
    'optimised' interpolation and hyperviscous der2nd -- every operator and the direction's transeq against the FP64
    dense solve at FP32's tolerances (2e-5; 5e-4 where second derivatives amplify the inputs' rounding)"""
    from test_hip_single_prec import _worker
    res = _worker("wide", timeout=600)
    assert len(res) == 8, sorted(res)
    for case, worst in res.items():
        loose = {k: v for k, v in worst.items() if "der2nd" in k or k.startswith("transeq")}
        tight = {k: v for k, v in worst.items() if k not in loose}
        assert max(tight.values()) < 2e-5, (case, max(tight, key=tight.get), max(tight.values()))
        assert max(loose.values()) < 5e-4, (case, max(loose, key=loose.get), max(loose.values()))
