"""The RK stages inside the z launch of transeq carry the RUNNING SUM of the step's final combination instead of the stored
derivatives (TimeIntegrator.runge_kutta_fused / _runsum_stage, x3d_transeq_lincomb3_sum, k_ytile_transeq3<EPI>):

    u = ((base + b_1 dt d_1) + b_2 dt d_2) + b_3 dt d_3        evaluated left to right, one fused multiply-add per term,

so a partial sum e_s stored as a field and continued by the next stage gives the bits of the chain in one go.  Everything here
is bit for bit: the reference of every check is the same arithmetic through the calls that existed before (X3D_NO_RK_RUNSUM=1,
or x3d_transeq_acc followed by x3d_lincomb), never a tolerance.

Shapes: the z launch has one instantiation for 256-row and one for 512-row pencils (FP32: two pencils per wave, nx a multiple
of 32).  Whole steps run on 32 x 32 x 256 and 32 x 32 x 512 (64 tiles, one per workgroup); the launch by itself also on
48 x 88 x 256 = 264 tiles, eight more than the 256 workgroups of a launch, so that some workgroups walk a second tile with the
next tile's rows in flight across the store phase that was changed."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STEP_DIMS = [(32, 32, 256), (32, 32, 512)]


@contextlib.contextmanager
def switches(**env):
    """the driver's switches are read when the backend is made: set them around make_tgv, put the environment back after"""
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_steps(dims, time_intg, steps, **env):
    """`steps` fused TGV steps under the given switches: (u, v, w), the counters"""
    from x3d2_amd import make_tgv
    env.setdefault("X3D_NO_RK_RUNSUM", None)
    env.setdefault("X3D_EPI3_STAGES", None)
    env.setdefault("X3D_NO_EPI3", None)
    with switches(**env):
        case = make_tgv(dims, time_intg=time_intg, fused=True)
    for it in range(1, steps + 1):
        case.step(it, more=it < steps)
    s = case.solver
    b = s.backend
    fields = [b.get_field_data(f) for f in (s.u, s.v, s.w)]
    counts = {"in_transeq": getattr(s.time_integrator, "n_stage_in_transeq", 0), "nstage": s.time_integrator.nstage,
              "passes": getattr(b, "rk_in_tile3_passes", 0), "launches": getattr(b, "rk_in_tile3_launches", 0),
              "tq3": int(b.lib.x3d_backend_counter(b.h, 0))}
    return fields, counts


# ---------------------------------------------------------------- 1. whole steps
@pytest.mark.parametrize("time_intg", ["RK2", "RK3", "RK4"])
@pytest.mark.parametrize("dims", STEP_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_whole_steps_equal_the_stored_derivative_form_bit_for_bit(dims, time_intg):
    """two steps, the default against X3D_NO_RK_RUNSUM=1; every stage of both runs inside the z launch"""
    new, cn = run_steps(dims, time_intg, 2)
    old, co = run_steps(dims, time_intg, 2, X3D_NO_RK_RUNSUM="1")
    assert cn["in_transeq"] == 2 * cn["nstage"] and co["in_transeq"] == 2 * co["nstage"], (cn, co)
    for a, b in zip(new, old):
        assert np.isfinite(a).all() and np.array_equal(a, b)


# ---------------------------------------------------------------- 2. the launch by itself
def _solver(dims):
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.solver import Solver, SolverConfig
    per = ("periodic",) * 2
    mesh = Mesh(dims, (1, 1, 1), (6.283185307179586, 2.0, 3.0), per, per, per)
    return Solver(HipBackend(mesh), mesh, SolverConfig(poisson_solver_type="CG", fused=True))


class _Blocks:
    """device blocks filled with seeded random numbers (the padding too: both sides of a comparison start from the same
    bits); `like(f)` is a second block with f's contents"""

    def __init__(self, s, seed):
        import torch
        from x3d2_amd.common import DIR_X, VERT
        self.s, self.dir, self.loc = s, DIR_X, VERT
        self.gen = torch.Generator(device=s.u.data.device)
        self.gen.manual_seed(seed)
        self.torch = torch

    def new(self):
        f = self.s.backend.allocator.get_block(self.dir, self.loc)
        f.data.copy_(self.torch.randn(f.data.shape, generator=self.gen, device=f.data.device, dtype=f.data.dtype))
        return f

    def like(self, f):
        g = self.s.backend.allocator.get_block(self.dir, self.loc)
        g.data.copy_(f.data)
        return g


def _same(b, f, g):
    from x3d2_amd.common import VERT
    return np.array_equal(b.get_field_data(f, VERT), b.get_field_data(g, VERT))


# per variable: the stage's coefficient a dt, the running sum's b dt -- all different, so that a swapped variable shows
A_DT = (0.37e-3, 0.53e-3, 0.71e-3)
B_DT = (0.29e-3, 0.43e-3, 0.61e-3)


@pytest.mark.parametrize("alias", ["sbase_is_base", "in_place", "no_second_output"])
@pytest.mark.parametrize("store", [0, 1])
@pytest.mark.parametrize("dims", [(48, 88, 256), (32, 16, 512)], ids=lambda d: "x".join(map(str, d)))
def test_the_launch_equals_transeq_acc_then_lincomb_twice(dims, store, alias):
    """x3d_transeq_lincomb3_sum on random fields against x3d_transeq_acc, x3d_lincomb for y, x3d_lincomb for e: u, v and w
    each, in the three forms the driver uses -- stage 1 (sbase == base == the velocity the launch reads), a middle stage
    (e in place, y the velocity itself), the last stage (no second output: the parent's entry point).  store = 0 leaves
    the derivative blocks as they were, store = 1 holds the complete derivative"""
    from x3d2_amd.common import DIR_Z
    s = _solver(dims)
    b = s.backend
    assert b.transeq_stage_ok(DIR_Z, s.zdirps)
    bl = _Blocks(s, 20 + store)
    vel = [bl.new() for _ in range(3)]
    rhs = [bl.new() for _ in range(3)]
    rhs_in = [bl.like(f) for f in rhs]
    # the reference: the accumulating launch on copies, then the plain combinations
    d = [bl.like(f) for f in rhs]
    b.transeq_dir(DIR_Z, d[0], d[1], d[2], vel[0], vel[1], vel[2], s.nu, s.zdirps, accumulate=True)
    if alias == "sbase_is_base":
        base, y, e = vel, [bl.new() for _ in range(3)], [bl.new() for _ in range(3)]
        sbase = base
    else:
        base, y, e = [bl.new() for _ in range(3)], vel, [bl.new() for _ in range(3)]  # (y_i IS the velocity it updates)
        sbase = e
    y_ref, e_ref = [bl.new() for _ in range(3)], [bl.new() for _ in range(3)]
    for i in range(3):
        b.lincomb(y_ref[i], base[i], [A_DT[i]], [d[i]])
        b.lincomb(e_ref[i], sbase[i], [B_DT[i]], [d[i]])
    specs = [(y[i], base[i], [A_DT[i]], [rhs[i]], bool(store)) for i in range(3)]
    sums = None if alias == "no_second_output" else [(e[i], sbase[i], B_DT[i]) for i in range(3)]
    e_in = [bl.like(f) for f in e]
    assert b.transeq_lincomb3(DIR_Z, rhs, vel, s.nu, s.zdirps, specs, sums), "the z launch declined"
    for i, name in enumerate("uvw"):
        assert _same(b, y[i], y_ref[i]), ("y", name)
        if sums is None:
            assert bool((e[i].data == e_in[i].data).all()), ("e untouched", name)
        else:
            assert _same(b, e[i], e_ref[i]), ("e", name)
        if store:
            assert _same(b, rhs[i], d[i]), ("stored derivative", name)
        else:
            assert bool((rhs[i].data == rhs_in[i].data).all()), ("derivative block untouched", name)
    # (the outputs differ from one variable to the next: equal results would not tell a swapped variable)
    assert not _same(b, y[0], y[1]) and not _same(b, y[1], y[2])


# ---------------------------------------------------------------- 3. mixed steps
@pytest.mark.parametrize("stages,which", [("1,3", "middle"), ("1,2", "last")])
def test_a_stage_outside_the_z_launch_continues_from_the_running_sum(stages, which):
    """X3D_EPI3_STAGES without the middle / the last stage: that stage of a running-sum step runs as the plain accumulating
    launch, lincomb for y and lincomb for e (or for u from e) -- two RK3 steps equal the default's bits"""
    dims = STEP_DIMS[0]
    ref, cr = run_steps(dims, "RK3", 2)
    got, cg = run_steps(dims, "RK3", 2, X3D_EPI3_STAGES=stages)
    assert cr["in_transeq"] == 6 and cr["launches"] == 6, cr
    assert cg["in_transeq"] == 4 and cg["launches"] == 4, cg  # two of the three stages of each step inside the z launch
    # passes of the launches that ran (the counter's convention, test 5): stage 1 = 6, stage 2 = 9, stage 3 = 6
    assert cg["passes"] == 2 * (6 + (6 if which == "middle" else 9)), cg
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 4. argument checks
@pytest.mark.parametrize("clash", ["velocity", "y", "derivative", "base", "other_sum"])
def test_a_running_sum_that_aliases_something_else_is_refused(clash):
    from x3d2_amd.common import DIR_Z, X3dError
    s = _solver((32, 16, 256))
    b = s.backend
    bl = _Blocks(s, 4)
    vel, rhs, y, e = ([bl.new() for _ in range(3)] for _ in range(4))
    bad = {"velocity": vel[2], "y": y[1], "derivative": rhs[0], "base": vel[0], "other_sum": e[1]}[clash]
    specs = [(y[i], vel[i], [A_DT[i]], [rhs[i]], False) for i in range(3)]
    sums = [(bad if i == 0 else e[i], vel[i], B_DT[i]) for i in range(3)]
    keep = [bl.like(f) for f in vel + rhs + y + e]
    n0 = int(b.lib.x3d_backend_counter(b.h, 0))
    with pytest.raises(X3dError, match="aliases"):
        b.transeq_lincomb3(DIR_Z, rhs, vel, s.nu, s.zdirps, specs, sums)
    assert int(b.lib.x3d_backend_counter(b.h, 0)) == n0  # nothing was launched ...
    for f, g in zip(vel + rhs + y + e, keep):
        assert bool((f.data == g.data).all())            # ... and nothing written
    # the same call with its own block for the sum goes through
    sums[0] = (e[0], vel[0], B_DT[0])
    assert b.transeq_lincomb3(DIR_Z, rhs, vel, s.nu, s.zdirps, specs, sums)


# ---------------------------------------------------------------- 5. work counts
def test_an_rk3_step_moves_three_fields_fewer():
    """rk_in_tile3_passes counts the fields a stage reads or writes on top of the launch's own 64 B/DoF, which hold the
    store of d.  Stored derivatives: (y, base) in stages 1 and 2, (u, base, d1, d2) in stage 3 = 6 + 6 + 12.  Running sum,
    whose write stands where d's was: (y, base) ; (y, base, + R e) ; (u, e) = 6 + 9 + 6 -- in whole passes of the three
    launches 12 + 18 + 12 against 12 + 15 + 18.  Same launches"""
    _, new = run_steps(STEP_DIMS[0], "RK3", 1)
    _, old = run_steps(STEP_DIMS[0], "RK3", 1, X3D_NO_RK_RUNSUM="1")
    assert (old["passes"], new["passes"]) == (24, 21), (old, new)
    assert new["launches"] == old["launches"] == 3 and new["tq3"] == old["tq3"], (old, new)
    assert new["in_transeq"] == old["in_transeq"] == 3


# ---------------------------------------------------------------- 6. the FP32 flavour
def test_whole_steps_in_the_fp32_flavour():
    """libx3d2_hip_sp.so in a process of its own (the real kind is chosen at import): test 1's RK3 and RK4 runs on both
    pencil lengths, two pencils per wave -- bit for bit on 4-byte reals too"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "rk_runsum_sp_worker.py")], capture_output=True, text=True,
                       env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = json.loads([l for l in r.stdout.splitlines() if l.startswith("RUNSUMRESULT ")][-1][13:])
    assert len(rows) == 4
    for row in rows:
        assert row["dtype"] == "float32" and row["finite"], row
        assert row["in_transeq_new"] == row["in_transeq_old"] == 2 * row["nstage"], row
        assert row["equal"] == [True, True, True], row
