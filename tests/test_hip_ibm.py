"""Immersed boundary and the cylinder case on the device (csrc/ibm.hip, x3d2_amd/ibm.py, CylinderCase).

1. the sparse body kernel against three vecmult calls, bit for bit, and nothing written outside the valid points
2. the outflow parameters against numpy on the same field
3. the one-launch face stamp against three field_set_face_from_field(X_FACE) calls
4. the inlet plane against a numpy restatement of the generator
5. full steps against the reference's step composed from the oracle's pieces (tests/cylinder_ref.py)
6. the sparse path against X3D_NO_IBM_SPARSE=1
7. an Ibm on the channel and the TGV case
8. the FP32 flavour (tests/ibm_sp_worker.py)"""
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import cylinder_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PER, DIR = ("periodic", "periodic"), ("dirichlet", "dirichlet")
L = (20.0, 12.0, 6.0)
# (dims, x BC): a row shorter than one segment; a last segment with ONE valid point; three segments, odd ny and nz;
# periodic, whole segments only (the library pads a row by 16 reals from 256 points on: at 128 the pitch IS nx, the
# other pitches here are 48, 80 and 144); periodic with whole segments AND the default padding (pitch 272)
SHAPES = [((33, 16, 8), DIR), ((65, 12, 6), DIR), ((130, 9, 5), DIR), ((128, 16, 8), PER), ((256, 8, 4), PER)]
MASKS = ["cylinder", "cross64", "ends", "ones", "zeros", "fractional"]


# ---------------------------------------------------------------- helpers (also used by tests/ibm_sp_worker.py)
def make_backend(dims, xbc=DIR, lazy=False):
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    mesh = Mesh(tuple(dims), (1, 1, 1), L, xbc, PER, PER)
    return HipBackend(mesh, lazy=lazy)


def np_real():
    from x3d2_amd import _lib
    return np.dtype(_lib.NP_REAL)


def make_mask(kind, mesh, seed=3):
    from x3d2_amd.ibm import cylinder_mask
    nx, ny, nz = (int(n) for n in mesh.vert_dims)
    ep1 = np.ones((nz, ny, nx))
    if kind == "cylinder":
        ep1 = cylinder_mask(mesh, (0.4 * L[0], 0.5 * L[1]), 0.2 * L[1])
    elif kind == "cross64":  # a body across the boundary between the first two segments (or up to the row's end)
        ep1[1:nz - 1, 2:ny - 2, 57:min(nx, 71)] = 0.0
        if nx <= 64:
            ep1[1:nz - 1, 2:ny - 2, nx - 7:] = 0.0
    elif kind == "ends":  # touches i = 1 and i = nx
        ep1[:, 1:ny:2, 0] = 0.0
        ep1[:, 1:ny:3, nx - 1] = 0.0
    elif kind == "zeros":
        ep1[...] = 0.0
    elif kind == "fractional":
        rng = np.random.default_rng(seed)
        pick = rng.random(ep1.shape) < 0.3
        ep1[pick] = rng.uniform(0.01, 0.99, size=int(pick.sum())).astype(np.float32)  # (exact in both flavours)
    elif kind != "ones":
        raise ValueError(kind)
    return ep1


def numpy_counts(ep1):
    nz, ny, nx = ep1.shape
    hit = np.zeros((nz, ny, (nx + 63) // 64 * 64), dtype=bool)
    hit[:, :, :nx] = ep1 != 1
    return int(hit.reshape(nz, ny, -1, 64).any(axis=3).sum()), int(hit.sum())


def random_blocks(b, seed, count=3):
    """blocks whose WHOLE extent, padding included, holds seeded standard_normal values"""
    import torch
    from x3d2_amd.common import DIR_X, VERT
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        f = b.allocator.get_block(DIR_X, VERT)
        a = rng.standard_normal(b.nblock, dtype=np.float32).astype(np_real())
        f.data.copy_(torch.from_numpy(a))
        out.append(f)
    return out


def whole(b, f):
    """the padded block as [nzp, nyp, nxp]"""
    nxp, nyp, nzp = b.padded_dims
    return f.data.cpu().numpy().reshape(nzp, nyp, nxp).copy()


def clone(b, fields):
    from x3d2_amd.common import DIR_X, VERT
    out = []
    for f in fields:
        g = b.allocator.get_block(DIR_X, VERT)
        g.data.copy_(f.data)
        out.append(g)
    return out


def body_case(dims, xbc, kind):
    """(n_segments, n_masked, numpy counts, valid points equal to three vecmult, nothing else written, fields changed,
    row pitch)"""
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.ibm import Ibm
    b = make_backend(dims, xbc)
    nx, ny, nz = dims
    ep1 = make_mask(kind, b.mesh)
    ibm = Ibm(SimpleNamespace(backend=b), ep1)
    assert ibm.h is not None and ibm.ep1_field is None
    uvw = random_blocks(b, 11)
    ref = clone(b, uvw)
    before = [whole(b, f) for f in uvw]
    ibm.body(*uvw)
    mask = b.allocator.get_block(DIR_X, VERT)  # the reference's form: a block of ones with ep1 on the vertices
    mask.fill(1.0)
    b.set_field_data(mask, ep1)
    for f in ref:
        b.vecmult(f, mask)
    valid_equal = outside_untouched = True
    for f, g, a0 in zip(uvw, ref, before):
        got, want = whole(b, f), whole(b, g)
        valid_equal &= np.array_equal(got[:nz, :ny, :nx], want[:nz, :ny, :nx])
        keep = np.ones(got.shape, dtype=bool)
        keep[:nz, :ny, :nx] = False
        outside_untouched &= np.array_equal(got[keep], a0[keep])
        if kind == "ones":
            outside_untouched &= np.array_equal(got, a0)
    changed = any(not np.array_equal(whole(b, f), a0) for f, a0 in zip(uvw, before))
    return ibm.n_segments, ibm.n_masked, numpy_counts(ep1.astype(np_real())), bool(valid_equal), bool(outside_untouched), changed, int(b.padded_dims[0])


# ---------------------------------------------------------------- 1. body kernel
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("dims,xbc", SHAPES)
def test_body_equals_three_vecmult_and_writes_nothing_else(dims, xbc, kind):
    nseg, nmask, counts, valid_equal, outside_untouched, changed, nxp = body_case(dims, xbc, kind)
    if os.environ.get("X3D_PAD_X") is None:
        assert nxp == {33: 48, 65: 80, 130: 144, 128: 128, 256: 272}[dims[0]]
    assert (nseg, nmask) == counts
    assert valid_equal and outside_untouched
    if kind == "ones":
        assert nseg == 0 and nmask == 0 and not changed
    else:
        assert nseg > 0 and changed
    if kind == "zeros":
        assert nmask == dims[0] * dims[1] * dims[2] and nseg == (dims[0] + 63) // 64 * dims[1] * dims[2]


def test_body_rejects_what_it_cannot_do_and_iibm_0_does_nothing():
    from x3d2_amd.common import X3dError
    from x3d2_amd.ibm import Ibm
    b = make_backend((33, 16, 8))
    s = SimpleNamespace(backend=b)
    with pytest.raises(X3dError):
        Ibm(s, np.ones((8, 16, 32)))
    ibm = Ibm(s, make_mask("cylinder", b.mesh))
    u, v, w = random_blocks(b, 5)
    with pytest.raises(X3dError):
        ibm.body(u, u, w)  # one block twice
    off = Ibm(s, make_mask("zeros", b.mesh), iibm=0)
    before = [whole(b, f) for f in (u, v, w)]
    off.body(u, v, w)
    assert off.n_segments == 0 and all(np.array_equal(whole(b, f), a) for f, a in zip((u, v, w), before))


def test_body_behind_queued_calls_equals_the_eager_result():
    """deferred execution: the body runs at once on the buffers that hold its handles' data, after what was recorded"""
    from x3d2_amd.ibm import Ibm
    dims, out = (65, 12, 6), {}
    for lazy in (False, True):
        b = make_backend(dims, lazy=lazy)
        ibm = Ibm(SimpleNamespace(backend=b), make_mask("fractional", b.mesh))
        rng = np.random.default_rng(2)
        from x3d2_amd.common import DIR_X, VERT
        u, v, w = (b.allocator.get_block(DIR_X, VERT) for _ in range(3))
        for f in (u, v, w):
            f.fill(0.0)
            b.set_field_data(f, rng.standard_normal((6, 12, 65), dtype=np.float32).astype(np.float64))
        b.vecadd(0.5, v, 1.0, u)  # recorded, not run, while the deferred layer is on
        b.field_scale(w, 1.25)
        ibm.body(u, v, w)
        b.vecadd(1.0, u, 1.0, v)
        out[lazy] = [b.get_field_data(f) for f in (u, v, w)]
    for a, c in zip(out[True], out[False]):
        assert np.array_equal(a, c) and float(np.max(np.abs(c))) > 0.0


# ---------------------------------------------------------------- 2. outflow parameters
@pytest.mark.parametrize("dims", [(33, 16, 8), (130, 9, 5)])
def test_outflow_params_against_numpy(dims):
    b = make_backend(dims)
    nx, ny, nz = dims
    (u,) = random_blocks(b, 21, count=1)
    a = b.get_field_data(u).astype(np.float64)
    gdt, dx = 0.0075 * 4.0 / 9.0, float(b.mesh.d[0])
    got = []
    for _ in range(2):
        b.outflow_params(u, gdt, dx)
        got.append(b.outflow_params_get())
    assert got[0] == got[1]  # deterministic: bitwise the same twice
    out_vel, frd = got[0]
    rt = np_real().type
    assert out_vel == float(rt(rt(a[:, :, nx - 2].max()) * rt(gdt)) / rt(dx))  # the maximum is order-independent: exact
    want = (math.fsum(a[:, :, 0].ravel()) - math.fsum(a[:, :, nx - 1].ravel())) / (ny * nz)
    eps = float(np.finfo(np_real()).eps)
    bound = 2 * ny * nz * eps * float(np.max(np.abs(a))) / (ny * nz)
    print("outflow_params", dims, "flow_rate_diff err", abs(frd - want), "bound", bound)
    assert abs(frd - want) <= bound
    assert abs(want) > 100 * bound  # (the check means something: the two plane sums do not cancel)


# ---------------------------------------------------------------- 3. faces
@pytest.mark.parametrize("dims", [(33, 16, 8), (130, 9, 5)])
def test_cylinder_apply_bc_equals_three_set_face_calls(dims):
    from x3d2_amd.common import X_FACE
    b = make_backend(dims)
    uvw = random_blocks(b, 31)
    inlet = random_blocks(b, 32)
    ref = clone(b, uvw)
    before = whole(b, uvw[1])
    params = b.outflow_params(uvw[0], 0.0075, float(b.mesh.d[0]))
    out_vel, frd = b.outflow_params_get()
    assert out_vel != 0.0 and frd != 0.0
    b.cylinder_apply_bc(*uvw, *inlet, params)
    for f, st in zip(ref, inlet):
        b.field_set_face_from_field(f, st, out_vel, X_FACE, flow_rate_diff=frd)
    for f, g in zip(uvw, ref):
        assert np.array_equal(whole(b, f), whole(b, g))
    assert not np.array_equal(whole(b, uvw[1]), before)  # (something was stamped)


# ---------------------------------------------------------------- 4. inlet plane
M64 = (1 << 64) - 1


def mix64(z):
    """x3d_mix64 (splitmix64) on uint64 arrays"""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def inlet_plane(ny, nz, base, amp, seed, draw):
    key = mix64(np.array([(seed + draw) & M64], dtype=np.uint64))
    with np.errstate(over="ignore"):
        z = mix64(key + np.arange(ny * nz, dtype=np.uint64))  # index k * ny + j
    r = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return (base + amp * (2.0 * r - 1.0)).reshape(nz, ny)


@pytest.mark.parametrize("dims", [(33, 16, 8), (130, 9, 5)])
def test_inlet_noise_against_the_numpy_generator(dims):
    b = make_backend(dims)
    nx, ny, nz = dims
    (f,) = random_blocks(b, 41, count=1)
    before = whole(b, f)
    base, amp, seed = 1.0, 0.125 * math.exp(-0.2 * 10.0 * 10.0) * 1e8, 2 ** 63 + 12345
    b.inlet_noise(f, base, amp, seed, 4)
    got = whole(b, f)
    want = inlet_plane(ny, nz, base, amp, seed, 4)
    plane = got[:nz, :ny, 0]
    assert np.max(np.abs(plane - want) / np.abs(want)) <= 1e-15
    # inside [base - amp, base + amp): r < 1 (the upper edge could only be reached by r = 1 - 2^-53 after rounding)
    assert np.all(plane >= base - amp) and np.all(plane < base + amp) and np.ptp(plane) > amp
    keep = np.ones(got.shape, dtype=bool)
    keep[:nz, :ny, 0] = False
    assert np.array_equal(got[keep], before[keep])  # the rest of the block is unchanged
    b.inlet_noise(f, base, amp, seed, 4)
    assert np.array_equal(whole(b, f), got)  # the same (seed, draw) repeats
    b.inlet_noise(f, base, amp, seed, 5)
    other = whole(b, f)[:nz, :ny, 0]
    assert not np.array_equal(other, plane)
    assert np.max(np.abs(other - inlet_plane(ny, nz, base, amp, seed, 5)) / np.abs(other)) <= 1e-15
    b.inlet_noise(f, 0.0, 0.0, seed, 6)  # no noise on a component: its base value
    assert np.all(whole(b, f)[:nz, :ny, 0] == 0.0)


# ---------------------------------------------------------------- 5. full steps
CASES = {"AB3": (33, 16, 8), "RK3": (65, 32, 8)}
BODY = dict(centre=(5.0, 6.0), radius=1.3)  # (the default body, diameter 1, holds a single vertex per plane at these sizes)


def cylinder_pair(time_intg, fused, with_ref=True, **kw):
    from x3d2_amd import make_cylinder
    from x3d2_amd.ibm import cylinder_mask
    dims = CASES[time_intg]
    case = make_cylinder(dims, L, time_intg=time_intg, fused=fused, **BODY, **kw)
    s = case.solver
    ep1 = cylinder_mask(s.mesh, BODY["centre"], BODY["radius"])
    assert np.array_equal(ep1, s.ibm.ep1) and s.ibm.n_masked == int((ep1 == 0).sum()) > 8
    pert = cylinder_ref.smooth_perturbation(s.mesh)
    init = (1.0 + pert[0], pert[1], pert[2])
    for f, a in zip((s.u, s.v, s.w), init):
        s.backend.set_field_data(f, a)
    ref = None
    if with_ref:
        ref = cylinder_ref.CylinderRef(dims, L, time_intg=time_intg, ep1=ep1)
        ref.set_velocity(*init)
    return case, ref, ep1


def fields_of(case):
    s = case.solver
    return [s.backend.get_field_data(f) for f in (s.u, s.v, s.w)]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("time_intg", ["AB3", "RK3"])
def test_cylinder_steps_against_the_composed_reference(time_intg, fused):
    case, ref, ep1 = cylinder_pair(time_intg, fused)
    s = case.solver
    dx, dt = float(s.mesh.d[0]), s.dt
    for it in range(1, 4):
        case.step(it)
        ref.step()
        got = fields_of(case)
        scale = max(max(float(np.max(np.abs(r))) for r in ref.velocity()), 1.0)
        out_vel, frd = s.backend.outflow_params_get()
        # the parameters are plane functionals of u with weights gdt / dx (a maximum) and 1 / (ny nz) (two means): fields
        # that agree to 1e-10 * scale give parameters that agree to gdt / dx and 2 times that
        print("cylinder", time_intg, fused, it, "out_vel", out_vel, ref.out_vel, "flow_rate_diff", frd, ref.flow_rate_diff)
        assert abs(out_vel - ref.out_vel) <= 1e-10 * scale * dt / dx
        assert abs(frd - ref.flow_rate_diff) <= 2e-10 * scale
        assert ref.out_vel > 0.0 if (it > 1 or time_intg == "RK3") else ref.out_vel == 0.0
    for nm, a, r in zip("uvw", got, ref.velocity()):
        err, bound = float(np.max(np.abs(a - r))), 1e-10 * max(float(np.max(np.abs(r))), 1.0)
        print("cylinder", time_intg, fused, nm, "err", err, "bound", bound)
        assert err < bound, nm
    row = case.postprocess(3, 3 * dt)
    eo = ref.monitor()
    assert abs(row[1] - eo[0]) < 1e-10 * abs(eo[0])
    assert case.outflow_rows[-1][1:] == (case.out_vel, case.flow_rate_diff) == s.backend.outflow_params_get()
    # the velocity is exactly zero inside the body once ibm%body has run
    s.ibm.body(s.u, s.v, s.w)
    for a in fields_of(case):
        assert np.all(a[ep1 == 0] == 0.0) and np.any(a[ep1 == 1] != 0.0)


def test_inlet_noise_case_repeats_for_a_seed_and_differs_for_another():
    runs = []
    for seed in (5, 5, 6):
        case, _, _ = cylinder_pair("AB3", True, with_ref=False, inlet_noise=(0.1, 0.05, 0.05), seed=seed)
        for it in range(1, 3):
            case.step(it)
        runs.append(fields_of(case))
    assert all(np.array_equal(a, c) for a, c in zip(runs[0], runs[1]))
    assert not np.array_equal(runs[0][0], runs[2][0])
    assert all(np.all(np.isfinite(a)) for a in runs[2])


# ---------------------------------------------------------------- 6. sparse against the reference's three vecmult calls
def test_sparse_body_equals_the_dense_path_over_three_steps(monkeypatch):
    out = {}
    for dense in (False, True):
        if dense:
            monkeypatch.setenv("X3D_NO_IBM_SPARSE", "1")
        case, _, _ = cylinder_pair("AB3", False, with_ref=False)
        assert case.solver.ibm.sparse == (not dense) and (case.solver.ibm.ep1_field is not None) == dense
        for it in range(1, 4):
            case.step(it)
        out[dense] = fields_of(case)
    for a, c in zip(out[False], out[True]):
        assert np.array_equal(a, c)


# ---------------------------------------------------------------- 7. other cases
def _other_case(kind, fused):
    from x3d2_amd import make_channel, make_tgv
    from x3d2_amd.ibm import cylinder_mask
    if kind == "channel":
        case = make_channel((24, 33, 16), fused=fused)
        m = case.solver.mesh
        ep1 = np.ones((16, 33, 24))
        ep1[4:12, :6, 8:14] = 0.0  # a block on the lower wall
    else:
        case = make_tgv(32, fused=fused)
        m = case.solver.mesh
        ep1 = cylinder_mask(m, (math.pi, math.pi, math.pi), 0.9, axis=None)  # a sphere
    assert 0 < int((ep1 == 0).sum()) < ep1.size // 4
    return case, ep1


@pytest.mark.parametrize("kind,fused", [("channel", True), ("tgv", False), ("tgv", True)])
def test_ibm_on_the_other_cases(kind, fused, monkeypatch):
    from x3d2_amd.ibm import Ibm
    out = {}
    for mode in ("none", "sparse", "dense"):
        if mode == "dense":
            monkeypatch.setenv("X3D_NO_IBM_SPARSE", "1")
        case, ep1 = _other_case(kind, fused)
        if mode != "none":
            case.solver.ibm = Ibm(case.solver, ep1)
            assert case.solver.ibm.sparse == (mode == "sparse")
        for it in range(1, 3):
            case.step(it)
        out[mode] = fields_of(case)
    for a, c, n in zip(out["sparse"], out["dense"], out["none"]):
        assert np.all(np.isfinite(a)) and np.array_equal(a, c)
    assert not np.array_equal(out["sparse"][0], out["none"][0])


def test_fused_driver_with_an_ibm_equals_the_op_granular_order():
    """TGV 32^3, RK3, a sphere: the fused driver defers the velocity correction to the next transeq_x kernel while the mask
    is attached; the op-granular driver issues the reference's order call for call.  The bound the suite puts on fused
    against op-granular full steps (test_fused_full_step_matches_op_granular_and_survey_trace): 1e-12 relative."""
    from x3d2_amd.ibm import Ibm
    out = {}
    for fused in (False, True):
        case, ep1 = _other_case("tgv", fused)
        case.solver.ibm = Ibm(case.solver, ep1)
        for it in range(1, 4):
            case.step(it, more=(it < 3))
        case.solver.flush_grad()
        out[fused] = fields_of(case)
    for nm, a, c in zip("uvw", out[True], out[False]):
        err = float(np.max(np.abs(a - c)) / np.max(np.abs(c)))
        print("ibm fused vs op-granular", nm, err)
        assert err < 1e-12, nm


def test_mask_file_round_trip_through_an_ibm(tmp_path):
    from x3d2_amd.ibm import Ibm
    b = make_backend((33, 16, 8))
    s = SimpleNamespace(backend=b)
    ibm = Ibm(s, make_mask("fractional", b.mesh))
    path = str(tmp_path / "ibm_100.npz")
    ibm.save(path)
    back = Ibm.from_file(s, path)
    assert back.iibm == 1 and np.array_equal(back.ep1, ibm.ep1)
    assert (back.n_segments, back.n_masked) == (ibm.n_segments, ibm.n_masked) == numpy_counts(ibm.ep1)


# ---------------------------------------------------------------- 8. FP32
def _worker(script, *args, timeout=600, env=None):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(HERE, script)] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("IBMRESULT ")][-1][10:])


# one AB3 step of case 5 at 33 x 16 x 8, FP32 against FP64, max |difference| over u, v, w: measured 8.23e-07 on an MI355X
# (about 7 FP32 eps on fields of O(1), through the compact solves and the Poisson solve); asserted at 10 times that
FP32_MEASURED = 8.23e-07


def test_fp32_flavour(tmp_path):
    """the body kernel on 4-byte reals, bit for bit, and one step of the cylinder against the FP64 run of the same case"""
    path = str(tmp_path / "sp_step.npz")
    res = _worker("ibm_sp_worker.py", path, env={"X3D_SINGLE_PREC": "1"})
    assert res["dtype"] == "float32" and len(res["body"]) == len(MASKS)
    for kind, (nseg, nmask, counts, valid_equal, outside_untouched, changed, _) in res["body"].items():
        assert [nseg, nmask] == counts and valid_equal and outside_untouched, kind
        assert changed == (kind != "ones"), kind
    case, _, _ = cylinder_pair("AB3", False, with_ref=False)
    case.step(1)
    sp = np.load(path)
    err = max(float(np.max(np.abs(sp[nm].astype(np.float64) - a))) for nm, a in zip("uvw", fields_of(case)))
    print("fp32 cylinder step: max |FP32 - FP64| =", err)
    assert 0.0 < err <= 10 * FP32_MEASURED
