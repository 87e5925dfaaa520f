"""Loads and probes on the device (csrc/ibm.hip: x3d_ibm_body_loads; csrc/probe.hip; x3d2_amd/loads.py, x3d2_amd/probes.py)
against the numpy restatement (tests/loads_ref.py), on the shapes and masks of tests/test_hip_ibm.py.

The bound on a load row, |row_c - ref_c| <= 1e-13 sum|terms_c|, is derived, not tuned: a term carries three product roundings
(1 - ep1 is exact for the masks here or one more), a fixed-tree sum of n <= 2^20 terms adds at most about (log2 n + 3)
roundings per term, together below 30 * 2^-53 = 3.3e-15 of sum|terms|; the bound leaves a factor of about 30.  It is the same
in FP32, where every factor is widened to double before any product.

 1. field bits and rows for every shape and mask        2. accumulate        3. a uniform flow        4. determinism, lazy
 5. the cylinder case, step by step                     6. probes            7. the series            8. restart
 9. two ranks (tests/mp_loads_worker.py)               10. FP32 (tests/loads_sp_worker.py)            11. errors"""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import loads_ref as ref
import test_hip_ibm as tib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 1e-13
PER, WALL = tib.PER, tib.DIR
DP = ctypes.POINTER(ctypes.c_double)


# ---------------------------------------------------------------- helpers (also used by the two workers)
def set_weights(b, ibm, w):
    from x3d2_amd import _lib
    w = [np.ascontiguousarray(a, dtype=np.float64) for a in w]
    _lib.check(b.lib.x3d_ibm_set_weights(ibm.h, *[a.ctypes.data_as(DP) for a in w]))


def new_row(b, fill=0.0):
    import torch
    return torch.full((4,), fill, dtype=torch.float64, device=b.device)


def raw_of(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def interior(b, f):
    nx, ny, nz = (int(n) for n in b.mesh.vert_dims)
    return tib.whole(b, f)[:nz, :ny, :nx]


def check_rows(rows):
    """rows: (name, |err|, bound); every figure is printed before the first assertion"""
    for name, err, bound in rows:
        print("loads %-28s err %.3e  bound %.3e" % (name, err, bound))
    for name, err, bound in rows:
        assert err <= bound, name


def stretched_backend(dims, lazy=False):
    """Dirichlet x, y stretched towards its walls, periodic z"""
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    mesh = Mesh(tuple(dims), (1, 1, 1), tib.L, WALL, WALL, PER, ("uniform", "top-bottom", "uniform"), (1.0, 2.0, 1.0))
    return HipBackend(mesh, lazy=lazy)


def body_loads_case(dims, xbc, kind):
    """x3d_ibm_body_loads next to x3d_ibm_body on the same seeded blocks: a dict of plain values (it crosses a process
    boundary in the FP32 test)"""
    from x3d2_amd.ibm import Ibm
    b = tib.make_backend(dims, xbc)
    ep1 = tib.make_mask(kind, b.mesh)
    ibm = Ibm(SimpleNamespace(backend=b), ep1)
    w = ref.weights(b.mesh)
    set_weights(b, ibm, w)
    uvw = tib.random_blocks(b, 11)
    twin = tib.clone(b, uvw)
    before = [tib.whole(b, f) for f in uvw]
    row = new_row(b, 7.0)
    b.ibm_body_loads(ibm.h, *uvw, row.data_ptr(), 0)
    got = raw_of(row)
    ibm.body(*twin)  # (no Loads attached: x3d_ibm_body)
    nx, ny, nz = dims
    same_bits = outside_untouched = True
    for f, g, a0 in zip(uvw, twin, before):
        after = tib.whole(b, f)
        same_bits &= after.tobytes() == tib.whole(b, g).tobytes()  # the whole padded block
        keep = np.ones(after.shape, dtype=bool)
        keep[:nz, :ny, :nx] = False
        outside_untouched &= np.array_equal(after[keep], a0[keep])
    m = ep1.astype(tib.np_real())
    fields = [a0[:nz, :ny, :nx] for a0 in before]
    want, mag = ref.impulse(m, *fields, w)
    solid, _ = ref.impulse(np.where(m != 1, 0.0, 1.0), *fields, w)  # every listed point taken as ep1 = 0
    # a second call with accumulate = 1 on the (already masked) fields
    want2, mag2 = ref.impulse(m, *[interior(b, f) for f in uvw], w)
    b.ibm_body_loads(ibm.h, *uvw, row.data_ptr(), 1)
    got2 = raw_of(row)
    return dict(same_bits=bool(same_bits), outside_untouched=bool(outside_untouched), nseg=ibm.n_segments,
                row=got[:3].tolist(), slot3=float(got[3]), want=want.tolist(), mag=mag.tolist(), solid=solid.tolist(),
                row2=got2[:3].tolist(), want2=(want + want2).tolist(), mag2=(mag + mag2).tolist())


def check_body_loads(kind, r):
    assert r["same_bits"] and r["outside_untouched"]
    assert r["slot3"] == 7.0  # (the call writes three slots)
    if kind == "ones":
        assert r["nseg"] == 0 and r["row"] == [0.0, 0.0, 0.0] and r["row2"] == [0.0, 0.0, 0.0]
        return
    assert r["nseg"] > 0 and min(r["mag"]) > 0.0
    check_rows([("%s %s" % (kind, c), abs(r["row"][k] - r["want"][k]), BOUND * r["mag"][k]) for k, c in enumerate("uvw")])
    check_rows([("%s %s twice" % (kind, c), abs(r["row2"][k] - r["want2"][k]), BOUND * r["mag2"][k]) for k, c in enumerate("uvw")])
    if kind == "fractional":  # (1 - ep1) is a factor: far from what a mask of zeros on the same list would give
        for k in range(3):
            assert abs(r["row"][k] - r["solid"][k]) > 1e6 * BOUND * r["mag"][k]


def uniform_flow_case(dims=(65, 12, 6), U=1.25):
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.ibm import Ibm, cylinder_mask
    b = stretched_backend(dims)
    assert np.ptp(np.diff(np.asarray(b.mesh.vert_coords[1]))) > 0.01
    ep1 = cylinder_mask(b.mesh, (0.4 * tib.L[0], 0.5 * tib.L[1]), 0.2 * tib.L[1])
    ibm = Ibm(SimpleNamespace(backend=b), ep1)
    w = ref.weights(b.mesh)
    set_weights(b, ibm, w)
    u, v, wf = (b.allocator.get_block(DIR_X, VERT) for _ in range(3))
    for f, val in zip((u, v, wf), (U, 0.0, 0.0)):
        f.fill(val)
    row = new_row(b, 3.0)
    b.ibm_body_loads(ibm.h, u, v, wf, row.data_ptr(), 0)
    got = raw_of(row)
    vol = ref.masked_volume(ep1, w)
    return dict(row=got[:3].tolist(), vol=vol, U=U, n_masked=ibm.n_masked)


def check_uniform_flow(r):
    assert r["n_masked"] > 20 and r["vol"] > 0.0
    check_rows([("uniform flow u", abs(r["row"][0] - r["U"] * r["vol"]), BOUND * r["U"] * r["vol"])])
    assert r["row"][1] == 0.0 and r["row"][2] == 0.0


class Stub:
    """the part of Solver that Loads and Probes read"""

    def __init__(self, backend, nstage=1, dt=0.0075):
        from x3d2_amd.common import DIR_X, VERT
        self.backend, self.mesh, self.dt, self.current_iter = backend, backend.mesh, dt, 0
        self.time_integrator = SimpleNamespace(nstage=nstage)
        self.ibm = None
        self.u, self.v, self.w = (backend.allocator.get_block(DIR_X, VERT) for _ in range(3))

    def flush_grad(self):
        pass


def probe_points(mesh):
    """7 points: the first and the last vertex of every axis, a tie in x (the lower index wins), and points off the
    vertices; -> (points, the global 0-based indices they must snap to)"""
    from x3d2_amd.diagnostics import global_vert_coords
    c = [global_vert_coords(mesh, d) for d in range(3)]
    n = [a.size for a in c]
    mid = 0.5 * (c[0][:-1] + c[0][1:])
    tie = int(np.flatnonzero(mid - c[0][:-1] == c[0][1:] - mid)[2])  # a midpoint that is EXACTLY as far from both vertices
    idx = [(0, 0, 0), (n[0] - 1, n[1] - 1, n[2] - 1), (n[0] - 1, 0, 2), (0, n[1] - 1, 0), (3, 2, n[2] - 1), (tie, 4, 3),
           (n[0] // 2, n[1] // 2, n[2] // 2)]
    pts = np.array([[c[d][i[d]] for d in range(3)] for i in idx])
    pts[5, 0] = mid[tie]
    pts[6] += [0.3 * (c[0][1] - c[0][0]), -0.4 * (c[1][1] - c[1][0]), 0.2 * (c[2][1] - c[2][0])]
    return pts, np.array(idx)


def probes_case(dims, prefix):
    """three samples of three seeded field sets: dict(rows [3][21], want [3][21], file coordinates ok)"""
    from x3d2_amd.diagnostics import parse_csv
    from x3d2_amd.probes import Probes, ProbesConfig
    b = tib.make_backend(dims)
    s = Stub(b)
    pts, idx = probe_points(b.mesh)
    pr = Probes(s, ProbesConfig(pts, prefix=prefix, flush_every=2))
    assert np.array_equal(pr.ijk, idx)
    want = []
    for it in range(1, 4):
        u, v, w = tib.random_blocks(b, 50 + it)
        pr.record(it, u, v, w)
        a = [b.get_field_data(f) for f in (u, v, w)]
        want.append([float(a[c][k, j, i]) for (i, j, k) in idx for c in range(3)])  # (widened: exact)
        pr.poll()
    pr.finalise()
    rows = pr.rows()
    cols, arr = parse_csv(prefix + ".csv")
    comments = [l for l in open(prefix + ".csv") if l.startswith("# probe")]
    coords_ok = len(comments) == 7
    for q, line in enumerate(comments):
        word = line.split()
        coords_ok &= [int(x) for x in word[4:7]] == [int(i) + 1 for i in idx[q]]
        coords_ok &= [float(x) for x in word[8:11]] == [float(x) for x in pr.xyz[q]]
    return dict(rows=pr.raw_rows().tolist(), want=want, iterations=[int(i) for i in rows["iteration"]],
                coords_ok=bool(coords_ok), ncol=len(cols), file_rows=arr.shape[0], sync_count=pr.sync_count)


def check_probes(r):
    assert r["iterations"] == [1, 2, 3] and r["ncol"] == 21 and r["file_rows"] == 3 and r["coords_ok"]
    assert np.array(r["rows"]).tobytes() == np.array(r["want"]).tobytes()  # the fields' own bits, in order
    assert len({tuple(x) for x in r["rows"]}) == 3


# ---------------------------------------------------------------- 1. field bits and rows
@pytest.mark.parametrize("kind", tib.MASKS)
@pytest.mark.parametrize("dims,xbc", tib.SHAPES)
def test_body_loads_gives_the_bits_of_body_and_the_numpy_row(dims, xbc, kind):
    check_body_loads(kind, body_loads_case(dims, xbc, kind))


# ---------------------------------------------------------------- 2. accumulate
def test_store_then_add_is_the_sum_and_a_store_forgets(tmp_path):
    from x3d2_amd.ibm import Ibm
    dims = (130, 9, 5)
    b = tib.make_backend(dims)
    ep1 = tib.make_mask("fractional", b.mesh).astype(tib.np_real())
    ibm = Ibm(SimpleNamespace(backend=b), ep1)
    w = ref.weights(b.mesh)
    set_weights(b, ibm, w)
    sets = [tib.random_blocks(b, seed) for seed in (21, 22, 23)]
    wants = [ref.impulse(ep1, *[interior(b, f) for f in fs], w) for fs in sets]
    row = new_row(b, 5.0)
    b.ibm_body_loads(ibm.h, *sets[0], row.data_ptr(), 0)
    b.ibm_body_loads(ibm.h, *sets[1], row.data_ptr(), 1)
    two = raw_of(row)
    b.ibm_body_loads(ibm.h, *sets[2], row.data_ptr(), 0)
    last = raw_of(row)
    check_rows([("store + add %s" % c, abs(two[k] - (wants[0][0][k] + wants[1][0][k])), BOUND * (wants[0][1][k] + wants[1][1][k]))
                for k, c in enumerate("uvw")])
    check_rows([("store again %s" % c, abs(last[k] - wants[2][0][k]), BOUND * wants[2][1][k]) for k, c in enumerate("uvw")])
    assert all(abs(last[k] - two[k]) > 1e6 * BOUND * wants[2][1][k] for k in range(3)) and two[3] == last[3] == 5.0
    # a mask of ones: exact zeros when stored, a pre-filled row unchanged when added
    ones = Ibm(SimpleNamespace(backend=b), np.ones_like(ep1))
    set_weights(b, ones, w)
    row = new_row(b, 2.5)
    b.ibm_body_loads(ones.h, *sets[0], row.data_ptr(), 1)
    assert raw_of(row).tolist() == [2.5] * 4
    b.ibm_body_loads(ones.h, *sets[0], row.data_ptr(), 0)
    assert raw_of(row).tolist() == [0.0, 0.0, 0.0, 2.5]


# ---------------------------------------------------------------- 3. uniform flow
def test_uniform_flow_gives_U_times_the_masked_volume():
    check_uniform_flow(uniform_flow_case())


# ---------------------------------------------------------------- 4. determinism, deferred execution
def test_a_row_repeats_bit_for_bit_and_behind_queued_calls():
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.ibm import Ibm
    dims, out = (65, 12, 6), {}
    for lazy in (False, True, "again"):
        b = tib.make_backend(dims, lazy=bool(lazy) and lazy != "again")
        ibm = Ibm(SimpleNamespace(backend=b), tib.make_mask("fractional", b.mesh))
        set_weights(b, ibm, ref.weights(b.mesh))
        rng = np.random.default_rng(2)
        u, v, w = (b.allocator.get_block(DIR_X, VERT) for _ in range(3))
        for f in (u, v, w):
            f.fill(0.0)
            b.set_field_data(f, rng.standard_normal((6, 12, 65), dtype=np.float32).astype(np.float64))
        b.vecadd(0.5, v, 1.0, u)  # recorded, not run, while the deferred layer is on
        b.field_scale(w, 1.25)
        row = new_row(b)
        b.ibm_body_loads(ibm.h, u, v, w, row.data_ptr(), 0)
        b.vecadd(1.0, u, 1.0, v)
        fields = [b.get_field_data(f) for f in (u, v, w)]
        out[lazy] = (raw_of(row), fields)
    for other in (True, "again"):
        assert out[other][0].tobytes() == out[False][0].tobytes()
        assert all(a.tobytes() == c.tobytes() for a, c in zip(out[other][1], out[False][1]))
    assert np.all(out[False][0][:3] != 0.0)


# ---------------------------------------------------------------- 5. the cylinder case
CASE_DIMS = (65, 32, 8)


def recording_ibm_class():
    from x3d2_amd.ibm import Ibm

    class RecordingIbm(Ibm):
        """copies u, v, w to the host before every body call and keeps the reference impulse of that call"""

        def body(self, u, v, w):
            b = self.backend
            fields = [b.get_field_data(f) for f in (u, v, w)]
            self.calls.append(ref.impulse(self.ep1.astype(tib.np_real()), *fields, self.w_ref))
            super().body(u, v, w)

    return RecordingIbm


def cylinder_case(time_intg, fused, record=False):
    import cylinder_ref
    from x3d2_amd import make_cylinder
    case = make_cylinder(CASE_DIMS, tib.L, time_intg=time_intg, fused=fused, **tib.BODY)
    s = case.solver
    assert s.ibm.area_ref == 2.0 * tib.BODY["radius"] * tib.L[2] and s.ibm.n_masked > 8
    if record:
        area = s.ibm.area_ref
        s.ibm = recording_ibm_class()(s, s.ibm.ep1)
        s.ibm.area_ref, s.ibm.calls, s.ibm.w_ref = area, [], ref.weights(s.mesh)
    pert = cylinder_ref.smooth_perturbation(s.mesh)
    for f, a in zip((s.u, s.v, s.w), (1.0 + pert[0], pert[1], pert[2])):
        s.backend.set_field_data(f, a)
    return case


@functools.lru_cache(maxsize=None)
def plain_run(time_intg, fused, nsteps=4):
    """the final u, v, w of the run without Loads; computed once per (integrator, driver)"""
    case = cylinder_case(time_intg, fused)
    case.run(n_iters=nsteps)
    return tuple(tib.fields_of(case))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("time_intg", ["RK3", "AB3"])
def test_case_rows_match_the_host_reference_and_the_fields_do_not_change(time_intg, fused, tmp_path):
    from x3d2_amd.diagnostics import parse_csv
    from x3d2_amd.loads import COLUMNS, Loads, LoadsConfig
    case = cylinder_case(time_intg, fused, record=True)
    s = case.solver
    cfg = LoadsConfig(prefix=str(tmp_path / "loads"), flush_every=3, u_ref=1.0)
    case.loads = Loads(s, cfg)
    assert s.ibm.loads is case.loads and not hasattr(case.loads, "reads_state")
    n0 = s.backend.sync_count()
    case.run(n_iters=4)
    ns = s.time_integrator.nstage
    assert ns == (3 if time_intg == "RK3" else 1) and len(s.ibm.calls) == 4 * ns
    raw, rows = case.loads.raw_rows(), case.loads.rows()
    assert raw.shape == (4, 4) and list(rows["iteration"]) == [1, 2, 3, 4] and np.all(raw[:, 3] == 0.0)
    checks = []
    for r in range(4):
        want = sum(c[0] for c in s.ibm.calls[r * ns:(r + 1) * ns])
        mag = sum(c[1] for c in s.ibm.calls[r * ns:(r + 1) * ns])
        checks += [("step %d %s" % (r + 1, c), abs(raw[r, k] - want[k]), BOUND * mag[k]) for k, c in enumerate("uvw")]
    check_rows(checks)
    assert np.all(raw[:, 0] > 0.0)  # the body takes momentum out of a flow along +x
    for k, c in enumerate("xyz"):
        assert np.array_equal(rows["f" + c], raw[:, k] / s.dt)
        assert np.array_equal(rows["c" + c], 2.0 / (1.0 * s.ibm.area_ref) * (raw[:, k] / s.dt))
    cols, arr = parse_csv(cfg.prefix + ".csv")
    assert cols == COLUMNS and arr.shape == (4, 7)
    assert np.allclose(arr[:, 1], rows["fx"], rtol=1e-12, atol=0.0) and np.allclose(arr[:, 0], s.dt * np.arange(1, 5), rtol=1e-12)
    assert case.loads.sync_count == 0
    print("host waits during the run with Loads:", s.backend.sync_count() - n0)
    for a, c in zip(tib.fields_of(case), plain_run(time_intg, fused)):
        assert a.tobytes() == c.tobytes()


def test_iloadfreq_2_leaves_the_even_steps_and_they_equal_the_every_step_rows(tmp_path):
    from x3d2_amd.loads import Loads, LoadsConfig
    out = {}
    for freq in (1, 2):
        case = cylinder_case("RK3", True)
        case.loads = Loads(case.solver, LoadsConfig(initload=freq, iloadfreq=freq, prefix=str(tmp_path / ("l%d" % freq))))
        case.run(n_iters=4)
        out[freq] = (case.loads.rows(), case.loads.raw_rows(), tib.fields_of(case))
    assert list(out[2][0]["iteration"]) == [2, 4]
    assert out[2][1].tobytes() == out[1][1][1::2].tobytes()
    assert all(a.tobytes() == c.tobytes() for a, c in zip(out[1][2], out[2][2]))


def test_loads_need_the_work_list_and_a_reference_area(monkeypatch, tmp_path):
    from x3d2_amd import make_cylinder
    from x3d2_amd.common import X3dError
    from x3d2_amd.ibm import Ibm
    from x3d2_amd.loads import Loads, LoadsConfig
    cfg = LoadsConfig(prefix=str(tmp_path / "l"))
    case = cylinder_case("AB3", False)
    s = case.solver
    ep1 = s.ibm.ep1
    s.ibm = Ibm(s, ep1)  # (a mask of the caller's: nobody knows its frontal area)
    with pytest.raises(X3dError):
        Loads(s, cfg)
    assert s.ibm.loads is None
    assert Loads(s, LoadsConfig(prefix=cfg.prefix, area_ref=2.0)).area_ref == 2.0
    s.ibm = Ibm(s, ep1, iibm=0)
    with pytest.raises(X3dError):
        Loads(s, LoadsConfig(prefix=cfg.prefix, area_ref=2.0))
    monkeypatch.setenv("X3D_NO_IBM_SPARSE", "1")
    s.ibm = Ibm(s, ep1)
    with pytest.raises(X3dError):
        Loads(s, LoadsConfig(prefix=cfg.prefix, area_ref=2.0))
    custom = make_cylinder((33, 16, 8), tib.L, ep1=np.ones((8, 16, 33)))
    assert custom.solver.ibm.area_ref is None and custom.loads is None and custom.probes is None


# ---------------------------------------------------------------- 6. probes
@pytest.mark.parametrize("dims", [(33, 16, 8), (130, 9, 5)])
def test_probes_hold_the_bits_of_the_fields_at_the_snapped_vertices(dims, tmp_path):
    check_probes(probes_case(dims, str(tmp_path / "probes")))


# ---------------------------------------------------------------- 7. the series
def test_seven_due_steps_cross_two_row_tables_in_order_without_a_wait(tmp_path):
    from x3d2_amd.loads import Loads, LoadsConfig
    from x3d2_amd.probes import Probes, ProbesConfig
    case = cylinder_case("AB3", True)
    s = case.solver
    pts, idx = probe_points(s.mesh)
    case.loads = Loads(s, LoadsConfig(prefix=str(tmp_path / "loads"), flush_every=2))
    case.probes = Probes(s, ProbesConfig(pts, prefix=str(tmp_path / "probes"), flush_every=2))
    assert all(case.probes.reads_state(it) for it in range(1, 8))
    case.run(n_iters=7)
    for series in (case.loads, case.probes):
        rows = series.rows()
        assert list(rows["iteration"]) == list(range(1, 8)) and np.all(np.diff(rows["time"]) > 0)
        assert series.sync_count == 0 and series.sample_count == 7
        assert len(open(series.file).read().splitlines()) == 8 + (7 if series is case.probes else 0)
    fields = tib.fields_of(case)
    last = case.probes.raw_rows()[-1].reshape(7, 3)
    for q, (i, j, k) in enumerate(idx):
        assert [float(f[k, j, i]) for f in fields] == last[q].tolist()
    assert len({r.tobytes() for r in case.loads.raw_rows()}) == 7


def test_every_attachment_at_once_fills_both_slots_of_every_ring(tmp_path):
    """snapshots, checkpoints, diagnostics, loads and probes on one cylinder run, tables of one or two rows: nine packed
    buffers on one backend (2 + 1 + 2 + 2 + 2), each of which the library keeps a pair of copy events for"""
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints
    from x3d2_amd.diagnostics import Diagnostics, DiagnosticsConfig
    from x3d2_amd.loads import Loads, LoadsConfig
    from x3d2_amd.probes import Probes, ProbesConfig
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots
    case = cylinder_case("AB3", True)
    s = case.solver
    pts, _ = probe_points(s.mesh)
    snap, ck = str(tmp_path / "snapshot"), str(tmp_path / "checkpoint")
    case.snapshots = Snapshots(s, SnapshotConfig(snapshot_freq=1, snapshot_prefix=snap, output_stride=(2, 2, 2)))
    case.checkpoints = Checkpoints(s, CheckpointConfig(checkpoint_freq=2, checkpoint_prefix=ck), case)
    case.diagnostics = Diagnostics(s, DiagnosticsConfig(prefix=str(tmp_path / "diagnostics"), flush_every=1))
    case.loads = Loads(s, LoadsConfig(prefix=str(tmp_path / "loads"), flush_every=1))
    case.probes = Probes(s, ProbesConfig(pts, prefix=str(tmp_path / "probes"), flush_every=2))
    case.run(n_iters=6)
    rings = [case.snapshots.ring, case.checkpoints.ring, case.diagnostics.ring, case.loads.ring, case.probes.ring]
    assert [r.allocated for r in rings] == [2, 1, 2, 2, 2]
    assert len({slot.dev.data_ptr() for r in rings for slot in r.slots}) == 9
    assert case.snapshots.files == [snap + "_%06d.npz" % it for it in range(1, 7)]
    assert all(os.path.exists(ck + "_%06d.npz" % it) for it in (2, 4, 6))
    for series in (case.diagnostics, case.loads, case.probes):
        rows = series.rows()
        assert list(rows["iteration"]) == list(range(1, 7))
        assert all(np.all(np.isfinite(rows[c])) for c in series.columns)
    assert np.all(case.loads.rows()["fx"] > 0.0)


def test_a_body_call_from_outside_the_step_is_reported_at_the_next_step(tmp_path):
    from x3d2_amd.common import X3dError
    from x3d2_amd.loads import Loads, LoadsConfig
    case = cylinder_case("AB3", True)
    s = case.solver
    case.loads = Loads(s, LoadsConfig(prefix=str(tmp_path / "loads")))
    case.run(n_iters=1)
    s.ibm.body(s.u, s.v, s.w)  # (counted as iteration 2's)
    fields = tib.fields_of(case)
    with pytest.raises(X3dError):
        s.ibm.body(s.u, s.v, s.w)  # the count says iteration 3, the solver is about to take iteration 2: nothing is launched
    assert all(a.tobytes() == c.tobytes() for a, c in zip(tib.fields_of(case), fields))
    with pytest.raises(X3dError):
        case.run(n_iters=2)


# ---------------------------------------------------------------- 8. restart
def test_restarted_series_equal_the_uninterrupted_ones_byte_for_byte(tmp_path):
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    from x3d2_amd.loads import Loads, LoadsConfig
    from x3d2_amd.probes import Probes, ProbesConfig

    def attach(case, where, append=False):
        s = case.solver
        pts, _ = probe_points(s.mesh)
        case.loads = Loads(s, LoadsConfig(prefix=str(where / "loads"), flush_every=4), append=append)
        case.probes = Probes(s, ProbesConfig(pts, prefix=str(where / "probes"), flush_every=4), append=append)

    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir()
    two.mkdir()
    case = cylinder_case("AB3", True)
    attach(case, one)
    case.run(n_iters=6)
    ck = str(two / "checkpoint")
    first = cylinder_case("AB3", True)
    attach(first, two)
    first.checkpoints = Checkpoints(first.solver, CheckpointConfig(checkpoint_freq=3, checkpoint_prefix=ck), first)
    first.run(n_iters=5)  # (two steps beyond the checkpoint: the restarted run drops their rows)
    assert len(open(str(two / "loads.csv")).read().splitlines()) == 6
    again = cylinder_case("AB3", True)
    assert restore(again, ck + "_000003.npz") == 3 and again.restarted
    attach(again, two, append=again.restarted)
    assert len(open(str(two / "loads.csv")).read().splitlines()) == 4
    again.run(n_iters=6)
    assert list(again.loads.rows()["iteration"]) == [4, 5, 6]
    for name in ("loads.csv", "probes.csv"):
        full = open(str(one / name), "rb").read()
        assert len(full.splitlines()) == 7 + (7 if name == "probes.csv" else 0)
        assert open(str(two / name), "rb").read() == full, name


# ---------------------------------------------------------------- 9. two ranks
BOX = (48, 24, 24)
BOX_STEPS, BOX_STAGES = 3, 3
BOX_PROBES = [(3, 2, 5), (40, 20, 20), (10, 12, 12), (0, 11, 11), (47, 23, 23), (7, 12, 3), (9, 3, 12)]  # (i, j, k), 0-based


def box_global():
    """the global mesh, sphere mask and probe points of the two-rank case: a sphere about the middle of a periodic box,
    which both the y cut and the z cut (index 12) go through; probes on both sides of either cut and on the cut planes"""
    from x3d2_amd import Mesh
    from x3d2_amd.ibm import cylinder_mask
    mesh = Mesh(BOX, (1, 1, 1), (2.0 * math.pi,) * 3, PER, PER, PER)
    ep1 = cylinder_mask(mesh, (math.pi, math.pi, math.pi), 1.2, axis=None)
    pts = np.array([[mesh.vert_coords[d][p[d]] for d in range(3)] for p in BOX_PROBES])
    return mesh, ep1, pts


def box_fields(it, sub):
    rng = np.random.default_rng(9000 + 10 * it + sub)
    return [rng.standard_normal((BOX[2], BOX[1], BOX[0]), dtype=np.float32).astype(np.float64) for _ in range(3)]


def box_run(nproc_dir, rank, comm, prefix):
    """every rank masks its part of the same global random fields, BOX_STAGES body calls a step, and samples its probes;
    -> (load rows [steps, 4], probe rows [steps, 21]) as landed, that is, combined over the ranks"""
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.common import VERT
    from x3d2_amd.ibm import Ibm
    from x3d2_amd.loads import Loads, LoadsConfig
    from x3d2_amd.probes import Probes, ProbesConfig
    _, ep1, pts = box_global()
    mesh = Mesh(BOX, tuple(nproc_dir), (2.0 * math.pi,) * 3, PER, PER, PER, nrank=rank)
    b = HipBackend(mesh, comm=comm)
    s = Stub(b, nstage=BOX_STAGES)
    lo, nl = [int(v) for v in mesh.n_offset], [int(v) for v in mesh.get_dims(VERT)]
    cut = (slice(lo[2], lo[2] + nl[2]), slice(lo[1], lo[1] + nl[1]), slice(lo[0], lo[0] + nl[0]))
    s.ibm = Ibm(s, np.ascontiguousarray(ep1[cut]))
    assert 0 < s.ibm.n_masked < int((ep1 == 0).sum()) or int(np.prod(nproc_dir)) == 1  # the body straddles the cut
    loads = Loads(s, LoadsConfig(prefix=prefix + "_loads", flush_every=2, area_ref=1.0))
    probes = Probes(s, ProbesConfig(pts, prefix=prefix + "_probes", flush_every=2))
    assert np.array_equal(probes.ijk, np.array(BOX_PROBES))
    assert 0 < probes.owned.size < len(BOX_PROBES) or int(np.prod(nproc_dir)) == 1
    for it in range(1, BOX_STEPS + 1):
        for sub in range(BOX_STAGES):
            for f, a in zip((s.u, s.v, s.w), box_fields(it, sub)):
                b.set_field_data(f, np.ascontiguousarray(a[cut]))
            s.ibm.body(s.u, s.v, s.w)
        s.current_iter = it
        assert probes.update(it)
        loads.poll()
        probes.poll()
    loads.finalise()
    probes.finalise()
    return loads.raw_rows(), probes.raw_rows(), loads.file is not None


@functools.lru_cache(maxsize=None)
def box_one_rank(prefix):
    return box_run((1, 1, 1), 0, None, prefix)


@pytest.mark.parametrize("layout,port", [((1, 1, 2), 29561), ((1, 2, 1), 29562)])
def test_two_ranks_give_the_one_rank_rows(layout, port, tmp_path_factory, tmp_path):
    """two processes share the GPU and exchange through gloo (tests/mp_loads_worker.py): load rows within twice the bound
    of the one-rank rows (two partial sums, then one more addition), probe rows bit-equal"""
    one_loads, one_probes, _ = box_one_rank(str(tmp_path_factory.getbasetemp() / "box_one"))
    mesh, ep1, _ = box_global()
    w = ref.weights(mesh)
    checks = []
    for it in range(1, BOX_STEPS + 1):
        parts = [ref.impulse(ep1, *box_fields(it, sub), w) for sub in range(BOX_STAGES)]
        want, mag = sum(p[0] for p in parts), sum(p[1] for p in parts)
        checks += [("one rank step %d %s" % (it, c), abs(one_loads[it - 1, k] - want[k]), BOUND * mag[k]) for k, c in enumerate("uvw")]
    check_rows(checks)
    out = str(tmp_path / "mp")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(HERE, "mp_loads_worker.py"),
           ",".join(map(str, layout)), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    parts = [dict(np.load(out + ".%d.npz" % k)) for k in range(2)]
    assert parts[0]["loads"].tobytes() == parts[1]["loads"].tobytes() and parts[0]["probes"].tobytes() == parts[1]["probes"].tobytes()
    assert bool(parts[0]["has_file"]) and not bool(parts[1]["has_file"])
    got = parts[0]["loads"]
    assert got.shape == (BOX_STEPS, 4) and np.all(got[:, 3] == 0.0)
    checks = []
    for it in range(1, BOX_STEPS + 1):
        mag = sum(ref.impulse(ep1, *box_fields(it, sub), w)[1] for sub in range(BOX_STAGES))
        checks += [("two ranks step %d %s" % (it, c), abs(got[it - 1, k] - one_loads[it - 1, k]), 2 * BOUND * mag[k])
                   for k, c in enumerate("uvw")]
    check_rows(checks)
    assert parts[0]["probes"].tobytes() == one_probes.tobytes() and np.all(one_probes != 0.0)
    assert len(open(out + "_probes.csv").read().splitlines()) == 1 + 7 + BOX_STEPS


# ---------------------------------------------------------------- 10. FP32
def test_fp32_flavour(tmp_path):
    """field bits, the numpy rows, the uniform flow and the probes on 4-byte reals (libx3d2_hip_sp.so), in a process of its
    own; the rows are FP64 there too and meet the same bound"""
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "loads_sp_worker.py"), str(tmp_path / "sp_probes")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("LOADSRESULT ")][-1][12:])
    assert res["dtype"] == "float32" and sorted(res["body"]) == sorted(tib.MASKS)
    for kind, case in res["body"].items():
        check_body_loads(kind, case)
    check_uniform_flow(res["uniform"])
    check_probes(res["probes"])


# ---------------------------------------------------------------- 11. errors
def test_every_refused_call_launches_nothing(tmp_path):
    from x3d2_amd import _lib
    from x3d2_amd.common import VERT, X3dError
    from x3d2_amd.ibm import Ibm
    from x3d2_amd.probes import Probes, ProbesConfig
    dims = (33, 16, 8)
    b, other = tib.make_backend(dims), tib.make_backend(dims)
    ep1 = tib.make_mask("cylinder", b.mesh)
    ibm, foreign, bare = (Ibm(SimpleNamespace(backend=x), ep1) for x in (b, other, b))
    w = ref.weights(b.mesh)
    set_weights(b, ibm, w)
    set_weights(other, foreign, w)
    u, v, wf = tib.random_blocks(b, 5)
    before = [tib.whole(b, f) for f in (u, v, wf)]
    row = new_row(b, 4.0)
    refused = [lambda: b.ibm_body_loads(ibm.h, u, v, wf, 0, 0),                  # a null row
               lambda: b.ibm_body_loads(foreign.h, u, v, wf, row.data_ptr(), 0),  # another backend's mask
               lambda: b.ibm_body_loads(ibm.h, u, u, wf, row.data_ptr(), 0),      # one block twice
               lambda: b.ibm_body_loads(bare.h, u, v, wf, row.data_ptr(), 0),     # no weights
               lambda: _lib.check(b.lib.x3d_ibm_body_loads(b.h, ibm.h, u.ptr, v.ptr, wf.ptr, _lib.ints(32, 16, 8),
                                                           ctypes.c_void_p(row.data_ptr()), 0)),  # other dims
               lambda: _lib.check(b.lib.x3d_ibm_set_weights(ibm.h, None, None, None))]
    s = Stub(b)
    pts, _ = probe_points(b.mesh)
    pr = Probes(s, ProbesConfig(pts, prefix=str(tmp_path / "p")))
    alien = Probes(Stub(other), ProbesConfig(pts, prefix=str(tmp_path / "q")))
    refused += [lambda: b.probe_sample(pr.h, u, v, wf, 0),
                lambda: b.probe_sample(alien.h, u, v, wf, row.data_ptr()),
                lambda: _lib.check(b.lib.x3d_probe_sample(b.h, pr.h, u.ptr, v.ptr, wf.ptr, _lib.ints(32, 16, 8),
                                                          ctypes.c_void_p(row.data_ptr())))]  # the last vertex lies outside
    h = ctypes.c_void_p()
    for ijk, slots, n in (([33, 0, 0], [0], 1), ([0, 0, -1], [0], 1), ([0, 0, 0], [1], 1), ([0, 0, 0, 1, 1, 1], [0, 0], 2),
                          ([0, 0, 0], [0], 0), ([0, 0, 0], [0], 4097)):
        refused.append(lambda ijk=ijk, slots=slots, n=n: _lib.check(b.lib.x3d_probe_create(
            b.h, _lib.ints(*ijk), len(slots), _lib.ints(*slots), n, ctypes.byref(h))))
    for k, call in enumerate(refused):
        with pytest.raises(X3dError):
            call()
        assert h.value is None, k
    assert raw_of(row).tolist() == [4.0] * 4
    assert all(tib.whole(b, f).tobytes() == a.tobytes() for f, a in zip((u, v, wf), before))
    with pytest.raises(X3dError):
        Probes(s, ProbesConfig([[tib.L[0] + 0.1, 1.0, 1.0]], prefix=str(tmp_path / "r")))
    with pytest.raises(X3dError):
        Probes(s, ProbesConfig(pts, prefix=str(tmp_path / "r"), flush_every=4097))
    assert not os.path.exists(str(tmp_path / "r.csv"))  # a refused construction touches no file
    b.ibm_body_loads(ibm.h, u, v, wf, row.data_ptr(), 0)  # (and the accepted call does run)
    assert raw_of(row)[3] == 4.0 and np.all(raw_of(row)[:3] != 4.0)
