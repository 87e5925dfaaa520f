"""Device-side diagnostics series (csrc/diagnostics.hip, x3d2_amd/diagnostics.py) against the numpy restatement
tests/diagnostics_ref.py (pinned on the host by tests/test_diagnostics_host.py).

Bounds of the synthetic cases (derived, not tuned), with eps the machine epsilon of the loaded library's real kind, ref the
restatement's exactly rounded value and A = sum over the points of sum_ij g_ij^2:
    slots 0-2   |dev - ref| <= 8 eps ref                    a sum of squares: one rounding per term, a tree of roundings
    slots 3, 4  |dev - ref| <= 32 eps A                     each integrand is at most 2 sum_ij g_ij^2 and carries a few
                                                            roundings of magnitude eps sum_ij g_ij^2
    slots 5, 6  |dev - ref| <= 8 eps sum |uy| on that row
    slots 8-10  bit-equal to numpy's abs().max()
    slot 11     |dev - ref| <= 16 eps ref                   slot 12   |dev - ref| <= 8 eps ref
Every block is filled with 1e30 before its data are set: a kernel that reads the row padding or stale pool contents fails
by thirty orders of magnitude."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import diagnostics_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2
SHAPES = [(64, 9, 8),     # one full wave of 16-byte loads per row (FP64: 32 lanes), pitch = nx: no padding at all
          (256, 5, 4),    # pitch 272 != nx: the +16 pad of rows of 256 points and more
          (17, 33, 10),   # an odd tail shorter than a wave; 330 rows: more work items than workgroups
          (130, 8, 9),    # two full waves plus a 2-point tail
          (257, 5, 4)]    # an odd channel-like row


# ---------------------------------------------------------------- helpers (also used by the worker processes)
def eps_real():
    from x3d2_amd import _lib
    return float(np.finfo(np.dtype(_lib.NP_REAL)).eps)


class Fields:
    """the part of Solver that Diagnostics.reduce / record read: mesh, backend, dt, nu, current_iter, flush_grad"""

    def __init__(self, backend, dt=1e-3, Re=1600.0):
        self.backend, self.mesh = backend, backend.mesh
        self.dt, self.nu, self.current_iter = dt, 1.0 / Re, 0

    def flush_grad(self):
        pass


def make_backend(dims, ybc=WALL, lazy=False, nproc_dir=(1, 1, 1), rank=0, comm=None):
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    mesh = Mesh(tuple(dims), nproc_dir, (1.0, 1.0, 1.0), PER, ybc, PER, nrank=rank)
    return HipBackend(mesh, lazy=lazy, comm=comm)


def poisoned_blocks(b, arrays):
    """fresh pool blocks, each filled with 1e30 and then given the interior `a`"""
    from x3d2_amd.common import DIR_X, VERT
    out = []
    for a in arrays:
        f = b.allocator.get_block(DIR_X, VERT)
        f.fill(1e30)
        b.set_field_data(f, a)
        out.append(f)
    return out


def random_arrays(dims, seed, count=12):
    """standard_normal fields [nz, ny, nx], exactly representable in both flavours"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(count)]


def random_tables(dims, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.5, 2.0, int(n)) for n in dims]


def diagnostics_of(s, prefix, tables=None, **kw):
    import torch
    from x3d2_amd.diagnostics import Diagnostics, DiagnosticsConfig
    dg = Diagnostics(s, DiagnosticsConfig(prefix=prefix, **kw))
    if tables is not None:
        dg.ih = [torch.from_numpy(np.ascontiguousarray(t)).to(s.backend.device) for t in tables]
    return dg


def raw_of(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def compare(got, arrays, tables, flags, eps):
    """[(slot name, |err|, bound)] of a device row against the restatement on the same arrays"""
    want = ref.row(arrays[0], arrays[1], arrays[2], arrays[3:], tables, flags)
    A = ref.grad_square_sum(arrays[3:])
    uy = np.abs(arrays[4])
    rows = []
    for k in (0, 1, 2):
        rows.append(("sum%d" % k, abs(got[k] - want[k]), 8 * eps * want[k]))
    for k in (3, 4):
        rows.append(("sum%d" % k, abs(got[k] - want[k]), 32 * eps * A))
    rows.append(("wall_lo", abs(got[5] - want[5]), 8 * eps * ref.fsum(uy[:, 0, :]) if flags[0] else 0.0))
    rows.append(("wall_hi", abs(got[6] - want[6]), 8 * eps * ref.fsum(uy[:, -1, :]) if flags[1] else 0.0))
    for k in (8, 9, 10):
        rows.append(("max%d" % k, abs(got[k] - want[k]), 0.0))
    rows.append(("max11", abs(got[11] - want[11]), 16 * eps * want[11]))
    rows.append(("max12", abs(got[12] - want[12]), 8 * eps * want[12]))
    for k in (7, 13, 14, 15):
        rows.append(("slot%d" % k, abs(got[k]), 0.0))
    return rows


def synthetic_rows(dims, prefix, seed=5):
    """twelve random blocks and random spacing tables through one reduce against the restatement"""
    b = make_backend(dims)
    s = Fields(b)
    arrays, tables = random_arrays(dims, seed), random_tables(dims, seed + 1)
    dg = diagnostics_of(s, prefix, tables, divergence=False)
    assert dg.first_y and dg.last_y and dg.columns[-2:] == ("tau_w_lo", "tau_w_hi")
    blocks = poisoned_blocks(b, arrays)
    got = raw_of(dg.reduce(blocks[0], blocks[1], blocks[2], blocks[3:]))
    return compare(got, arrays, tables, (True, True), eps_real())


def check_rows(rows):
    for r in rows:
        print("diagnostics check:", *r)
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, bad


# ---------------------------------------------------------------- 1. synthetic inputs
@pytest.mark.parametrize("dims", SHAPES)
def test_reduce_against_the_restatement(dims, tmp_path):
    from x3d2_amd import _lib
    b = make_backend(dims)
    assert b.padded_dims[0] != dims[0] or dims[0] % 16 == 0
    if dims == (256, 5, 4):
        assert b.padded_dims[0] == 272
    check_rows(synthetic_rows(dims, str(tmp_path / "d")))
    assert _lib.load().x3d_abi_version() == 1


# ---------------------------------------------------------------- 2. placement
def test_a_spike_lands_in_its_own_slots_only(tmp_path):
    dims = (130, 8, 9)
    nx, ny, nz = dims
    b = make_backend(dims)
    s = Fields(b)
    tables = random_tables(dims, 8)
    dg = diagnostics_of(s, str(tmp_path / "d"), tables, divergence=False)
    zero = np.zeros((nz, ny, nx))
    blocks = poisoned_blocks(b, [zero] * 12)
    spike = 3.0
    for (i, j, k) in ((0, 0, 0), (nx - 1, 0, 0), (nx - 1, ny - 1, nz - 1), (0, ny - 1, 0)):
        cfl = [tables[0][i], tables[1][j], tables[2][k]]
        for m in (0, 1, 2, 4):  # u, v, w, uy
            a = zero.copy()
            a[k, j, i] = -spike
            b.set_field_data(blocks[m], a)
            for flags in ((True, True), (False, False)):
                dg.first_y, dg.last_y = flags
                got = raw_of(dg.reduce(blocks[0], blocks[1], blocks[2], blocks[3:]))
                want = np.zeros(16)
                if m < 3:
                    want[m], want[8 + m], want[12] = spike * spike, spike, spike * cfl[m]
                else:
                    want[3], want[4], want[11] = spike * spike, 0.5 * spike * spike, spike * spike
                    if flags[0] and j == 0:
                        want[5] = -spike
                    if flags[1] and j == ny - 1:
                        want[6] = -spike
                assert np.array_equal(got, want), ((i, j, k), m, flags, got, want)
            b.set_field_data(blocks[m], zero)


# ---------------------------------------------------------------- 3. determinism
def test_a_row_is_a_function_of_the_fields_and_the_shape(tmp_path):
    dims = (17, 33, 10)
    b = make_backend(dims)
    s = Fields(b)
    arrays, tables = random_arrays(dims, 31), random_tables(dims, 32)
    dg = diagnostics_of(s, str(tmp_path / "d"), tables, divergence=False)
    blocks = poisoned_blocks(b, arrays)
    first = raw_of(dg.reduce(blocks[0], blocks[1], blocks[2], blocks[3:]))
    b.scalar_product(blocks[0], blocks[1])  # (an unrelated user of the reduction buffer in between)
    second = raw_of(dg.reduce(blocks[0], blocks[1], blocks[2], blocks[3:]))
    assert first.tobytes() == second.tobytes() and first[3] > 0.0
    fresh = poisoned_blocks(b, arrays)  # other allocations, other offsets
    assert {f.ptr for f in fresh}.isdisjoint({f.ptr for f in blocks})
    third = raw_of(dg.reduce(fresh[0], fresh[1], fresh[2], fresh[3:]))
    assert first.tobytes() == third.tobytes()


# ---------------------------------------------------------------- 4. no host wait
def _stepped_series(flush_every, prefix, nsteps=10):
    from x3d2_amd import make_tgv
    case = make_tgv(32, fused=True)
    s = case.solver
    b = s.backend
    dg = diagnostics_of(s, prefix, flush_every=flush_every)
    moved = 0
    for it in range(1, nsteps + 1):
        case.step(it)
        s.current_iter = it
        n0 = b.sync_count()
        assert dg.update(it)
        moved += b.sync_count() - n0
        dg.poll()
    return dg, moved


def test_ten_samples_make_no_host_wait_and_cross_the_tables_unchanged(tmp_path):
    dg, moved = _stepped_series(4, str(tmp_path / "a"))
    assert moved == 0 and dg.sync_count == 0
    dg.finalise()
    rows = dg.rows()
    assert len(rows) == 10 and list(rows["iteration"]) == list(range(1, 11))
    assert np.all(np.diff(rows["time"]) > 0) and np.all(rows["ke"] > 0) and np.all(rows["div_u_max"] > 0)
    big, moved = _stepped_series(256, str(tmp_path / "b"))
    assert moved == 0 and big.sync_count == 0
    big.finalise()
    assert dg.raw_rows().tobytes() == big.raw_rows().tobytes()
    assert open(str(tmp_path / "a.csv")).read() == open(str(tmp_path / "b.csv")).read()
    assert len(open(str(tmp_path / "a.csv")).read().splitlines()) == 11


# ---------------------------------------------------------------- 5. end to end, TGV
def test_tgv_series_agrees_with_monitoring_and_leaves_the_run_alone(tmp_path):
    """TGV 32^3, 3 steps, fused driver, a row per step.  div_u_max and div_u_mean are BIT-EQUAL to field_max_mean's:
    x3d_diag_max_sum runs that reduction's own first stage and adds its partials on the device in the order the host does."""
    from x3d2_amd import make_tgv
    from x3d2_amd.diagnostics import Diagnostics, DiagnosticsConfig, parse_csv
    eps = eps_real()
    case = make_tgv(32, fused=True)
    case.solver.n_output = 1
    assert case.diagnostics is None
    case.diagnostics = Diagnostics(case.solver, DiagnosticsConfig(prefix=str(tmp_path / "tgv")))
    kes, post = [], case.postprocess
    case.postprocess = lambda it, t: (kes.append(case.monitoring.kinetic_energy()), post(it, t))[1]
    mon = case.run(n_iters=3)
    rows = case.diagnostics.rows()
    assert list(rows["iteration"]) == [1, 2, 3] and len(mon) == 4 and len(kes) == 4
    for r, m, ke in zip(rows, mon[1:], kes[1:]):
        print("diagnostics check: tgv it", int(r["iteration"]), "enstrophy", r["enstrophy"], m[1], "div", r["div_u_max"], m[2],
              r["div_u_mean"], m[3], "ke", r["ke"], ke, "rel", abs(r["ke"] - ke) / ke / eps, "eps")
    for r, m, ke in zip(rows, mon[1:], kes[1:]):
        assert r["time"] == m[0]
        assert abs(r["enstrophy"] - m[1]) <= 1e-12 * m[1]
        assert r["div_u_max"] == m[2] and r["div_u_mean"] == m[3]
        assert abs(r["ke"] - ke) <= 8 * eps * ke
    # periodic, and solenoidal up to the scheme's error: <S_ij S_ij> - 1/2 <|curl u|^2> = <(div u)^2>, second order in an error
    # that is itself below 1e-6 at 32 points per wavelength
    assert abs(rows["dissipation"][0] - 2.0 * case.solver.nu * rows["enstrophy"][0]) <= 1e-6 * rows["dissipation"][0]
    plain = make_tgv(32, fused=True)
    plain.solver.n_output = 1
    plain.run(n_iters=3)
    sv, pv = case.solver, plain.solver
    for f, g in zip((sv.u, sv.v, sv.w), (pv.u, pv.v, pv.w)):
        assert sv.backend.get_field_data(f).tobytes() == pv.backend.get_field_data(g).tobytes()
    cols, back = parse_csv(str(tmp_path / "tgv.csv"))
    assert cols == case.diagnostics.columns and back.shape == (3, 1 + len(cols))


# ---------------------------------------------------------------- 6. channel
@pytest.mark.parametrize("fused,lazy", [(True, False), (False, True)])
def test_channel_wall_shear_and_cfl_against_the_restatement(fused, lazy, tmp_path):
    from x3d2_amd import make_channel
    from x3d2_amd.common import DIR_X, DIR_Y, VERT
    from x3d2_amd.diagnostics import Diagnostics, DiagnosticsConfig
    dims = (32, 17, 16)
    eps = eps_real()
    case = make_channel(dims, fused=fused, lazy=lazy)
    s = case.solver
    b = s.backend
    case.diagnostics = Diagnostics(s, DiagnosticsConfig(prefix=str(tmp_path / "ch")))
    assert case.diagnostics.columns[-2:] == ("tau_w_lo", "tau_w_hi")
    case.run(n_iters=2)
    rows = case.diagnostics.rows()
    assert list(rows["iteration"]) == [1, 2]
    last = rows[-1]
    g = b.allocator.get_block(DIR_X, VERT)
    b.tds_apply(g, s.u, s.ydirps.der1st, DIR_Y)
    uy = b.get_field_data(g, VERT).astype(np.float64)
    u, v, w = (b.get_field_data(f).astype(np.float64) for f in (s.u, s.v, s.w))
    m = s.mesh
    ih = [np.full(dims[0], 1.0 / float(m.d[0])), ref.inverse_spacing(m.vert_coords[1], False, float(m.L[1])),
          np.full(dims[2], 1.0 / float(m.d[2]))]
    zero = np.zeros_like(u)
    grads = [zero] * 9
    grads[1] = uy
    want = ref.derive(ref.row(u, v, w, grads, ih, (True, True)), np.prod(dims), 1.0, dims[0] * dims[2], s.nu, s.dt,
                      divergence=False, y_walls=True)
    scale = s.nu / (dims[0] * dims[2])
    print("diagnostics check: channel tau", last["tau_w_lo"], want["tau_w_lo"], last["tau_w_hi"], want["tau_w_hi"], "cfl",
          last["cfl"], want["cfl"])
    assert abs(last["tau_w_lo"] - want["tau_w_lo"]) <= 8 * eps * scale * ref.fsum(np.abs(uy[:, 0, :]))
    assert abs(last["tau_w_hi"] - want["tau_w_hi"]) <= 8 * eps * scale * ref.fsum(np.abs(uy[:, -1, :]))
    assert last["tau_w_lo"] > 0.0 and last["tau_w_hi"] > 0.0  # (the parabola: du/dy > 0 at the lower wall, < 0 at the upper)
    assert abs(last["cfl"] - want["cfl"]) <= 8 * eps * want["cfl"]
    assert last["u_max"] == want["u_max"] and abs(last["ke"] - want["ke"]) <= 8 * eps * want["ke"]
    if lazy:
        assert b.lazy_stats()["recorded"] > 0


# ---------------------------------------------------------------- 7. errors
def test_bad_calls_raise_and_a_valid_call_still_works(tmp_path):
    import ctypes
    import torch
    from x3d2_amd import _lib
    from x3d2_amd.common import X3dError
    dims = (64, 9, 8)
    b = make_backend(dims)
    s = Fields(b)
    arrays, tables = random_arrays(dims, 41), random_tables(dims, 42)
    dg = diagnostics_of(s, str(tmp_path / "d"), tables, divergence=False)
    blocks = poisoned_blocks(b, arrays)
    good = raw_of(dg.reduce(blocks[0], blocks[1], blocks[2], blocks[3:]))
    row = torch.zeros(16, dtype=torch.float64, device=b.device)
    prm = _lib.DiagParams(dg.ih[0].data_ptr(), dg.ih[1].data_ptr(), dg.ih[2].data_ptr(), 1, 1)
    gp = (ctypes.c_void_p * 9)(*[f.ptr for f in blocks[3:]])
    args = [b.h, blocks[0].ptr, blocks[1].ptr, blocks[2].ptr, gp, _lib.ints(*dims), ctypes.byref(prm), ctypes.c_void_p(row.data_ptr())]
    for k in (1, 4, 6, 7):  # u, the gradient table, the parameters, the row
        bad = list(args)
        bad[k] = None
        assert b.lib.x3d_diag_reduce(*bad) != 0 and b"null" in b.lib.x3d_last_error()
    gnull = (ctypes.c_void_p * 9)(*[f.ptr for f in blocks[3:11]], None)
    bad = list(args)
    bad[4] = gnull
    assert b.lib.x3d_diag_reduce(*bad) != 0 and b"null" in b.lib.x3d_last_error()
    bad = list(args)
    bad[5] = _lib.ints(64, 0, 8)
    assert b.lib.x3d_diag_reduce(*bad) != 0 and b"positive" in b.lib.x3d_last_error()
    assert b.lib.x3d_diag_max_sum(b.h, None, _lib.ints(*dims), ctypes.c_void_p(row.data_ptr())) != 0
    assert b.lib.x3d_diag_max_sum(b.h, blocks[0].ptr, _lib.ints(64, 9, -1), ctypes.c_void_p(row.data_ptr())) != 0
    assert not np.any(raw_of(row))  # nothing was launched
    with pytest.raises(X3dError, match="nine"):
        dg.reduce(blocks[0], blocks[1], blocks[2], blocks[3:11])
    with pytest.raises(X3dError, match="flush_every"):
        diagnostics_of(s, str(tmp_path / "e"), flush_every=10 ** 6)
    again = raw_of(dg.reduce(blocks[0], blocks[1], blocks[2], blocks[3:]))
    assert again.tobytes() == good.tobytes()
    assert b.lib.x3d_diag_reduce(*args) == 0 and raw_of(row).tobytes() == good.tobytes()
    assert b.lib.x3d_diag_max_sum(b.h, blocks[0].ptr, _lib.ints(*dims), ctypes.c_void_p(row.data_ptr())) == 0
    mx, sm = ref.max_sum(arrays[0])
    got = raw_of(row)
    assert got[13] == mx and abs(got[7] - sm) <= np.prod(dims) * eps_real() * sm  # (the worst case of ANY summation order)
    want_mx, want_mean = b.field_max_mean(blocks[0])
    assert got[13] == want_mx and got[7] / np.prod(dims) == want_mean  # bit-equal to the host-finished reduction


# ---------------------------------------------------------------- 8. restart
def test_restarted_series_equals_the_uninterrupted_one_byte_for_byte(tmp_path):
    from x3d2_amd import make_tgv
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    from x3d2_amd.diagnostics import Diagnostics, DiagnosticsConfig
    ck = str(tmp_path / "checkpoint")
    cfg = DiagnosticsConfig(prefix=str(tmp_path / "series"), flush_every=3)
    case = make_tgv(32, fused=True)
    case.diagnostics = Diagnostics(case.solver, cfg)
    case.checkpoints = Checkpoints(case.solver, CheckpointConfig(checkpoint_freq=2, checkpoint_prefix=ck), case)
    case.run(n_iters=4)
    full = open(cfg.prefix + ".csv").read()
    assert len(full.splitlines()) == 5
    again = make_tgv(32, fused=True)
    assert restore(again, ck + "_000002.npz") == 2 and again.restarted
    again.diagnostics = Diagnostics(again.solver, cfg, append=again.restarted)
    assert open(cfg.prefix + ".csv").read() == "".join(full.splitlines(True)[:3])  # the rows later than step 2 are gone
    again.run(n_iters=4)
    assert open(cfg.prefix + ".csv").read() == full
    assert list(again.diagnostics.rows()["iteration"]) == [3, 4]


# ---------------------------------------------------------------- 9. two ranks
def test_two_z_slabs_give_the_global_row(tmp_path):
    """two processes share the GPU and exchange through gloo (tests/mp_diagnostics_worker.py), z slabs, both with the wall
    flags on: the combined sums meet the one-rank bounds against the restatement on the GLOBAL arrays (a doubled wall
    contribution would not), the maxima are bit-equal, only rank 0 writes the file"""
    dims, n = (64, 9, 8), 3
    out = str(tmp_path / "mp")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", "29553", os.path.join(HERE, "mp_diagnostics_worker.py"),
           ",".join(map(str, dims)), str(n), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    parts = [dict(np.load(out + ".%d.npz" % k)) for k in range(2)]
    assert parts[0]["raw"].shape == (n, 16) and parts[0]["raw"].tobytes() == parts[1]["raw"].tobytes()
    assert list(parts[0]["iteration"]) == list(range(1, n + 1))
    assert bool(parts[0]["has_file"]) and not bool(parts[1]["has_file"])
    assert os.path.exists(out + ".csv") and len(open(out + ".csv").read().splitlines()) == n + 1
    tables = random_tables(dims, 77)
    rows = []
    for it in range(1, n + 1):
        rows += compare(parts[0]["raw"][it - 1], random_arrays(dims, 300 + it), tables, (True, True), eps_real())
    check_rows(rows)


# ---------------------------------------------------------------- 10. FP32
def test_reduce_in_the_fp32_flavour():
    """the synthetic case at (64, 9, 8) and (17, 33, 10) on 4-byte reals (libx3d2_hip_sp.so), in a process of its own, with
    the same bounds in that flavour's eps; the row is still FP64"""
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "diagnostics_sp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("DIAGRESULT ")][-1][11:])
    assert res["eps"] == float(np.finfo(np.float32).eps) and res["dtype"] == "float32" and res["row_dtype"] == "float64"
    assert len(res["rows"]) == 2 * 16
    check_rows([tuple(r) for r in res["rows"]])
