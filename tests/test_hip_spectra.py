"""Device-side energy spectra (csrc/spectrum.hip, x3d2_amd/spectra.py) against the numpy restatement tests/spectra_ref.py
(pinned on the host by tests/test_spectra_host.py).

Tolerance (derived, not tuned): a bin is a sum of non-negative terms bounded by the total; a Cooley-Tukey transform carries
a relative l2 error of order eps log2 N; squaring doubles it:

    |E_dev[b] - E_ref[b]| <= 16 eps_real log2(N) sum(E_ref)

with N the points of the transform (nx ny nz, plane mode: nx nz) and the total that of the field (plane mode: of the y row).
Before a comparison the test asserts on the host that no mode lies within 1e-9 dk of a bin edge.

Two notes on the cases.  (1) Shapes with fewer than 8 points along a direction (160 x 8 x 6) cannot carry a Solver -- the
compact operators need 8 rows -- so the bare shell cases build the FFT Poisson object alone, from host-side operators.
(2) The weights case: u = cos(pi i) + c has <u^2> = 1 + c^2 (cos(pi i) = +-1 on the grid), so its energy is
1/2 (1 + c^2), with 1/2 in the Nyquist bin and 1/2 c^2 in bin 0; a doubled Nyquist weight would give 1/2 (2 + c^2)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import spectra_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2
TWOPI = 6.283185307179586
BOX = (5.0, TWOPI, 3.0)


# ---------------------------------------------------------------- helpers (also used by tests/spectra_sp_worker.py)
def eps_real():
    from x3d2_amd import _lib
    return float(np.finfo(np.dtype(_lib.NP_REAL)).eps)


class Fields:
    """the part of Solver that Spectra reads: u, v, w, species, mesh, backend, flush_grad"""

    def __init__(self, backend, nspecies=0):
        from x3d2_amd.common import DIR_X, VERT
        self.backend, self.mesh = backend, backend.mesh
        self.u, self.v, self.w = (backend.allocator.get_block(DIR_X, VERT) for _ in range(3))
        self.species = [backend.allocator.get_block(DIR_X, VERT) for _ in range(nspecies)]
        self.flushes = 0

    def flush_grad(self):
        self.flushes += 1

    def set(self, arrays):
        for f, a in zip([self.u, self.v, self.w] + self.species, arrays):
            self.backend.set_field_data(f, a)


def periodic_fields(dims, L=(TWOPI,) * 3, lazy=False, poisson=True):
    """an all-periodic backend with its FFT Poisson object and three VERT fields, without a Solver"""
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.common import BC_PERIODIC, CELL
    from x3d2_amd.tdsops import Dirps, Tdsops
    mesh = Mesh(tuple(dims), (1, 1, 1), tuple(L), PER, PER, PER)
    b = HipBackend(mesh, lazy=lazy)
    if poisson:
        dps = []
        for d in range(3):  # (the wave numbers of the solve need these two of every direction; host objects)
            dp, n = Dirps(d + 1), int(mesh.get_dims(CELL)[d])
            dp.stagder_v2p = Tdsops(n, float(mesh.d[d]), "stag-deriv", "compact6", BC_PERIODIC, BC_PERIODIC, from_to="v2p")
            dp.interpl_v2p = Tdsops(n, float(mesh.d[d]), "interpolate", "classic", BC_PERIODIC, BC_PERIODIC, from_to="v2p")
            dps.append(dp)
        b.init_poisson_fft(mesh, *dps)
    return Fields(b)


def channel_fields(dims=(32, 17, 16)):
    """the channel's mesh (y Dirichlet and stretched) through make_channel; its solver is what Spectra reads"""
    from x3d2_amd import make_channel
    return make_channel(dims).solver


def random_arrays(dims, seed, count=3):
    """standard_normal fields [nz, ny, nx], exactly representable in both flavours"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(count)]


def set_fields(s, arrays):
    for f, a in zip((s.u, s.v, s.w), arrays):
        s.backend.set_field_data(f, a)


def spectra_of(s, mode, **kw):
    from x3d2_amd.spectra import Spectra, SpectraConfig
    return Spectra(s, SpectraConfig(mode=mode, initspec=1, **kw))


def shell_rows(dims, L, dk=None, seed=3):
    """random u, v, w through one shell sample against the checker: [(name, worst |err|, bound)]"""
    s = periodic_fields(dims, L)
    arrays = random_arrays(dims, seed)
    set_fields(s, arrays)
    sp = spectra_of(s, "shell", dk=dk)
    dk = spectra_ref.default_dk(L) if dk is None else dk
    _, margin = spectra_ref.shell_bins(dims, L, dk)
    assert margin > 1e-9, "a mode sits on a bin edge: choose other box lengths"
    sp.sample()
    got = sp.spectrum()
    assert got["k"].size == spectra_ref.nbins(dims, L, dk) and np.array_equal(got["k"], np.arange(got["k"].size) * dk)
    rows, n = [], float(np.prod(dims))
    for name, a in zip("uvw", arrays):
        ref = spectra_ref.shell(a, L, dk)
        assert got["E_" + name].shape == ref.shape
        rows.append(("E_" + name, float(np.max(np.abs(got["E_" + name] - ref))), spectra_ref.tolerance(n, eps_real(), ref.sum())))
    assert np.array_equal(got["E"], (got["E_u"] + got["E_v"]) + got["E_w"])
    return rows, sp


def plane_rows(s, dims, seed=4):
    """random u, v, w through one plane sample against the checker, row by row, and both sums against the row's 1/2 <f^2>"""
    arrays = random_arrays(dims, seed)
    set_fields(s, arrays)
    sp = spectra_of(s, "plane")
    sp.sample()
    got = sp.spectrum()
    nx, ny, nz = dims
    assert np.array_equal(got["y"], np.asarray(s.mesh.vert_coords[1], dtype=np.float64)[:ny])
    assert got["kx"].shape == (nx // 2 + 1,) and got["kz"].shape == (nz // 2 + 1,)
    rows, n = [], float(nx * nz)
    for name, a in zip("uvw", arrays):
        ex, ez = spectra_ref.plane(a)
        gx, gz = got["Ex_" + name], got["Ez_" + name]
        assert gx.shape == ex.shape == (ny, nx // 2 + 1) and gz.shape == ez.shape == (ny, nz // 2 + 1)
        half = 0.5 * np.mean(a * a, axis=(0, 2))  # the plane's 1/2 <f^2>
        for j in range(ny):
            tol = spectra_ref.tolerance(n, eps_real(), ex[j].sum())
            rows.append(("Ex_%s[%d]" % (name, j), float(np.max(np.abs(gx[j] - ex[j]))), tol))
            rows.append(("Ez_%s[%d]" % (name, j), float(np.max(np.abs(gz[j] - ez[j]))), tol))
            rows.append(("sum Ex_%s[%d]" % (name, j), abs(float(gx[j].sum()) - half[j]), tol))
            rows.append(("sum Ez_%s[%d]" % (name, j), abs(float(gz[j].sum()) - half[j]), tol))
    return rows, sp


def check_rows(rows, quiet=False):
    worst = max(rows, key=lambda r: r[-2] / r[-1] if r[-1] > 0 else (0.0 if r[-2] == 0 else np.inf))
    print("spectra check: %d rows, worst %s err %.3e bound %.3e" % (len(rows), worst[0], worst[-2], worst[-1]))
    if not quiet:
        for r in rows[:12]:
            print("spectra check:", *r)
    bad = [r for r in rows if not r[-2] <= r[-1]]
    assert not bad, bad[:8]


# ---------------------------------------------------------------- 1. shell mode against the checker
# 16^3: 9 modes per row, less than a wave.  40 x 24 x 12 in (5, 2 pi, 3): three distinct dims and lengths, 21 modes padded to
# 24 -- the pad columns must count for nothing.  160 x 8 x 6: 81 modes, a row spans two waves; with the default dk = 1 the
# modes 63 and 64 of a row never share a bin, with dk = 2.2 they do in every row: a bin segment crosses the wave boundary.
# 48 x 40 x 36: 1440 row segments, 45 workgroup partials of 8 segments per wave.
SHELL_CASES = [((16, 16, 16), (TWOPI,) * 3, None), ((40, 24, 12), BOX, None), ((160, 8, 6), (TWOPI,) * 3, None),
               ((160, 8, 6), (TWOPI,) * 3, 2.2), ((48, 40, 36), BOX, None)]


@pytest.mark.parametrize("dims,L,dk", SHELL_CASES)
def test_shell_against_the_numpy_checker(dims, L, dk):
    rows, sp = shell_rows(dims, L, dk)
    if dims == (48, 40, 36):
        assert sp.groups > 1
    if dk == 2.2:  # (a bin whose modes lie on both sides of lane 63 | 64 of a row)
        b, _ = spectra_ref.shell_bins(dims, L, dk)
        assert np.all(b[:, :, 63] == b[:, :, 64])
    check_rows(rows)


# ---------------------------------------------------------------- 2. - 4. known answers
def test_tgv_initial_condition_puts_its_energy_into_bin_2():
    from x3d2_amd import make_tgv
    case = make_tgv(16)
    sp = spectra_of(case.solver, "shell")
    sp.sample()
    E = sp.spectrum()["E"]
    tol = spectra_ref.tolerance(16.0 ** 3, eps_real(), 0.125)
    print("spectra check: tgv E[2]", E[2], "others", float(np.max(np.delete(E, 2))), "bound", tol)
    assert E.shape == (15,)
    assert abs(E[2] - 0.125) <= tol
    assert np.all(np.delete(E, 2) <= tol)


def test_sum_over_the_bins_is_the_kinetic_energy():
    from x3d2_amd import make_tgv
    case = make_tgv(16)
    s = case.solver
    set_fields(s, random_arrays((16, 16, 16), 9))
    sp = spectra_of(s, "shell")
    sp.sample()
    E = sp.spectrum()["E"]
    ke = case.monitoring.kinetic_energy()
    tol = spectra_ref.tolerance(16.0 ** 3, eps_real(), ke)
    print("spectra check: parseval", float(E.sum()), ke, "bound", tol)
    assert abs(float(E.sum()) - ke) <= tol


def test_nyquist_mode_is_not_doubled():
    dims, c = (16, 16, 16), 0.75
    s = periodic_fields(dims)
    u = np.cos(np.pi * np.arange(16))[None, None, :] + c + np.zeros((16, 16, 16))
    set_fields(s, [u, np.zeros_like(u), np.zeros_like(u)])
    sp = spectra_of(s, "shell")
    sp.sample()
    got = sp.spectrum()
    total = 0.5 * (1.0 + c * c)
    tol = spectra_ref.tolerance(16.0 ** 3, eps_real(), total)
    E = got["E_u"]
    print("spectra check: nyquist", E[8], E[0], float(E.sum()), "bound", tol)
    assert abs(float(E.sum()) - total) <= tol
    assert abs(E[8] - 0.5) <= tol and abs(E[0] - 0.5 * c * c) <= tol  # kx = 8 = the Nyquist mode, weight 1
    assert np.max(np.abs(E - spectra_ref.shell(u, (TWOPI,) * 3))) <= tol
    assert not np.any(got["E_v"]) and not np.any(got["E_w"])


# ---------------------------------------------------------------- 5. reproducibility
@pytest.mark.parametrize("mode", ["shell", "plane"])
def test_same_field_twice_gives_the_same_bytes(mode):
    dims = (40, 24, 12)
    s = periodic_fields(dims, BOX)
    set_fields(s, random_arrays(dims, 21))
    sp = spectra_of(s, mode)
    sp.sample()
    first = sp._read(0)
    b = s.backend
    from x3d2_amd.common import DIR_X, VERT
    t = b.allocator.get_block(DIR_X, VERT)
    b.veccopy(t, s.u)           # unrelated launches in between
    b.vecadd(0.5, s.v, 1.0, t)
    other = spectra_of(s, mode, fields=("w",))
    other.sample()
    b.scalar_product(t, t)
    sp.sample()
    second = sp._read(0)
    assert first.tobytes() == second.tobytes()
    assert float(np.max(first)) > 0.0


# ---------------------------------------------------------------- 6. plane mode against the checker
def test_plane_on_the_channel_mesh_against_the_numpy_checker():
    dims = (32, 17, 16)
    rows, _ = plane_rows(channel_fields(dims), dims)
    check_rows(rows, quiet=True)


def test_plane_on_a_periodic_box_against_the_numpy_checker():
    dims = (40, 24, 12)
    rows, _ = plane_rows(periodic_fields(dims, BOX, poisson=False), dims)
    check_rows(rows, quiet=True)


# ---------------------------------------------------------------- 7. the running mean
def test_running_mean_is_the_numpy_recurrence_bit_for_bit():
    from x3d2_amd import make_tgv
    case = make_tgv(16)
    sp = spectra_of(case.solver, "shell")
    samples = []
    for it in range(1, 6):
        case.step(it)
        assert sp.update(it)
        samples.append(sp._read(0))
    assert sp.sample_count == 5
    assert not np.array_equal(samples[0], samples[4])  # (the run evolves)
    want = spectra_ref.running_mean(samples)
    assert sp._read(1).tobytes() == want.tobytes()


# ---------------------------------------------------------------- 8. the driver
def _case(kind, fused):
    from x3d2_amd import make_channel, make_tgv
    if kind == "tgv":
        return make_tgv(32, fused=fused)
    return make_channel((32, 17, 16), fused=fused)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kind", ["tgv", "channel"])
def test_driver_samples_on_schedule_and_leaves_the_run_alone(kind, fused, tmp_path):
    """6 steps, initspec = 2, ispecfreq = 2, ispecout = 4: samples at 2, 4, 6, one file at 4; u, v, w bit-identical to the
    run without spectra; the running mean is that of the spectra of three plain runs stopped at 2, 4 and 6"""
    from x3d2_amd.spectra import Spectra, SpectraConfig, load_spectra
    mode = "shell" if kind == "tgv" else "plane"
    prefix = str(tmp_path / "spectra")
    case = _case(kind, fused)
    assert case.spectra is None
    case.spectra = Spectra(case.solver, SpectraConfig(mode=mode, initspec=2, ispecfreq=2, ispecout=4, spectra_prefix=prefix))
    taken = []
    update = case.spectra.update
    case.spectra.update = lambda it: taken.append(it) if update(it) else None
    case.run(n_iters=6)
    assert taken == [2, 4, 6] and case.spectra.sample_count == 3
    assert case.spectra.files == [prefix + "_000004.npz"] and os.path.exists(prefix + "_000004.npz")
    back = load_spectra(prefix, 4)
    assert back["mode"] == mode and back["sample_count"] == 2 and back["iteration"] == 4
    plain = _case(kind, fused)
    probe = spectra_of(plain.solver, mode)
    snaps = []
    for stop in (2, 4, 6):
        plain.run(n_iters=stop)
        probe.sample()
        snaps.append(probe._read(0))
    sv, pv = case.solver, plain.solver
    for f, g in zip((sv.u, sv.v, sv.w), (pv.u, pv.v, pv.w)):
        assert sv.backend.get_field_data(f).tobytes() == pv.backend.get_field_data(g).tobytes()
    assert case.spectra._read(0).tobytes() == snaps[2].tobytes()
    assert case.spectra._read(1).tobytes() == spectra_ref.running_mean(snaps).tobytes()
    key = "E_u" if mode == "shell" else "Ex_u"
    assert np.array_equal(back["mean"][key], probe.layout.arrays(spectra_ref.running_mean(snaps[:2]), "uvw")[key])


# ---------------------------------------------------------------- 9. deferred execution
@pytest.mark.parametrize("mode", ["shell", "plane"])
def test_sample_behind_queued_blas1_calls_equals_the_eager_result(mode):
    dims = (32, 32, 32)
    out = {}
    for lazy in (False, True):
        s = periodic_fields(dims, lazy=lazy)
        b = s.backend
        set_fields(s, random_arrays(dims, 3))
        sp = spectra_of(s, mode)
        for it in range(1, 4):
            b.vecadd(0.5, s.v, 1.0, s.u)   # recorded, not run, while the deferred layer is on
            b.vecmult(s.w, s.u)
            b.field_scale(s.v, 1.25)
            assert sp.update(it)
        if lazy:
            assert b.lazy_stats()["recorded"] >= 9
        assert s.flushes == 3 and sp.sample_count == 3
        out[lazy] = (sp._read(0), sp._read(1))
    for a, c in zip(out[True], out[False]):
        assert a.tobytes() == c.tobytes() and float(np.max(c)) > 0.0


# ---------------------------------------------------------------- 10. restart
def test_restart_continues_the_mean_exactly(tmp_path):
    from x3d2_amd import make_tgv
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    from x3d2_amd.spectra import Spectra, SpectraConfig
    prefix = str(tmp_path / "checkpoint")
    cases = []
    for restart in (False, True):
        case = make_tgv(32, fused=True)
        case.spectra = Spectra(case.solver, SpectraConfig(mode="shell", initspec=1))
        if restart:
            assert restore(case, prefix + "_000003.npz") == 3 and case.spectra.sample_count == 3
        else:
            case.checkpoints = Checkpoints(case.solver, CheckpointConfig(checkpoint_freq=3, checkpoint_prefix=prefix), case)
        case.run(n_iters=6)
        cases.append(case)
    a, c = cases
    assert a.spectra.sample_count == c.spectra.sample_count == 6
    assert a.spectra._read(1).tobytes() == c.spectra._read(1).tobytes()
    assert float(np.max(a.spectra._read(1))) > 0.0
    z = np.load(prefix + "_000003.npz")
    assert int(z["spectra_sample_count"]) == 3 and str(z["spectra_mode"]) == "shell" and "spectra_E_w" in z.files


# ---------------------------------------------------------------- 11. bad calls
def test_bad_calls_raise_and_change_nothing():
    import ctypes
    from x3d2_amd import Mesh, _lib
    from x3d2_amd.backend import HipBackend
    from x3d2_amd.common import X3dError
    from x3d2_amd.spectra import Spectra, SpectraConfig
    # shell mode on the channel: y is not periodic -- at the Python layer and at the C ABI
    ch = channel_fields((32, 17, 16))
    with pytest.raises(X3dError, match="periodic"):
        Spectra(ch, SpectraConfig(mode="shell", initspec=1))
    b = ch.backend
    h = ctypes.c_void_p()
    L = (ctypes.c_double * 3)(4.0, 2.0, 2.0)
    rc = b.lib.x3d_spectra_create(b.h, ctypes.byref(h), 0, _lib.ints(32, 17, 16), _lib.ints(1, 0, 1), L, 0.0, 3)
    assert rc != 0 and h.value is None and b"periodic" in b.lib.x3d_last_error()
    # a two-slab mesh
    mesh2 = Mesh((32, 16, 32), (1, 1, 2), (TWOPI,) * 3, PER, PER, PER, nrank=0)
    with pytest.raises(X3dError, match="decomposed"):
        Spectra(Fields(HipBackend(mesh2)), SpectraConfig(mode="plane", initspec=1))
    s = periodic_fields((16, 16, 16))
    b = s.backend
    Lp = (ctypes.c_double * 3)(TWOPI, TWOPI, TWOPI)
    rc = b.lib.x3d_spectra_create(b.h, ctypes.byref(h), 1, _lib.ints(16, 16, 32), _lib.ints(1, 1, 1), Lp, 0.0, 3)
    assert rc != 0 and h.value is None and b"decomposed" in b.lib.x3d_last_error()
    # more than 4096 bins
    with pytest.raises(X3dError, match="4096"):
        Spectra(s, SpectraConfig(mode="shell", initspec=1, dk=1e-3))
    rc = b.lib.x3d_spectra_create(b.h, ctypes.byref(h), 0, _lib.ints(16, 16, 16), _lib.ints(1, 1, 1), Lp, 1e-3, 3)
    assert rc != 0 and h.value is None and b"4096" in b.lib.x3d_last_error()
    # a null field, a null object, a slot outside the object, shell mode without the Poisson object: the arrays stay
    set_fields(s, random_arrays((16, 16, 16), 2))
    sp = spectra_of(s, "shell")
    assert sp.update(1)
    before = (sp._read(0).tobytes(), sp._read(1).tobytes())
    ph = s.backend.poisson_fft.h
    for args, word in (((sp.h, ph, None, 0), b"null"), ((None, ph, s.u.ptr, 0), b"null"), ((sp.h, ph, s.u.ptr, 3), b"slot"),
                       ((sp.h, None, s.u.ptr, 0), b"Poisson")):
        rc = b.lib.x3d_spectra_sample(*args)
        assert rc != 0 and word in b.lib.x3d_last_error(), (args, b.lib.x3d_last_error())
    assert b.lib.x3d_spectra_accumulate(sp.h, 0) != 0 and b.lib.x3d_spectra_accumulate(None, 1) != 0
    assert b.lib.x3d_spectra_read(sp.h, 2, np.empty(64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))) != 0
    assert b.lib.x3d_spectra_load(sp.h, None) != 0
    assert (sp._read(0).tobytes(), sp._read(1).tobytes()) == before
    with pytest.raises(X3dError, match="inactive"):
        Spectra(s, SpectraConfig(mode="shell")).spectrum()


# ---------------------------------------------------------------- 12. FP32
def test_shell_and_plane_in_the_fp32_flavour():
    """cases 1 and 6 on 4-byte reals (libx3d2_hip_sp.so), in a process of its own, at the FP32 tolerance; the bins are FP64 in
    both flavours"""
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "spectra_sp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("SPECTRARESULT ")][-1][14:])
    assert res["eps"] == float(np.finfo(np.float32).eps) and res["dtype"] == "float32"
    assert len(res["shell"]) == 3 * len(SHELL_CASES) and len(res["plane"]) == 4 * 3 * (17 + 24)
    check_rows([tuple(r) for r in res["shell"]])
    check_rows([tuple(r) for r in res["plane"]], quiet=True)
