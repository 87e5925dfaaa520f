"""Particles on the device (csrc/particles.hip, x3d2_amd/particles.py) against the numpy restatement (tests/particles_ref.py).

Bounds.  An interpolated value is a sum of 64 (order 4) products of three Lagrange weights and a field value; the weights of a
direction sum to 1 with moduli that add up to at most about 1.6 (4 in three directions), each carries some ten roundings, the
sum another 64: a few 1e-14 of max|f|.  The bound is the project's FP64 parity figure, 1e-12 max|f|.  Updates are compared ONE
at a time, from the device's own previous state, so nothing is amplified over steps: positions to 1e-12 max(L), velocities to
1e-12 max(1, max|u|); F = (a - v) / tau + g carries the errors of a and v divided by tau: 2e-12 max(1, max|u|) / tau.  The
same figures hold on 4-byte fields, which are widened to double before any arithmetic.

 1. interpolation        2. single updates inside real runs        3. the fluid does not notice        4. sorting
 5. walls                6. exact resume                            7. determinism and output           8. errors       9. FP32"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import particles_ref as ref
from test_particles_host import special_points
from x3d2_amd.particles import Particles, ParticlesConfig, load_particles, seed_uniform

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 1e-12
KEYS = ("x", "v", "a", "v_prev", "F", "F_prev")
DP = ctypes.POINTER(ctypes.c_double)


# ---------------------------------------------------------------- helpers (also used by tests/particles_sp_worker.py)
def make_case(name, **kw):
    from x3d2_amd import make_channel, make_cylinder, make_tgv
    if name == "box":  # three different extents and lengths; never stepped (the CG Poisson takes any extents)
        return make_tgv((20, 12, 16), L=(2.0 * np.pi, np.pi, 3.0), poisson="CG", **kw)
    if name == "tgv16":
        return make_tgv(16, **kw)
    if name == "tgv32":
        return make_tgv(32, **kw)
    if name == "channel":
        return make_channel((24, 33, 16), **kw)
    if name == "cylinder":
        return make_cylinder((33, 16, 8), centre=(5.0, 6.0), radius=1.3, **kw)
    raise ValueError(name)


def fields_of(case):
    s = case.solver
    s.flush_grad()
    return [s.backend.get_field_data(f) for f in (s.u, s.v, s.w)]


def set_random_fields(case, seed):
    s = case.solver
    rng = np.random.default_rng(seed)
    nx, ny, nz = (int(n) for n in s.mesh.vert_dims)
    for f in (s.u, s.v, s.w):
        s.backend.set_field_data(f, rng.normal(size=(nz, ny, nx)))
    return fields_of(case)  # (what the device holds: rounded to 4 bytes in the FP32 flavour)


def full_state(p):
    """the whole device state in id order, as particles_ref.update takes it"""
    rows, id_, status, hist = p.raw_state()
    order = np.argsort(id_, kind="stable")
    rows, status = rows[:, order], status[order]
    st = {k: rows[3 * q:3 * q + 3].T.copy() for q, k in enumerate(KEYS[:p.nrow // 3])}
    st["status"] = status.astype(np.int32)
    return st, hist


def state_bits(p):
    st, hist = full_state(p)
    return b"".join(st[k].tobytes() for k in sorted(st)) + bytes([hist])


def check_rows(rows):
    """rows: (name, err, bound); every figure is printed before the first assertion"""
    for name, err, bound in rows:
        print("particles %-44s err %.3e  bound %.3e" % (name, err, bound))
    for name, err, bound in rows:
        assert err <= bound, name


def interpolation_rows(name):
    """test 1 on one mesh: both orders, 1000 random points and the hand-placed ones, and a single point"""
    case = make_case(name)
    s = case.solver
    axes = ref.axes_of(s.mesh)
    fields = set_random_fields(case, 21)
    fmax = max(float(np.max(np.abs(f))) for f in fields)
    pts = np.vstack([seed_uniform(s.mesh, 1000, seed=22), special_points(axes, np.random.default_rng(23))])
    assert pts.shape[0] % 256 != 0 and pts.shape[0] > 256
    rows = []
    for order in (2, 4):
        p = Particles(s, ParticlesConfig(pts[:1], order=order))
        for label, q in (("all", pts), ("one", pts[7:8])):
            got = p.interpolate(q, s.u, s.v, s.w)
            want = ref.interpolate(axes, fields, q, order)
            assert got.shape == want.shape == (q.shape[0], 3) and np.all(np.isfinite(got))
            rows.append(("%s order %d %s (%d points)" % (name, order, label, q.shape[0]),
                         float(np.max(np.abs(got - want))), BOUND * fmax))
        st, _ = full_state(p)  # the primed state of a single particle: a = u(x0), v = a
        want = ref.interpolate(axes, fields, pts[:1], order)
        rows.append(("%s order %d primed n = 1" % (name, order), float(np.max(np.abs(st["a"] - want))), BOUND * fmax))
        assert np.array_equal(st["v"], st["a"])
    return rows


def compare_states(label, got, want, Lmax, umax, tau):
    rows = [(label + " x", float(np.max(np.abs(got["x"] - want["x"]))), BOUND * Lmax)]
    for k in ("v", "a", "v_prev"):
        rows.append((label + " " + k, float(np.max(np.abs(got[k] - want[k]))), BOUND * max(1.0, umax)))
    if tau > 0.0:
        for k in ("F", "F_prev"):
            rows.append((label + " " + k, float(np.max(np.abs(got[k] - want[k]))), 2.0 * BOUND * max(1.0, umax) / tau))
    return rows


def update_rows(name, steps=5, n=2000, order=4, inertial=False, wall="reflect", x0=None, v0=None, tau=None, gravity=None,
                sort_every=0, **case_kw):
    """test 2: `steps` steps of BaseCase.run with particles attached; after every step the device state is compared with
    the restatement's ONE update from the device's previous state.  Returns (rows, per-step info, the case)."""
    case = make_case(name, **case_kw)
    s = case.solver
    axes = ref.axes_of(s.mesh)
    dt = float(s.dt)
    tau = (20.0 * dt if tau is None else tau) if inertial else 0.0
    g = ((0.3, -0.5, 0.2) if gravity is None else tuple(gravity)) if inertial else (0.0, 0.0, 0.0)
    x0 = seed_uniform(s.mesh, n, seed=31) if x0 is None else x0
    cfg = ParticlesConfig(x0, order=order, tau_p=tau, gravity=g, v0=v0, wall=wall, sort_every=sort_every)
    case.particles = p = Particles(s, cfg)
    Lmax = float(np.max(s.mesh.L))
    f0 = fields_of(case)
    umax = max(float(np.max(np.abs(f))) for f in f0)
    prev, hist = full_state(p)
    assert not hist
    rows = compare_states("%s primed" % name, prev, ref.prime(axes, f0, x0, order, tau, g, v0), Lmax, umax, tau)
    infos = []
    for it in range(1, steps + 1):
        case.run(n_iters=it)
        fields = fields_of(case)
        umax = max(float(np.max(np.abs(f))) for f in fields)
        got, hist = full_state(p)
        assert hist and p.iteration == it
        want, info = ref.update(axes, fields, prev, dt, order, it == 1, tau, g, wall)
        rows += compare_states("%s%s step %d" % (name, " inertial" if inertial else "", it), got, want, Lmax, umax, tau)
        info["status_equal"] = bool(np.array_equal(got["status"], want["status"]))
        info["got"] = got
        infos.append(info)
        prev = got
    return rows, infos, case


# ---------------------------------------------------------------- 1. interpolation
@pytest.mark.parametrize("name", ["box", "channel", "cylinder"])
def test_interpolation_against_the_restatement(name):
    check_rows(interpolation_rows(name))


# ---------------------------------------------------------------- 2. single updates inside real runs
@pytest.mark.parametrize("name,kw", [("tgv32", dict(fused=True)), ("tgv32", dict(fused=False)), ("channel", dict(fused=True)),
                                     ("cylinder", dict(time_intg="AB3"))])
@pytest.mark.parametrize("inertial", [False, True])
def test_single_updates_inside_real_runs(name, kw, inertial):
    rows, infos, _ = update_rows(name, inertial=inertial, **kw)
    check_rows(rows)
    assert all(i["status_equal"] for i in infos)


def test_order_2_updates_on_the_channel():
    rows, infos, _ = update_rows("channel", steps=3, order=2, fused=True)
    check_rows(rows)


def test_initpart_3_rests_primes_after_step_2_and_advances_from_step_3():
    """before initpart the particles rest; after step initpart - 1 the state is primed from u^2 (that step is completed like
    the ones that follow: reads_state is true there); step 3 is a first advance, steps 4 and 5 carry the history"""
    case = make_case("channel", fused=True)
    s = case.solver
    axes = ref.axes_of(s.mesh)
    dt = float(s.dt)
    tau, g = 20.0 * dt, (0.3, -0.5, 0.2)
    x0 = seed_uniform(s.mesh, 1000, seed=41)
    case.particles = p = Particles(s, ParticlesConfig(x0, tau_p=tau, gravity=g, initpart=3, sort_every=0))
    assert [p.reads_state(it) for it in range(1, 6)] == [False, True, True, True, True]
    Lmax = float(np.max(s.mesh.L))
    at0 = state_bits(p)
    case.run(n_iters=1)
    assert state_bits(p) == at0 and p.iteration == 1  # resting: nothing moved, nothing sampled
    case.run(n_iters=2)
    fields = fields_of(case)
    umax = max(float(np.max(np.abs(f))) for f in fields)
    prev, hist = full_state(p)
    assert not hist and p.iteration == 2 and np.array_equal(prev["x"], x0)
    rows = compare_states("initpart 3, primed after step 2", prev, ref.prime(axes, fields, x0, 4, tau, g), Lmax, umax, tau)
    for it in (3, 4, 5):
        case.run(n_iters=it)
        fields = fields_of(case)
        umax = max(float(np.max(np.abs(f))) for f in fields)
        got, hist = full_state(p)
        assert hist and p.iteration == it
        want, _ = ref.update(axes, fields, prev, dt, 4, it == 3, tau, g)
        rows += compare_states("initpart 3, step %d" % it, got, want, Lmax, umax, tau)
        assert np.max(np.abs(got["x"] - prev["x"])) > 1e-4  # (they do move)
        prev = got
    check_rows(rows)
    # ... and the fluid is the one of a run without particles
    plain = make_case("channel", fused=True)
    for it in range(1, 6):
        plain.step(it, more=False)
    for a, c in zip(fields_of(case), fields_of(plain)):
        assert a.tobytes() == c.tobytes()


def test_a_refused_advance_leaves_the_count_with_the_state():
    from x3d2_amd.common import X3dError
    case = make_case("channel", fused=True)
    s = case.solver
    p = Particles(s, ParticlesConfig(seed_uniform(s.mesh, 100, seed=42), tau_p=20.0 * float(s.dt)))
    case.step(1)
    before, dt = state_bits(p), s.dt
    s.dt = 100.0 * dt  # tau_p < 2 dt now
    with pytest.raises(X3dError, match="tau < 2 dt"):
        p.update(1)
    assert p.iteration == 0 and state_bits(p) == before
    s.dt = dt
    assert p.update(1) and p.iteration == 1 and state_bits(p) != before  # the real error was reported, the step is still due


# ---------------------------------------------------------------- 3. the fluid does not notice
def test_the_fluid_does_not_notice():
    with_p = make_case("tgv32", fused=True)
    s = with_p.solver
    with_p.particles = Particles(s, ParticlesConfig(seed_uniform(s.mesh, 500, seed=3), sort_every=2))
    with_p.run(n_iters=5)
    plain = make_case("tgv32", fused=True)
    for it in range(1, 6):
        plain.step(it, more=False)
    for a, c in zip(fields_of(with_p), fields_of(plain)):
        assert a.tobytes() == c.tobytes()


# ---------------------------------------------------------------- 4. sorting
def test_sorting_changes_no_value():
    bits, cases = [], []
    for m in (0, 1, 2):
        case = make_case("tgv16", fused=True)
        s = case.solver
        case.particles = Particles(s, ParticlesConfig(seed_uniform(s.mesh, 3000, seed=4), sort_every=m))
        case.run(n_iters=6)
        bits.append(state_bits(case.particles))
        cases.append(case)
    assert bits[0] == bits[1] == bits[2]
    axes = ref.axes_of(cases[0].solver.mesh)
    moved = []
    for case in cases[1:]:  # (both sorted after step 6)
        rows, id_, status, _ = case.particles.raw_state()
        keys = ref.cell_keys(axes, rows[0:3].T)
        assert np.all(np.diff(keys) >= 0) and len(set(keys.tolist())) > 100
        assert sorted(id_.tolist()) == list(range(3000)) and np.all(status == 1)
        moved.append(not np.array_equal(id_, np.arange(3000)))
    assert all(moved)
    rows, id_, _, _ = cases[0].particles.raw_state()
    assert np.array_equal(id_, np.arange(3000))  # never sorted: the order it was seeded in


# ---------------------------------------------------------------- 5. walls
def wall_seed(mesh, n=400):
    rng = np.random.default_rng(5)
    x0 = seed_uniform(mesh, n, seed=6)
    x0[:, 1] = 0.005 + 0.025 * rng.random(n)
    return x0, np.tile(np.array([0.0, -1.0, 0.0]), (n, 1))


def test_reflecting_wall():
    case0 = make_case("channel", fused=True)
    assert float(case0.solver.dt) == 5e-3
    x0, v0 = wall_seed(case0.solver.mesh)
    del case0
    rows, infos, case = update_rows("channel", steps=12, inertial=True, wall="reflect", x0=x0, v0=v0, tau=0.1,
                                    gravity=(0.0, 0.0, 0.0), fused=True)
    reflected = np.zeros(x0.shape[0], dtype=bool)
    for info in infos:
        reflected |= info["reflected"]
        assert not info["clamped"].any() and not info["absorbed"].any() and info["status_equal"]
    print("reflected in the restatement: %d of %d" % (int(reflected.sum()), reflected.size))
    assert reflected.sum() * 2 >= reflected.size  # a condition on this test's own inputs
    check_rows(rows)
    axes = ref.axes_of(case.solver.mesh)
    for info in infos:
        y = info["got"]["x"][:, 1]
        assert y.min() >= axes[1].lo and y.max() <= axes[1].hi
    assert np.all(infos[-1]["got"]["status"] == 1)


def test_absorbing_wall():
    case0 = make_case("channel", fused=True)
    x0, v0 = wall_seed(case0.solver.mesh)
    del case0
    rows, infos, case = update_rows("channel", steps=12, inertial=True, wall="absorb", x0=x0, v0=v0, tau=0.1,
                                    gravity=(0.0, 0.0, 0.0), fused=True)
    check_rows(rows)
    absorbed = np.zeros(x0.shape[0], dtype=bool)
    frozen = {}
    for step, info in enumerate(infos):
        assert info["status_equal"]
        for q in np.flatnonzero(info["absorbed"]):
            frozen[int(q)] = {k: info["got"][k][q].copy() for k in KEYS}
        absorbed |= info["absorbed"]
        for q, kept in frozen.items():  # frozen from then on: every row keeps its bits
            for k in KEYS:
                assert np.array_equal(info["got"][k][q], kept[k]), (step, q, k)
    assert absorbed.sum() * 2 >= absorbed.size
    last = infos[-1]["got"]
    assert np.array_equal(last["status"] == 0, absorbed) and np.all(last["x"][absorbed, 1] == ref.axes_of(case.solver.mesh)[1].lo)
    st = case.particles.state()
    assert np.array_equal(st["alive"] == 0, absorbed)


# ---------------------------------------------------------------- 6. exact resume
@pytest.mark.parametrize("name,inertial", [("tgv16", False), ("channel", True)])
def test_exact_resume(name, inertial, tmp_path):
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    from x3d2_amd.common import X3dError
    prefix = str(tmp_path / "ck")

    def build():
        case = make_case(name, fused=True)
        s = case.solver
        kw = dict(tau_p=20.0 * float(s.dt), gravity=(0.1, -0.4, 0.0)) if inertial else dict(sort_every=2)
        case.particles = Particles(s, ParticlesConfig(seed_uniform(s.mesh, 1500, seed=7), **kw))
        return case

    whole = build()
    whole.run(n_iters=6)
    first = build()
    first.checkpoints = Checkpoints(first.solver, CheckpointConfig(checkpoint_freq=3, checkpoint_prefix=prefix), first)
    first.run(n_iters=3)
    second = build()
    assert restore(second, prefix + "_000003.npz") == 3 and second.particles.iteration == 3
    second.run(n_iters=6)
    assert state_bits(second.particles) == state_bits(whole.particles)
    for a, c in zip(fields_of(second), fields_of(whole)):
        assert a.tobytes() == c.tobytes()
    if not inertial:
        # a checkpoint written without particles is refused by a run that has them, and so is another n
        bare = make_case(name, fused=True)
        bare.checkpoints = Checkpoints(bare.solver, CheckpointConfig(checkpoint_freq=3, checkpoint_prefix=prefix + "_bare"), bare)
        bare.run(n_iters=3)
        third = build()
        before = state_bits(third.particles)
        with pytest.raises(X3dError, match="holds none"):
            restore(third, prefix + "_bare_000003.npz")
        other = make_case(name, fused=True)
        other.particles = Particles(other.solver, ParticlesConfig(seed_uniform(other.solver.mesh, 1400, seed=7)))
        with pytest.raises(X3dError, match="particles_n"):
            restore(other, prefix + "_000003.npz")
        assert state_bits(third.particles) == before and third.solver.current_iter == 0 and not third.restarted


# ---------------------------------------------------------------- 7. determinism and output
def test_determinism_output_and_no_host_wait(tmp_path):
    runs = []
    for k in range(2):
        case = make_case("tgv16", fused=True)
        s, b = case.solver, case.solver.backend
        prefix = str(tmp_path / ("p%d" % k))
        cfg = ParticlesConfig(seed_uniform(s.mesh, 1000, seed=8), ipartout=2, prefix=prefix, sort_every=3)
        case.particles = p = Particles(s, cfg)
        case.run(n_iters=2)
        at2 = p.state()
        for it in (3, 4):  # by hand: the calls BaseCase.run makes, with the host waits of write counted
            case.step(it)
            s.current_iter = it
            assert p.update(it)
            n0 = b.sync_count()
            assert p.write(it) == (it == 4)
            assert b.sync_count() == n0  # no host wait
            p.poll()
        at4 = p.state()
        p.finalise()
        assert p.sync_count == 0 and p.files == [prefix + "_000002.npz", prefix + "_000004.npz"]
        for it, st in ((2, at2), (4, at4)):
            z = load_particles(prefix, it)
            assert sorted(z) == sorted(st) and int(z["iteration"]) == it and float(z["time"]) == it * float(s.dt)
            for key in st:
                assert np.array_equal(z[key], st[key]), key
        runs.append(state_bits(p))
    assert runs[0] == runs[1]


# ---------------------------------------------------------------- 8. errors
def raw_create(b, mesh, x0, order=4, n=None, tau=0.0, v0=None, null=None):
    from x3d2_amd import _lib
    from x3d2_amd.diagnostics import global_vert_coords
    coords = [np.ascontiguousarray(global_vert_coords(mesh, d), dtype=np.float64) for d in range(3)]
    prm = _lib.ParticlesParams()
    prm.n, prm.order, prm.wall, prm.tau = (int(x0.shape[0]) if n is None else n), order, 0, tau
    for d in range(3):
        prm.g[d], prm.periodic[d], prm.uniform[d], prm.L[d] = 0.0, int(bool(mesh.periodic_BC[d])), int(not mesh.stretched[d]), float(mesh.L[d])
        prm.coords[d] = coords[d].ctypes.data_as(DP)
    xs = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).T)
    vs = np.ascontiguousarray(np.asarray(v0, dtype=np.float64).T) if v0 is not None else None
    h = ctypes.c_void_p()
    rc = b.lib.x3d_particles_create(b.h if null != "b" else None, ctypes.byref(prm) if null != "prm" else None,
                                    xs.ctypes.data_as(DP) if null != "x0" else None,
                                    vs.ctypes.data_as(DP) if vs is not None else None, ctypes.byref(h) if null != "out" else None)
    if rc == 0:
        b.lib.x3d_particles_destroy(h)
    return rc


def test_every_refusal_raises_and_changes_nothing():
    from x3d2_amd import _lib
    from x3d2_amd.common import X3dError
    case = make_case("channel", fused=True)
    s, b = case.solver, case.solver.backend
    mesh = s.mesh
    x0 = seed_uniform(mesh, 300, seed=9)
    case.particles = p = Particles(s, ParticlesConfig(x0, tau_p=0.1, gravity=(0.0, -1.0, 0.0)))
    case.run(n_iters=1)
    before_state, before_fields = state_bits(p), [f.tobytes() for f in fields_of(case)]
    # creation
    assert raw_create(b, mesh, x0) == 0
    for null in ("b", "prm", "x0", "out"):
        assert raw_create(b, mesh, x0, null=null) != 0
    for n in (0, -1, (1 << 24) + 1):
        assert raw_create(b, mesh, x0, n=n) != 0
    for order in (0, 1, 3, 5):
        assert raw_create(b, mesh, x0, order=order) != 0
    for bad in (np.nan, np.inf, -np.inf):
        x = x0.copy()
        x[17, 0] = bad
        assert raw_create(b, mesh, x) != 0
        v = np.zeros_like(x0)
        v[5, 2] = bad
        assert raw_create(b, mesh, x0, tau=0.1, v0=v) != 0
    for y in (-1e-9, 2.0 + 1e-9):
        x = x0.copy()
        x[3, 1] = y
        assert raw_create(b, mesh, x) != 0
    x = x0.copy()
    x[:, 0] += 3.0 * 4.0  # (a periodic coordinate may lie anywhere)
    assert raw_create(b, mesh, x) == 0
    for kw in (dict(tau_p=0.009), dict(tau_p=1e-6)):  # 0 < tau_p < 2 dt
        with pytest.raises(X3dError, match="2 dt"):
            Particles(s, ParticlesConfig(x0, **kw))
    with pytest.raises(X3dError):
        Particles(s, ParticlesConfig(np.array([[0.0, 2.5, 0.0]])))
    # the launches
    dims = b._dims(0)
    args = (s.u.ptr, s.v.ptr, s.w.ptr)
    lib = b.lib
    other = make_case("channel", fused=True).solver.backend
    big = (ctypes.c_int * 3)()
    assert lib.x3d_padded_dims(b.h, big) == 0
    big[0] += 1
    calls = [lambda: lib.x3d_particles_advance(None, p.h, *args, dims, 5e-3),
             lambda: lib.x3d_particles_advance(b.h, None, *args, dims, 5e-3),
             lambda: lib.x3d_particles_advance(b.h, p.h, None, args[1], args[2], dims, 5e-3),
             lambda: lib.x3d_particles_advance(b.h, p.h, *args, None, 5e-3),
             lambda: lib.x3d_particles_advance(other.h, p.h, *args, dims, 5e-3),
             lambda: lib.x3d_particles_advance(b.h, p.h, *args, big, 5e-3),
             lambda: lib.x3d_particles_advance(b.h, p.h, *args, _lib.ints(24, 33, 15), 5e-3),
             lambda: lib.x3d_particles_advance(b.h, p.h, *args, dims, float("nan")),
             lambda: lib.x3d_particles_advance(b.h, p.h, *args, dims, 0.5),  # tau_p < 2 dt
             lambda: lib.x3d_particles_prime(other.h, p.h, *args, dims),
             lambda: lib.x3d_particles_sort(other.h, p.h),
             lambda: lib.x3d_particles_sort(b.h, None),
             lambda: lib.x3d_particles_interpolate(b.h, p.h, *args, dims, None, 4, None),
             lambda: lib.x3d_particles_pack(b.h, p.h, None, 1 << 30),
             lambda: lib.x3d_particles_pack(other.h, p.h, None, 1 << 30)]
    for call in calls:
        with pytest.raises(X3dError):
            _lib.check(call())
    for bad in (np.full((2, 3), np.nan), np.array([[0.0, -0.5, 0.0]]), np.zeros((0, 3))):
        with pytest.raises(X3dError):
            p.interpolate(bad, s.u, s.v, s.w)
    with pytest.raises(X3dError, match="every step"):
        p.update(3)  # the state is at 1: a skipped step is an error
    with pytest.raises(X3dError, match="every step"):
        p.update(1)
    rows, id_, status, hist = p.raw_state()
    bad_rows = rows.copy()
    bad_rows[4, 0] = np.inf
    for r, i in ((bad_rows, id_), (rows, np.zeros_like(id_))):
        assert lib.x3d_particles_upload(b.h, p.h, r.ctypes.data_as(DP), i.ctypes.data_as(_lib.c_int_p),
                                        status.ctypes.data_as(_lib.c_int_p), 1) != 0
    assert state_bits(p) == before_state
    assert [f.tobytes() for f in fields_of(case)] == before_fields
    # a decomposed mesh
    from x3d2_amd import Mesh
    from types import SimpleNamespace
    split = Mesh((16, 16, 16), (1, 1, 2), (1.0,) * 3, ("periodic",) * 2, ("periodic",) * 2, ("periodic",) * 2)
    with pytest.raises(X3dError, match="multi-rank particles are not built"):
        Particles(SimpleNamespace(backend=b, mesh=split, dt=1e-3, current_iter=0), ParticlesConfig(np.zeros((1, 3))))


# ---------------------------------------------------------------- 9. FP32
def test_fp32_flavour():
    """tests 1 and 2 on the channel on 4-byte fields (libx3d2_hip_sp.so), in a process of its own; the restatement takes
    the float32 fields widened to double and the same 1e-12 bounds hold: all particle arithmetic is FP64"""
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "particles_sp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("PARTICLESRESULT ")][-1][16:])
    assert res["dtype"] == "float32" and len(res["interpolation"]) == 6 and len(res["tracers"]) > 20 and len(res["inertial"]) > 30
    check_rows([tuple(row) for row in res["interpolation"] + res["tracers"] + res["inertial"]])
