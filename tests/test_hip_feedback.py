"""Two-way coupled particles on the device (csrc/particles.hip x3d_particles_feedback_*, x3d2_amd/particles.py Feedback,
BaseCase.substep) against the numpy restatement tests/feedback_ref.py (pinned on the host by tests/test_feedback_host.py).

Bounds:
  field     f of Feedback.field() against the restatement on the same state, 1e-12 max|f| (the bound tests/test_hip_forcing.py
            holds its blocks to): a vertex value is a sum of at most 8 records of at most 300 FP64 terms each, in one order.
            FP32 flavour: the arithmetic is FP64 there too, a vertex takes at most eight rounded adds: 8 * 2^-24 max(|before| +
            sum |contributions|).
  sums      sum f V = -sum D_p, 1e-12 of max |sum D_p| (the drag has a mean in these states, so that the sum is no accident).
  add       blocks of random values: after = before + f, FP64 1e-12 max(max|f|, max|before|) (one rounding of the sum), FP32 as
            above;
            the row padding, poisoned with 1e30, keeps its bits.
  bits      two builds, and the same particles in id order, in reversed slot order and after Particles.sort(): the same bits.
  steps     1e-10 max(max|ref|, 1) per field, the project's step tolerance (FP32: 2e-5); deferred against call-by-call 1e-12.
Every block is filled with 1e30 before its data are set."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import feedback_ref as R
import particles_ref as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TWOPI = 2.0 * np.pi
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int)
TAU, MASS = 0.05, 1e-3
HUGE = 1e300


# ---------------------------------------------------------------- helpers (also used by tests/feedback_sp_worker.py)
def single():
    from x3d2_amd import _lib
    return _lib.SINGLE


def make_solver(name, dims=None):
    from x3d2_amd import make_channel, make_tgv
    if name == "box":
        return make_tgv(dims or (16, 12, 10), L=(TWOPI, np.pi, 3.0), poisson="CG").solver
    return make_channel(dims or (16, 17, 8), poisson="CG").solver


def whole(f):
    import torch
    torch.cuda.synchronize()
    return f.data.cpu().numpy().copy()


def inside_mask(b, dims, like):
    nxp, nyp, nzp = (int(v) for v in b.padded_dims)
    inside = np.zeros(like.shape, dtype=bool)
    inside[:nxp * nyp * nzp].reshape(nzp, nyp, nxp)[:dims[2], :dims[1], :dims[0]] = True
    return inside


def inside_cell(axes, cell, rng, m):
    """m points strictly inside the cell (i, j, k)"""
    x = np.empty((m, 3))
    for d, ax in enumerate(axes):
        lo = ax.c[cell[d]]
        hi = ax.c[cell[d] + 1] if cell[d] + 1 < ax.n else ax.L
        x[:, d] = lo + (hi - lo) * (0.05 + 0.9 * rng.random(m))
    return x


def box_state(mesh, n=3000, seed=21):
    """the state of the box tests: 300 particles in the cell (5, 4, 3), one in the cell after it in key order, every seam cell
    occupied, 50 particles exactly on vertices, 50 particles that are not alive (status 0 and 2, a and v huge), the rest
    uniform -- and none of those in the two cells whose counts are prescribed"""
    from x3d2_amd.particles import seed_uniform
    axes = P.axes_of(mesh)
    nx, ny, nz = (ax.n for ax in axes)
    rng = np.random.default_rng(seed)
    crowd, after = (5, 4, 3), (6, 4, 3)
    parts = [inside_cell(axes, crowd, rng, 300), inside_cell(axes, after, rng, 1)]
    seam = [(i, j, k) for k in range(nz) for j in range(ny) for i in range(nx) if i == nx - 1 or j == ny - 1 or k == nz - 1]
    parts += [inside_cell(axes, c, rng, 1) for c in seam]
    banned = [(c[2] * ny + c[1]) * nx + c[0] for c in (crowd, after)]
    iv = rng.integers(0, [nx, ny, nz], size=(80, 3))
    iv = iv[~np.isin((iv[:, 2] * ny + iv[:, 1]) * nx + iv[:, 0], banned)][:50]
    parts.append(np.stack([axes[d].c[iv[:, d]] for d in range(3)], axis=1))  # exactly on vertices
    fixed = np.concatenate(parts)
    rest = seed_uniform(mesh, 4 * n, seed=seed)
    rest = rest[~np.isin(P.cell_keys(axes, rest), banned)][:n - fixed.shape[0]]
    x = np.concatenate([fixed, rest])
    perm = rng.permutation(n)  # (the ids carry no order of the cells)
    x = x[perm]
    st = {"x": x, "v": rng.standard_normal((n, 3)), "a": 1.0 + rng.standard_normal((n, 3)), "status": np.ones(n, dtype=np.int32)}
    key = P.cell_keys(axes, x)
    dead = np.nonzero(perm >= fixed.shape[0])[0][:50]  # (of the uniform ones: every prescribed particle stays alive)
    st["status"][dead] = np.arange(50) % 2 * 2  # 0 and 2
    st["v"][dead], st["a"][dead] = HUGE, -HUGE
    # what the test relies on
    alive = st["status"] == 1
    counts = np.bincount(key[alive], minlength=nx * ny * nz)
    assert counts[banned[0]] == 300 and counts[banned[1]] == 1 and banned[1] == banned[0] + 1
    assert all(counts[(c[2] * ny + c[1]) * nx + c[0]] >= 1 for c in seam)
    assert set(st["status"][dead]) == {0, 2} and alive.sum() == n - 50
    return st


def channel_state(mesh, n=600, seed=22):
    """particles in the cells next to both walls (j = 0 and j = 15) and one exactly on the top vertex"""
    from x3d2_amd.particles import seed_uniform
    axes = P.axes_of(mesh)
    rng = np.random.default_rng(seed)
    x = seed_uniform(mesh, n, seed=seed)
    cy = axes[1].c
    x[:60, 1] = cy[0] + (cy[1] - cy[0]) * rng.random(60)
    x[60:120, 1] = cy[-2] + (cy[-1] - cy[-2]) * rng.random(60)
    x[120, 1] = cy[-1]
    x[121, 1] = cy[0]
    st = {"x": x, "v": rng.standard_normal((n, 3)), "a": 1.0 + rng.standard_normal((n, 3)), "status": np.ones(n, dtype=np.int32)}
    st["status"][200:210] = np.arange(10) % 2 * 2
    st["v"][200:210], st["a"][200:210] = -HUGE, HUGE
    j = P.cell(axes[1], x[:, 1])
    assert np.sum(j == 0) >= 60 and np.sum(j == axes[1].n - 2) >= 61 and j.max() == axes[1].n - 2
    return st


def make_particles(s, st, **kw):
    from x3d2_amd.particles import Particles, ParticlesConfig
    args = dict(tau_p=TAU, two_way=True, mass=MASS, sort_every=0)
    args.update(kw)
    return Particles(s, ParticlesConfig(st["x"], **args))


def upload(p, st, slots=None):
    """the state st (id order) into the device slots: slot t holds particle slots[t]; then the records are built"""
    n = p.n
    slots = np.arange(n) if slots is None else np.asarray(slots)
    rows = np.zeros((p.nrow, n))
    for q, key in enumerate(("x", "v", "a")):
        rows[3 * q:3 * q + 3] = st[key].T
    rows = np.ascontiguousarray(rows[:, slots])
    ids = np.ascontiguousarray(slots, dtype=np.int32)
    status = np.ascontiguousarray(st["status"][slots], dtype=np.int32)
    b = p.solver.backend
    rc = b.lib.x3d_particles_upload(b.h, p.h, rows.ctypes.data_as(DP), ids.ctypes.data_as(IP), status.ctypes.data_as(IP), 0)
    assert rc == 0, b.lib.x3d_last_error()
    p.feedback.build()


def field_of(p):
    """(the three [nz, ny, nx] arrays of Feedback.field() in float64, the bytes of the three whole blocks)"""
    b = p.solver.backend
    blocks = p.feedback.field()
    out = [b.get_field_data(f).astype(np.float64) for f in blocks]
    bits = b"".join(whole(f).tobytes() for f in blocks)
    for f in blocks:
        b.allocator.release_block(f)
    return out, bits


def field_bound(axes, st, fmax, before=0.0):
    if single():
        return 8.0 * 2.0 ** -24 * max(float(np.max(before + c)) for c in R.contributions(axes, st, MASS, TAU))
    return 1e-12 * fmax


@functools.lru_cache(maxsize=None)
def kernel_reference(name):
    """(solver, state, reference field): computed once, never changed"""
    s = make_solver(name)
    st = box_state(s.mesh) if name == "box" else channel_state(s.mesh)
    return s, st, R.field(P.axes_of(s.mesh), st, MASS, TAU)


def check_field(name):
    """Feedback.field() of the hand-made state against the restatement; conservation; the dead contribute nothing"""
    s, st, ref = kernel_reference(name)
    axes = P.axes_of(s.mesh)
    p = make_particles(s, st)
    upload(p, st)
    got, bits = field_of(p)
    fmax = max(float(np.max(np.abs(f))) for f in ref)
    bound = field_bound(axes, st, fmax)
    worst = 0.0
    for c in range(3):
        err = float(np.max(np.abs(got[c] - ref[c])))
        worst = max(worst, err / bound)
        print("%s: f[%d] off by %.3e (bound %.3e, max|f| %.3e)" % (name, c, err, bound, fmax))
        assert err <= bound, c
    total = -R.total_drag(st, MASS, TAU)
    scale = float(np.max(np.abs(total)))
    err = float(np.max(np.abs(R.integral(axes, got) - total))) / scale
    print("%s: sum f V against -sum D: %.3e relative" % (name, err))
    vol = 1.0 / R.inverse_volumes(axes)
    # (FP32: f is stored in 4 bytes after at most eight rounded adds; the sums themselves are FP64 in both flavours)
    sums_bound = 8.0 * 2.0 ** -24 * sum(float(np.sum(c * vol)) for c in R.contributions(axes, st, MASS, TAU)) / scale if single() else 1e-12
    assert err <= sums_bound
    # the records are the restatement's, cell by cell, and the colour lists are ordered
    counts, cells, rec = p.feedback.records()
    rcells, rrec = R.records(axes, st, MASS, TAU)
    order = np.argsort(cells, kind="stable")
    assert np.array_equal(cells[order], rcells) and counts[8] == rcells.size and counts[0] == 0
    assert np.max(np.abs(rec[order] - rrec)) <= 1e-12 * float(np.max(np.abs(rrec)))
    col = R.colour_of(axes, cells.astype(np.int64))
    for c in range(8):
        sl = slice(counts[c], counts[c + 1])
        assert np.all(col[sl] == c) and np.all(np.diff(cells[sl].astype(np.int64)) > 0), c
    # other values in the particles that are not alive: not one bit changes
    st2 = {k: v.copy() for k, v in st.items()}
    dead = st2["status"] != 1
    st2["v"][dead], st2["a"][dead] = 3.0, -7e200
    upload(p, st2)
    assert field_of(p)[1] == bits
    return worst


def check_add(name="box"):
    """add() on poisoned blocks of random values: before + f, padding untouched"""
    from x3d2_amd.common import DIR_X, VERT
    s, st, ref = kernel_reference(name)
    b, axes = s.backend, P.axes_of(s.mesh)
    dims = tuple(ax.n for ax in axes)
    p = make_particles(s, st)
    upload(p, st)
    rng = np.random.default_rng(31)
    arrays = [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(3)]
    blocks = []
    for a in arrays:
        f = b.allocator.get_block(DIR_X, VERT)
        f.fill(1e30)
        b.set_field_data(f, a)
        blocks.append(f)
    before = [whole(f) for f in blocks]
    inside = inside_mask(b, dims, before[0])
    p.feedback.add(*blocks)
    after = [whole(f) for f in blocks]
    fmax = max(float(np.max(np.abs(f))) for f in ref)
    amax = max(float(np.max(np.abs(a))) for a in arrays)
    worst = 0.0
    contrib = R.contributions(axes, st, MASS, TAU)
    for c in range(3):
        assert before[c][~inside].tobytes() == after[c][~inside].tobytes(), "padding of block %d changed" % c
        got = b.get_field_data(blocks[c]).astype(np.float64)
        want = arrays[c] + ref[c]
        bound = 8.0 * 2.0 ** -24 * float(np.max(np.abs(arrays[c]) + contrib[c])) if single() else 1e-12 * max(fmax, amax)
        err = float(np.max(np.abs(got - want)))
        worst = max(worst, err / bound)
        print("add %s: block %d off by %.3e (bound %.3e)" % (name, c, err, bound))
        assert err <= bound, c
    for f in blocks:
        b.allocator.release_block(f)
    return worst


# ---------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("name", ["box", "channel"])
def test_field_against_the_restatement(name):
    check_field(name)


@pytest.mark.parametrize("name", ["box", "channel"])
def test_add_on_random_blocks(name):
    check_add(name)


def test_bit_identity_of_builds_and_slot_orders():
    s, st, _ = kernel_reference("box")
    n = st["status"].size
    p = make_particles(s, st)
    upload(p, st)
    first = p.feedback.records()
    bits = field_of(p)[1]
    p.feedback.build()
    again = p.feedback.records()
    assert all(a.tobytes() == c.tobytes() for a, c in zip(first, again))
    assert field_of(p)[1] == bits
    upload(p, st, slots=np.arange(n)[::-1])
    assert field_of(p)[1] == bits, "reversed slot order"
    upload(p, st, slots=np.random.default_rng(4).permutation(n))
    assert field_of(p)[1] == bits, "shuffled slot order"
    p.sort()
    p.feedback.build()
    assert field_of(p)[1] == bits, "after Particles.sort()"
    assert all(a.tobytes() == c.tobytes() for a, c in zip(first, p.feedback.records()))


# ---------------------------------------------------------------- 2. steps
HIT_DIMS, HIT_L = (32, 32, 32), (TWOPI, TWOPI, TWOPI)
HIT_KW = dict(Re=400.0, dt=2e-3, k0=2.0, ke0=0.5, seed=4)
NPART = 4096


def step_tol():
    return 2e-5 if single() else 1e-10


def hit_particles():
    """(x0, v0, mass): 4096 inertial particles that start with a slip, at a mass loading of 0.5"""
    rng = np.random.default_rng(17)
    x0 = rng.random((NPART, 3)) * TWOPI
    v0 = 0.5 * rng.standard_normal((NPART, 3))
    return x0, v0, 0.5 * TWOPI ** 3 / NPART


def make_case(time_intg="RK3", fused=True, two_way=True, particles=True, **kw):
    from x3d2_amd import make_hit
    from x3d2_amd.particles import Particles, ParticlesConfig
    case = make_hit(HIT_DIMS, L=HIT_L, time_intg=time_intg, fused=fused, **dict(HIT_KW, **kw))
    if particles:
        x0, v0, mass = hit_particles()
        extra = dict(two_way=True, mass=mass) if two_way else {}
        case.particles = Particles(case.solver, ParticlesConfig(x0, tau_p=TAU, v0=v0, sort_every=2, **extra))
    return case


def advance(case, it):
    """what BaseCase.run does with a step"""
    case.step(it)
    case.solver.current_iter = it
    if case.particles is not None:
        case.particles.update(it)


def fields_of(case):
    s = case.solver
    s.flush_grad()
    return [s.backend.get_field_data(f).astype(np.float64) for f in (s.u, s.v, s.w)]


@functools.lru_cache(maxsize=None)
def hit_reference(time_intg, nsteps=2):
    x0, v0, mass = hit_particles()
    r = R.FeedbackHit(HIT_DIMS, HIT_L, x0, TAU, mass, time_intg=time_intg, v0=v0, **HIT_KW)
    out = [r.fields()]
    for _ in range(nsteps):
        r.step()
        out.append(r.fields())
    return out


def assert_step(got, ref, what, tol=None):
    tol = step_tol() if tol is None else tol
    worst = 0.0
    for x, y, nm in zip(got, ref, "uvw"):
        err = float(np.max(np.abs(x - y))) / max(float(np.max(np.abs(y))), 1.0)
        worst = max(worst, err)
        print("%s: %s off by %.3e" % (what, nm, err))
        assert err < tol, "%s: %s off by %.3e" % (what, nm, err)
    return worst


def check_steps(time_intg, fused):
    ref = hit_reference(time_intg)
    case = make_case(time_intg, fused)
    assert case.solver.particle_feedback is case.particles.feedback
    worst = 0.0
    for it in (1, 2):
        advance(case, it)
        worst = max(worst, assert_step(fields_of(case), ref[it], "step %d (%s, fused=%s)" % (it, time_intg, fused)))
    return worst


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op"])
@pytest.mark.parametrize("time_intg", ["RK3", "AB3"])
def test_two_coupled_steps_against_the_composed_restatement(time_intg, fused):
    check_steps(time_intg, fused)


def test_deferred_execution_equals_call_by_call():
    out = {}
    for lazy in (False, True):
        case = make_case("RK3", fused=False, lazy=lazy)
        for it in (1, 2):
            advance(case, it)
        out[lazy] = fields_of(case)
    for x, y, nm in zip(out[True], out[False], "uvw"):
        err = float(np.max(np.abs(x - y))) / max(float(np.max(np.abs(y))), 1.0)
        print("deferred against call by call, %s: %.3e" % (nm, err))
        assert err <= 1e-12, nm
    assert_step(out[True], hit_reference("RK3")[2], "deferred, step 2")


def test_one_way_is_the_parents_run_and_two_way_changes_it():
    runs = {}
    for key, kw in (("none", dict(particles=False)), ("one", dict(two_way=False)), ("two", dict(two_way=True))):
        case = make_case("RK3", True, **kw)
        assert (case.solver.particle_feedback is not None) == (key == "two")
        for it in (1, 2):
            advance(case, it)
        runs[key] = fields_of(case)
    for x, y, nm in zip(runs["one"], runs["none"], "uvw"):
        assert x.tobytes() == y.tobytes(), nm
    change = max(float(np.max(np.abs(x - y))) for x, y in zip(runs["two"], runs["none"]))
    print("two-way against one-way after two steps: max change %.3e" % change)
    assert change > 1e-6


def test_resting_particles_add_nothing_before_initpart():
    from x3d2_amd.particles import Particles, ParticlesConfig
    # (op-granular: the sub-step has one branch there, so that the two runs can be compared bit by bit)
    plain = make_case("RK3", False, particles=False)
    case = make_case("RK3", False, particles=False)
    x0, v0, mass = hit_particles()
    case.particles = Particles(case.solver, ParticlesConfig(x0, tau_p=TAU, v0=v0, initpart=3, two_way=True, mass=mass))
    assert not case.particles.feedback.built
    advance(plain, 1)
    advance(case, 1)
    assert not case.particles.feedback.built
    for x, y in zip(fields_of(case), fields_of(plain)):
        assert x.tobytes() == y.tobytes()
    advance(case, 2)  # initpart - 1: primed, the records exist from here on
    assert case.particles.feedback.built


def test_exact_resume(tmp_path):
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    prefix = str(tmp_path / "ck")
    whole_run = make_case("RK3", True)
    whole_run.run(n_iters=4)
    first = make_case("RK3", True)
    first.checkpoints = Checkpoints(first.solver, CheckpointConfig(checkpoint_freq=2, checkpoint_prefix=prefix), first)
    first.run(n_iters=2)
    second = make_case("RK3", True)
    assert restore(second, prefix + "_000002.npz") == 2 and second.particles.iteration == 2
    second.run(n_iters=4)
    for a, c, nm in zip(fields_of(second), fields_of(whole_run), "uvw"):
        assert a.tobytes() == c.tobytes(), nm
    states = []
    for case in (second, whole_run):  # (the slots differ: a restored state arrives in id order, the other was sorted by cell)
        rows, id_, status, _ = case.particles.raw_state()
        order = np.argsort(id_, kind="stable")
        states.append(rows[:, order].tobytes() + status[order].tobytes())
    assert states[0] == states[1]


# ---------------------------------------------------------------- 3. FP32
def test_fp32_flavour():
    """the kernel cases and the coupled steps on 4-byte fields (libx3d2_hip_sp.so), in a process of its own; the worker asserts
    with the FP32 bounds of the module docstring"""
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "feedback_sp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("FEEDBACKRESULT ")][-1]
    print(line)
    assert "float32" in line


# ---------------------------------------------------------------- 4. refusals
def test_every_refusal_raises_and_launches_nothing():
    from x3d2_amd.common import DIR_X, VERT, X3dError
    from x3d2_amd.particles import Particles, ParticlesConfig
    s, st, _ = kernel_reference("box")
    b = s.backend
    lib, h = b.lib, b.h
    x0 = st["x"]
    s.particle_feedback = None  # (the solver is shared with the tests above)

    def refused(solver, cfg, match):
        p = Particles.__new__(Particles)
        with pytest.raises(X3dError, match=match):
            p.__init__(solver, cfg)
        assert p.h is None and p.feedback is None and solver.particle_feedback is None

    # the configuration
    for kw in (dict(tau_p=0.0, two_way=True, mass=1.0), dict(tau_p=TAU, two_way=True), dict(tau_p=TAU, two_way=True, mass=0.0),
               dict(tau_p=TAU, two_way=True, mass=-2.0), dict(tau_p=TAU, two_way=True, mass=float("nan")),
               dict(tau_p=TAU, two_way=True, mass=float("inf"))):
        with pytest.raises(X3dError):
            ParticlesConfig(x0, **kw)
    cfg = ParticlesConfig(x0, tau_p=TAU, two_way=True, mass=MASS)
    # an odd vertex count in a periodic direction
    for dims in ((15, 12, 10), (16, 12, 9)):
        odd = make_solver("box", dims)
        refused(odd, ParticlesConfig(x0[:10] * 0.0, tau_p=TAU, two_way=True, mass=MASS), "even vertex count")
    # several ranks: a communicator of two

    class Two:
        size = 2

    comm, b.comm = b.comm, Two()
    try:
        refused(s, cfg, "several ranks")
    finally:
        b.comm = comm
    # the C ABI
    p = make_particles(s, st)
    tracers = Particles(s, ParticlesConfig(x0))
    inv = [np.ascontiguousarray(t) for t in p.feedback.inv_d]
    tabs = [t.ctypes.data_as(DP) for t in inv]
    blocks = [b.allocator.get_block(DIR_X, VERT) for _ in range(3)]
    for f in blocks:
        f.fill(1e30)
    before = [whole(f) for f in blocks]
    dims = b._dims(VERT)
    other = make_solver("box").backend
    err = lib.x3d_last_error
    assert lib.x3d_particles_feedback_enable(h, tracers.h, 1.0, *tabs) != 0 and b"tracers" in err()
    assert lib.x3d_particles_feedback_enable(h, p.h, 1.0, *tabs) != 0 and b"already" in err()
    plain = Particles(s, ParticlesConfig(x0, tau_p=TAU))
    for mass in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.x3d_particles_feedback_enable(h, plain.h, mass, *tabs) != 0 and b"mass" in err()
    assert lib.x3d_particles_feedback_enable(h, plain.h, 1.0, tabs[0], None, tabs[2]) != 0 and b"null" in err()
    assert lib.x3d_particles_feedback_enable(None, plain.h, 1.0, *tabs) != 0
    assert lib.x3d_particles_feedback_enable(h, None, 1.0, *tabs) != 0
    assert lib.x3d_particles_feedback_enable(other.h, plain.h, 1.0, *tabs) != 0 and b"another backend" in err()
    assert lib.x3d_particles_feedback_build(h, plain.h) != 0 and b"not enabled" in err()
    assert lib.x3d_particles_feedback_add(h, plain.h, blocks[0].ptr, blocks[1].ptr, blocks[2].ptr, dims) != 0 and b"not built" in err()
    assert lib.x3d_particles_feedback_build(other.h, p.h) != 0 and b"another backend" in err()
    ptrs = [f.ptr for f in blocks]
    assert lib.x3d_particles_feedback_add(other.h, p.h, *ptrs, dims) != 0 and b"another backend" in err()
    assert lib.x3d_particles_feedback_add(h, p.h, None, ptrs[1], ptrs[2], dims) != 0 and b"null" in err()
    assert lib.x3d_particles_feedback_add(h, p.h, *ptrs, None) != 0 and b"null" in err()
    assert lib.x3d_particles_feedback_add(h, p.h, ptrs[0], ptrs[0], ptrs[2], dims) != 0 and b"same block" in err()
    assert lib.x3d_particles_feedback_add(h, p.h, ptrs[0], ptrs[1], ptrs[1], dims) != 0 and b"same block" in err()
    from x3d2_amd import _lib
    assert lib.x3d_particles_feedback_add(h, p.h, *ptrs, _lib.ints(16, 12, 9)) != 0 and b"dims" in err()
    assert lib.x3d_particles_feedback_download(h, p.h, None, None, None) != 0
    assert all(x.tobytes() == whole(f).tobytes() for x, f in zip(before, blocks))
    for f in blocks:
        b.allocator.release_block(f)
    s.particle_feedback = None
