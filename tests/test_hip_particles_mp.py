"""Particles on several ranks (csrc/particles.hip x3d_particles_mp_*, x3d2_amd/particles.py) against tests/particles_ref.py
(values) and tests/particles_mp_ref.py (ownership, classification, compaction order) and against the one-rank device run.

Ranks are processes that share cuda:0 and exchange through gloo (tests/mp_particles_worker.py); one start of the worker serves
every case of a layout.  The bounds are those of tests/test_hip_particles.py: updates are compared ONE at a time from the
device's own previous state, positions to 1e-12 max(L), velocities to 1e-12 max(1, max|u|), F to 2e-12 max(1, max|u|) / tau.
The split advance (move, migrate, sample) holds the expressions of the fused kernel: by id it gives the one-rank device run's
bits, which is asserted.

 1. fixed fields, many crossings   2. invariants after every step   3. compaction edge counts   4. overflow
 5. real runs   6. files and restart   7. refusals   8. FP32"""
import ctypes
import functools
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import particles_mp_ref as mref
import particles_ref as ref
from test_particles_mp_host import TWOPI, box_mesh, channel_mesh
from x3d2_amd.particles import Particles, ParticlesConfig, load_particles, seed_uniform, wrap

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 1e-12
KEYS = ("x", "v", "a", "v_prev", "F", "F_prev")
N = 3000
STEPS = 8
PORTS = {("fixed", "box", (1, 2, 1)): 29601, ("fixed", "box", (1, 1, 2)): 29602, ("fixed", "box", (1, 2, 2)): 29603,
         ("fixed", "channel", (1, 1, 2)): 29604, ("edges", "box", (1, 1, 2)): 29605, ("overflow", "box", (1, 1, 2)): 29606,
         ("real", "box", (1, 2, 1)): 29607, ("real", "box", (1, 1, 2)): 29608, ("real", "channel", (1, 1, 2)): 29609,
         ("restart", "box", (1, 1, 2)): 29610, ("fixed32", "box", (1, 1, 2)): 29611}
MESHES = {"box": box_mesh, "channel": channel_mesh}
# time steps of the fixed-field runs: max|u| is about 2, so a particle travels up to 0.45 of a slab (pi or 1) per step
DT = {"box": 0.6, "channel": 0.2}


# ---------------------------------------------------------------- what the ranks run (also imported by the worker)
def make_case(name, layout=(1, 1, 1), rank=0, comm=None, **kw):
    from x3d2_amd import make_channel, make_tgv
    if name == "box":
        kw.setdefault("poisson", "CG" if "fused" not in kw else "FFT")  # (never stepped with CG)
        return make_tgv(32, nproc_dir=layout, rank=rank, comm=comm, **kw)
    return make_channel((32, 33, 24), nproc_dir=layout, rank=rank, comm=comm, **kw)


def global_fields(axes):
    """a smooth field with every component depending on every coordinate and a flow through the walls of the channel (it
    is only interpolated, never stepped): [u, v, w] as [nz, ny, nx]"""
    ph = [2.0 * np.pi * (ax.c - (0.0 if ax.periodic else ax.lo)) / (ax.L if ax.periodic else ax.hi - ax.lo) for ax in axes]
    X, Y, Z = ph[0][None, None, :], ph[1][None, :, None], ph[2][:, None, None]
    u = np.sin(X) * np.cos(Y) + 0.3 * np.cos(2.0 * Z) + 0.0 * Y
    v = np.cos(X + 1.0) * np.sin(Y + 0.5) + 0.8 * np.cos(Z) + 0.4
    w = np.sin(Y) * np.cos(X) + 0.7 * np.sin(Z + 0.3) - 0.5 + 0.0 * X
    return [np.ascontiguousarray(np.broadcast_to(f, (axes[2].n, axes[1].n, axes[0].n))) for f in (u, v, w)]


def local_part(mesh, f):
    lo, nl = [int(v) for v in mesh.n_offset], [int(v) for v in mesh.vert_dims]
    return np.ascontiguousarray(f[lo[2]:lo[2] + nl[2], lo[1]:lo[1] + nl[1], lo[0]:lo[0] + nl[0]])


def set_fields(case, fields):
    s = case.solver
    for f, a in zip((s.u, s.v, s.w), fields):
        s.backend.set_field_data(f, local_part(s.mesh, a))


def particle_config(name, inertial, dt, seed=51, n=N, **kw):
    tau = 4.0 * dt if inertial else 0.0
    g = (0.3, -0.5, 0.2) if inertial else (0.0, 0.0, 0.0)
    return ParticlesConfig(seed_uniform(MESHES[name](), n, seed=seed), tau_p=tau, gravity=g, sort_every=0, **kw)


def record(p, res, s):
    """after step s: the rank's device order and (collective) the whole state by id"""
    _, id_, _, _ = p.raw_state()
    res["ids_%d" % s] = id_.astype(np.int64)
    rows, gid, status, _ = p._gathered()
    o = np.argsort(gid, kind="stable")
    res["rows_%d" % s], res["status_%d" % s] = rows[:, o], status[o].astype(np.int32)


def fixed_run(layout, rank, comm, name="box", order=4, inertial=False, wall="reflect", out=None):
    """prime and STEPS advances on the fixed global field; try interpolate once"""
    from x3d2_amd.common import X3dError
    case = make_case(name, layout, rank, comm)
    s = case.solver
    s.dt = DT[name]  # (the particles check tau_p against it)
    set_fields(case, global_fields(ref.axes_of(MESHES[name]())))
    p = Particles(s, particle_config(name, inertial, DT[name], order=order, wall=wall))
    res = {}
    record(p, res, 0)
    for it in range(1, STEPS + 1):
        p.advance(s.u, s.v, s.w, DT[name])
        record(p, res, it)
    p.check()
    if int(np.prod(layout)) > 1:
        try:
            p.interpolate(np.zeros((1, 3)), s.u, s.v, s.w)
            res["interpolate"] = np.array("returned")
        except X3dError as e:
            res["interpolate"] = np.array(str(e))
    return res


def edge_run(layout, rank, comm, n=256, order=4, out=None):
    """every particle starts in rank 0's half (z < pi); w = 1, u = v = 0: a step in which nobody leaves, then one in which
    every resident of rank 0 leaves (dt = pi), then one more of each"""
    case = make_case("box", layout, rank, comm)
    s = case.solver
    axes = ref.axes_of(box_mesh())
    shape = (axes[2].n, axes[1].n, axes[0].n)
    set_fields(case, [np.zeros(shape), np.zeros(shape), np.ones(shape)])
    x0 = seed_uniform(box_mesh(), n, seed=61)
    x0[:, 2] = 0.25 + x0[:, 2] * (np.pi - 0.5) / TWOPI
    s.dt = 1e-3
    p = Particles(s, ParticlesConfig(x0, order=order, sort_every=0, capacity=n + 8, mig_capacity=n))
    res = {"x0": x0}
    record(p, res, 0)
    for it, dt in enumerate((1e-3, np.pi, 1e-3, np.pi), start=1):
        p.advance(s.u, s.v, s.w, dt)
        record(p, res, it)
        res["count_%d" % it] = np.int64(p.check())
    return res


def overflow_run(layout, rank, comm, what="mig", out=None):
    """the second step of edge_run with a message of one slot (what = "mig"), or with 10 slots of state on the rank
    everybody moves to (what = "cap"): the step completes everywhere, check() names the cause on the rank it happened on"""
    from x3d2_amd.common import X3dError
    n = 500
    case = make_case("box", layout, rank, comm)
    s = case.solver
    axes = ref.axes_of(box_mesh())
    shape = (axes[2].n, axes[1].n, axes[0].n)
    set_fields(case, [np.zeros(shape), np.zeros(shape), np.ones(shape)])
    x0 = seed_uniform(box_mesh(), n, seed=62)
    x0[:, 2] = 0.25 + x0[:, 2] * (np.pi - 0.5) / TWOPI
    s.dt = 1e-3
    cap = (n + 8, 1) if what == "mig" else (n + 8 if rank == 0 else 10, n)
    p = Particles(s, ParticlesConfig(x0, sort_every=0, capacity=cap[0], mig_capacity=cap[1]))
    p.advance(s.u, s.v, s.w, np.pi)
    p.advance(s.u, s.v, s.w, 1e-3)  # (and the state can still be advanced)
    res = {}
    for call in ("check", "raw_state", "state_dict"):
        try:
            getattr(p, call)()
            res[call] = np.array("")
        except X3dError as e:
            res[call] = np.array(str(e))
    q = (ctypes.c_int * 2)(0, 0)
    assert s.backend.lib.x3d_particles_mp_query(s.backend.h, p.h, q) == 0
    res["count"], res["flags"] = np.int64(q[0]), np.int64(q[1])
    return res


def real_run(layout, rank, comm, name="box", fused=True, inertial=False, sort_every=0, particles=True, steps=2, out=None):
    """`steps` steps of BaseCase.run; after every step the rank's fields and the whole particle state; a file at step 2"""
    case = make_case(name, layout, rank, comm, fused=fused)
    s = case.solver
    res = {}
    p = None
    if particles:
        cfg = particle_config(name, inertial, float(s.dt), ipartout=2, prefix="%s_%s" % (out, "f" if fused else "o"))
        cfg.sort_every = sort_every
        case.particles = p = Particles(s, cfg)
        record(p, res, 0)
    s.flush_grad()
    for c, f in zip("uvw", (s.u, s.v, s.w)):
        res["%s_0" % c] = s.backend.get_field_data(f)
    for it in range(1, steps + 1):
        case.run(n_iters=it)
        s.flush_grad()
        for c, f in zip("uvw", (s.u, s.v, s.w)):
            res["%s_%d" % (c, it)] = s.backend.get_field_data(f)
        if p is not None:
            record(p, res, it)
    res["lo"], res["nl"] = np.array(s.mesh.n_offset), np.array(s.mesh.vert_dims)
    if p is not None:
        p.check()
        st = p.state()
        if rank == 0:
            got = load_particles(p.cfg.prefix, 2)
            res["file_equals_state"] = np.array(all(np.asarray(got[k]).tobytes() == np.asarray(st[k]).tobytes() for k in st))
            res["files"] = np.array([os.path.exists("%s_000002.r%d.npz" % (p.cfg.prefix, r)) for r in range(int(np.prod(layout)))])
    return res


def restart_run(layout, rank, comm, inertial=False, out=None):
    """6 steps in one piece; 3 steps, checkpoint, a fresh case restored and run to 6; a restore from the other rank's file"""
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    from x3d2_amd.common import X3dError
    prefix = "%s_ck%d" % (out, int(inertial))

    def build():
        case = make_case("box", layout, rank, comm, fused=True)
        case.particles = Particles(case.solver, particle_config("box", inertial, float(case.solver.dt)))
        case.particles.cfg.sort_every = 2
        return case

    def bits(case):
        rows, id_, status, hist = case.particles.raw_state()
        o = np.argsort(id_, kind="stable")  # (by id: a restored state starts in id order, the device order is no part of it)
        rows, id_, status = np.ascontiguousarray(rows[:, o]), id_[o], status[o]
        s = case.solver
        s.flush_grad()
        return b"".join([rows.tobytes(), id_.tobytes(), status.tobytes(), bytes([hist])] +
                        [s.backend.get_field_data(f).tobytes() for f in (s.u, s.v, s.w)])

    whole = build()
    whole.run(n_iters=6)
    first = build()
    first.checkpoints = Checkpoints(first.solver, CheckpointConfig(checkpoint_freq=3, checkpoint_prefix=prefix), first)
    first.run(n_iters=3)
    comm.barrier()
    second = build()
    res = {"restored_at": np.int64(restore(second, "%s_000003.r%d.npz" % (prefix, rank)))}
    second.run(n_iters=6)
    res["same_bits"] = np.array(bits(second) == bits(whole))
    res["moved"] = np.array(bits(whole) != bits(first))
    third = build()
    before = bits(third)
    # the other rank's file: restore() refuses it (its check of the decomposition sees the other rank's offsets before the
    # particles are looked at), and so does Particles.load_state_dict on its own, by the ownership rule
    try:
        restore(third, "%s_000003.r%d.npz" % (prefix, 1 - rank))
        res["swapped_restore"] = np.array("accepted")
    except X3dError as e:
        res["swapped_restore"] = np.array(str(e))
    res["untouched_by_restore"] = np.array(bits(third) == before and third.solver.current_iter == 0)
    z = dict(np.load("%s_000003.r%d.npz" % (prefix, 1 - rank)))
    try:
        third.particles.load_state_dict(z)
        res["swapped"] = np.array("accepted")
    except X3dError as e:
        res["swapped"] = np.array(str(e))
    res["untouched"] = np.array(bits(third) == before)
    return res


# ---------------------------------------------------------------- starting the ranks
@functools.lru_cache(maxsize=None)
def spawn(scenario, name, layout, cases_json, tmp, sp=False):
    """one start of the worker for all `cases` of a layout -> per rank the dict it saved"""
    nranks = int(np.prod(layout))
    out = os.path.join(tmp, "%s_%s_%s" % (scenario, name, "".join(map(str, layout))))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if sp:
        env["X3D_SINGLE_PREC"] = "1"
    else:
        env.pop("X3D_SINGLE_PREC", None)
    port = PORTS[(scenario + ("32" if sp else ""), name, layout)]
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % nranks,
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(HERE, "mp_particles_worker.py"), scenario,
           ",".join(map(str, layout)), out, cases_json]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load(out + ".%d.npz" % k)) for k in range(nranks)]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("mp_particles"))


def case_of(parts, i):
    """case i of every rank's file"""
    pre = "c%d_" % i
    return [{k[len(pre):]: v for k, v in p.items() if k.startswith(pre)} for p in parts]


def state_of(rows, status):
    st = {k: rows[3 * q:3 * q + 3].T.copy() for q, k in enumerate(KEYS[:rows.shape[0] // 3])}
    st["status"] = status.astype(np.int32)
    return st


def compare_states(label, got, want, Lmax, umax, tau):
    rows = [(label + " x", float(np.max(np.abs(got["x"] - want["x"]))), BOUND * Lmax)]
    for k in ("v", "a", "v_prev"):
        rows.append((label + " " + k, float(np.max(np.abs(got[k] - want[k]))), BOUND * max(1.0, umax)))
    if tau > 0.0:
        for k in ("F", "F_prev"):
            rows.append((label + " " + k, float(np.max(np.abs(got[k] - want[k]))), 2.0 * BOUND * max(1.0, umax) / tau))
    return rows


def check_rows(rows):
    for name, err, bound in rows:
        print("particles mp %-52s err %.3e  bound %.3e" % (name, err, bound))
    for name, err, bound in rows:
        assert err <= bound, name


def ulp_distance(a, b):
    """the largest distance of two double arrays in units of the last place, in exact integer arithmetic on the elements
    whose patterns differ (0: the same bits up to the sign of zero; the callers compare the bytes as well)"""
    ia, ib = (np.ascontiguousarray(q, dtype=np.float64).view(np.int64).ravel() for q in (a, b))
    big = 0
    for v, w in zip(ia[ia != ib].tolist(), ib[ia != ib].tolist()):
        v, w = (-2 ** 63 - v if v < 0 else v), (-2 ** 63 - w if w < 0 else w)  # the patterns in the order of the values
        big = max(big, abs(v - w))
    return big


def check_steps(label, parts, axes, layout, fields_at, x0, dt, order, tau, g, wall, steps, sorted_every=0):
    """tests 1 and 2 on the records of one case: every update against the restatement's ONE update from the device's previous
    state; after every step the ids a permutation, every particle on the rank that owns it, every rank's device order the
    restated one.  Returns (rows, per-step masks)."""
    Lmax = max(ax.L for ax in axes)
    nranks = len(parts)
    x0w = x0.copy()
    for d in range(3):
        if axes[d].periodic:
            x0w[:, d] = wrap(x0w[:, d], axes[d].L)
    order_now = mref.initial_order(axes, layout, x0w)
    for r in range(nranks):
        assert np.array_equal(parts[r]["ids_0"], order_now[r]), "seeding, rank %d" % r
    f0 = fields_at(0)
    umax = max(float(np.max(np.abs(f))) for f in f0)
    prev = state_of(parts[0]["rows_0"], parts[0]["status_0"])
    rows = compare_states(label + " primed", prev, ref.prime(axes, f0, x0, order, tau, g), Lmax, umax, tau)
    masks = []
    for s in range(1, steps + 1):
        fields = fields_at(s)
        umax = max(float(np.max(np.abs(f))) for f in fields)
        got = state_of(parts[0]["rows_%d" % s], parts[0]["status_%d" % s])
        want, info = ref.update(axes, fields, prev, dt, order, s == 1, tau, g, wall)
        rows += compare_states("%s step %d" % (label, s), got, want, Lmax, umax, tau)
        assert np.array_equal(got["status"], want["status"])
        # 2. invariants
        ids = [parts[r]["ids_%d" % s] for r in range(nranks)]
        assert np.array_equal(np.sort(np.concatenate(ids)), np.arange(x0.shape[0]))
        own = mref.owner(axes, layout, got["x"])
        for r in range(nranks):
            assert np.all(own[ids[r]][got["status"][ids[r]] != 2] == r), "step %d: a particle of rank %d lies outside its interval" % (s, r)
        if not sorted_every:
            order_now = mref.migrate(axes, layout, order_now, got["x"], got["status"])
            for r in range(nranks):
                assert np.array_equal(ids[r], order_now[r]), "step %d: device order of rank %d" % (s, r)
        was = mref.owner(axes, layout, prev["x"])
        changed = (own != was) & (prev["status"] == 1)
        oy, _ = mref.owner_1d(axes[1], layout[1], got["x"][:, 1])
        py, _ = mref.owner_1d(axes[1], layout[1], prev["x"][:, 1])
        oz, _ = mref.owner_1d(axes[2], layout[2], got["x"][:, 2])
        pz, _ = mref.owner_1d(axes[2], layout[2], prev["x"][:, 2])
        seam = np.zeros(x0.shape[0], dtype=bool)
        for d in (1, 2):
            if layout[d] > 1 and axes[d].periodic:
                seam |= np.abs(got["x"][:, d] - prev["x"][:, d]) > 0.5 * axes[d].L
        masks.append({"changed": changed, "both": changed & (oy != py) & (oz != pz), "seam": changed & seam,
                      "reflected": changed & info["reflected"], "absorbed": changed & info["absorbed"]})
        prev = got
    return rows, masks


# ---------------------------------------------------------------- 1. fixed fields, many crossings; 2. invariants
COMBOS = [dict(order=o, inertial=i) for o in (2, 4) for i in (False, True)]
FIXED = {("box", lay): [dict(name="box", **c) for c in COMBOS] for lay in [(1, 2, 1), (1, 1, 2), (1, 2, 2)]}
FIXED[("channel", (1, 1, 2))] = [dict(name="channel", wall=w, **c) for w in ("reflect", "absorb") for c in COMBOS]


@functools.lru_cache(maxsize=None)
def one_rank(name, order, inertial, wall):
    """the same run on one rank, in this process: the device's own answer by id"""
    res = fixed_run((1, 1, 1), 0, None, name=name, order=order, inertial=inertial, wall=wall)
    return res


@pytest.mark.parametrize("name,layout", sorted(FIXED))
def test_fixed_fields_many_crossings_and_invariants(name, layout, tmp):
    cases = FIXED[(name, layout)]
    parts = spawn("fixed", name, layout, json.dumps(cases), tmp)
    axes = ref.axes_of(MESHES[name]())
    fields = global_fields(axes)
    dt = DT[name]
    rows, worst_ulp, same_bits = [], 0, True
    seen = {k: 0 for k in ("changed", "both", "seam", "reflected", "absorbed")}
    most = 0.0
    for i, c in enumerate(cases):
        cfg = particle_config(name, c["inertial"], dt)
        wall = c.get("wall", "reflect")
        label = "%s %s o%d %s %s" % (name, layout, c["order"], "inertial" if c["inertial"] else "tracers", wall)
        got = case_of(parts, i)
        r, masks = check_steps(label, got, axes, layout, lambda s: fields, cfg.x0, dt, c["order"], cfg.tau_p, cfg.gravity, wall, STEPS)
        rows += r
        for m in masks:
            most = max(most, float(np.mean(m["changed"])))
            for k in seen:
                seen[k] += int(np.sum(m[k]))
        assert "not built on several ranks" in str(got[0]["interpolate"])
        one = one_rank(name, c["order"], c["inertial"], wall)
        for s in range(STEPS + 1):
            u = ulp_distance(one["rows_%d" % s], got[0]["rows_%d" % s])
            worst_ulp = max(worst_ulp, u)
            assert np.array_equal(one["status_%d" % s], got[0]["status_%d" % s])
            same_bits = same_bits and one["rows_%d" % s].tobytes() == got[0]["rows_%d" % s].tobytes()
            rows.append(("%s step %d against one rank" % (label, s),
                         float(np.max(np.abs(one["rows_%d" % s] - got[0]["rows_%d" % s]))), BOUND))
    print("particles mp %s %s: most particles changing rank in a step %.3f, crossings %s, largest distance from the one-rank run %d ulp, same bytes %s"
          % (name, layout, most, seen, worst_ulp, same_bits))
    check_rows(rows)
    # the run is not vacuous
    assert most >= 0.10
    assert seen["seam"] >= 1
    if layout == (1, 2, 2):
        assert seen["both"] >= 1
    if name == "channel":
        assert seen["reflected"] >= 1 and seen["absorbed"] >= 1
    assert worst_ulp == 0 and same_bits  # the split advance holds the fused kernel's expressions: the same bits by id


# ---------------------------------------------------------------- 3. compaction edge counts
def test_compaction_edge_counts(tmp):
    cases = [dict(n=n, order=o) for n, o in ((255, 4), (256, 4), (257, 2), (3000, 4))]
    parts = spawn("edges", "box", (1, 1, 2), json.dumps(cases), tmp)
    axes = ref.axes_of(box_mesh())
    shape = (axes[2].n, axes[1].n, axes[0].n)
    fields = [np.zeros(shape), np.zeros(shape), np.ones(shape)]
    dts = (1e-3, np.pi, 1e-3, np.pi)
    rows = []
    for i, c in enumerate(cases):
        got = case_of(parts, i)
        n = c["n"]
        assert got[0]["ids_0"].size == n and got[1]["ids_0"].size == 0  # the other rank holds none
        Lmax = TWOPI
        prev = state_of(got[0]["rows_0"], got[0]["status_0"])
        order_now = [np.arange(n), np.arange(0)]
        for s, dt in enumerate(dts, start=1):
            now = state_of(got[0]["rows_%d" % s], got[0]["status_%d" % s])
            want, _ = ref.update(axes, fields, prev, dt, c["order"], s == 1, 0.0, (0.0,) * 3, "reflect")
            rows += compare_states("edges n=%d step %d" % (n, s), now, want, Lmax, 1.0, 0.0)
            order_now = mref.migrate(axes, (1, 1, 2), order_now, now["x"], now["status"])
            counts = [int(got[r]["count_%d" % s]) for r in range(2)]
            for r in range(2):
                assert np.array_equal(got[r]["ids_%d" % s], order_now[r])
            # nobody leaves in steps 1 and 3; every resident of the full rank leaves in steps 2 and 4
            assert counts == {1: [n, 0], 2: [0, n], 3: [0, n], 4: [n, 0]}[s], (n, s, counts)
            prev = now
    check_rows(rows)


# ---------------------------------------------------------------- 4. overflow
def test_overflow_is_an_error_not_a_loss_or_a_hang(tmp):
    parts = spawn("overflow", "box", (1, 1, 2), json.dumps([dict(what="mig"), dict(what="cap")]), tmp)
    mig, cap = case_of(parts, 0), case_of(parts, 1)
    # a message of one slot: the 500 leavers of rank 0 stayed there, and every host call says why and where
    assert int(mig[0]["count"]) == 500 and int(mig[1]["count"]) == 0
    for call in ("check", "raw_state", "state_dict"):
        assert "rank 0" in str(mig[0][call]) and "mig_capacity" in str(mig[0][call])
        assert str(mig[1][call]) == ""
    # 10 slots on the rank everybody moves to: 10 were taken, the flag is up THERE
    assert int(cap[0]["count"]) == 0 and int(cap[1]["count"]) == 10
    assert "rank 1" in str(cap[1]["check"]) and "more residents than capacity" in str(cap[1]["check"])
    assert str(cap[0]["check"]) == ""


# ---------------------------------------------------------------- 5. real runs; 6. files
def gathered_fields(parts, s, shape):
    out = [np.zeros(shape) for _ in range(3)]
    for p in parts:
        lo, nl = p["lo"], p["nl"]
        for f, c in zip(out, "uvw"):
            f[lo[2]:lo[2] + nl[2], lo[1]:lo[1] + nl[1], lo[0]:lo[0] + nl[0]] = p["%s_%d" % (c, s)]
    return out


@pytest.mark.parametrize("name,layout", [("box", (1, 2, 1)), ("box", (1, 1, 2)), ("channel", (1, 1, 2))])
def test_real_runs_files_and_the_fluid_does_not_notice(name, layout, tmp):
    cases = []
    for fused in (True, False):
        cases += [dict(name=name, fused=fused, inertial=not fused, sort_every=0), dict(name=name, fused=fused, inertial=not fused, sort_every=1),
                  dict(name=name, fused=fused, particles=False)]
    parts = spawn("real", name, layout, json.dumps(cases), tmp)
    axes = ref.axes_of(MESHES[name]())
    shape = (axes[2].n, axes[1].n, axes[0].n)
    rows = []
    for i in (0, 3):
        c = cases[i]
        plain, srt, bare = case_of(parts, i), case_of(parts, i + 1), case_of(parts, i + 2)
        dt = {"box": 1e-3, "channel": 5e-3}[name]
        cfg = particle_config(name, c["inertial"], dt)
        label = "%s %s %s" % (name, layout, "fused" if c["fused"] else "op-granular")
        for got, every in ((plain, 0), (srt, 1)):
            r, _ = check_steps(label + " sort %d" % every, got, axes, layout, lambda s: gathered_fields(got, s, shape), cfg.x0, dt, 4,
                               cfg.tau_p, cfg.gravity, "reflect", 2, sorted_every=every)
            rows += r
        for s in range(3):  # sorting changes the device order, never a bit of the state by id
            assert plain[0]["rows_%d" % s].tobytes() == srt[0]["rows_%d" % s].tobytes()
        assert np.any(plain[0]["ids_2"] != srt[0]["ids_2"]) or np.all(np.diff(plain[0]["ids_2"]) > 0)
        for r in range(len(parts)):  # the fluid does not notice
            for s in range(3):
                for comp in "uvw":
                    assert plain[r]["%s_%d" % (comp, s)].tobytes() == bare[r]["%s_%d" % (comp, s)].tobytes()
        assert bool(plain[0]["file_equals_state"]) and np.all(plain[0]["files"])
    check_rows(rows)


@pytest.mark.parametrize("inertial", [False, True])
def test_a_two_rank_resume_continues_bit_for_bit(inertial, tmp):
    parts = spawn("restart", "box", (1, 1, 2), json.dumps([dict(inertial=inertial)]), tmp)
    for got in case_of(parts, 0):
        assert int(got["restored_at"]) == 3 and bool(got["moved"])
        assert bool(got["same_bits"])
        assert str(got["swapped_restore"]) not in ("", "accepted") and bool(got["untouched_by_restore"])
        print("particles mp restore of the other rank's file:", str(got["swapped_restore"]))
        assert "not owned by this rank" in str(got["swapped"]) and bool(got["untouched"])


# ---------------------------------------------------------------- 7. refusals
def test_refusals_launch_nothing():
    from x3d2_amd import Mesh, _lib, make_tgv
    from x3d2_amd.common import X3dError
    case = make_tgv(16, poisson="CG")
    s = case.solver
    b = s.backend
    cfg = ParticlesConfig(np.full((4, 3), 0.5))
    per = ("periodic",) * 2

    def fake(mesh, size):
        return SimpleNamespace(backend=SimpleNamespace(comm=SimpleNamespace(size=size), lib=b.lib, h=b.h), mesh=mesh, dt=1e-3, current_iter=0)

    with pytest.raises(X3dError, match="x is never cut"):
        Particles(fake(Mesh((16, 16, 16), (2, 1, 1), (1.0,) * 3, per, per, per), 2), cfg)
    with pytest.raises(X3dError, match="at least 4 vertices in a cut direction"):
        Particles(fake(Mesh((16, 16, 6), (1, 1, 2), (1.0,) * 3, per, per, per), 2), cfg)
    # the library itself: a cut x, three vertices on a rank, null and foreign handles
    p = Particles(s, cfg)  # a one-rank handle
    before = p.raw_state()[0].tobytes()
    lib = b.lib
    prm = _lib.ParticlesParams()
    prm.n, prm.order = 4, 4
    coords = [np.arange(32) / 32.0 for _ in range(3)]
    for d in range(3):
        prm.periodic[d], prm.uniform[d], prm.L[d] = 1, 1, 1.0
        prm.coords[d] = coords[d].ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    h = ctypes.c_void_p()
    for nproc, nglobal, nlocal, text in (((2, 1, 1), (32, 16, 16), (16, 16, 16), "x is never cut"),
                                         ((1, 1, 2), (16, 16, 6), (16, 16, 3), "4 vertices in a cut direction")):
        dc = _lib.ParticlesDecomp()
        for d in range(3):
            dc.nglobal[d], dc.offset[d], dc.nlocal[d], dc.nproc[d], dc.rank[d] = nglobal[d], 0, nlocal[d], nproc[d], 0
        dc.capacity, dc.mig_capacity = 16, 4
        assert lib.x3d_particles_mp_create(b.h, ctypes.byref(prm), ctypes.byref(dc), None, None, None, 0, ctypes.byref(h)) != 0
        assert text in lib.x3d_last_error().decode() and not h.value
    # create: every null argument, and a decomposition that is not this backend's block
    dc = _lib.ParticlesDecomp()
    for d in range(3):
        dc.nglobal[d], dc.offset[d], dc.nlocal[d], dc.nproc[d], dc.rank[d] = (32 if d == 2 else 16), 0, 16, (2 if d == 2 else 1), 0
    dc.capacity, dc.mig_capacity = 16, 4
    x1, id1 = np.full((3, 1), 0.25), np.zeros(1, dtype=np.int32)
    xp, ip = x1.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), id1.ctypes.data_as(_lib.c_int_p)
    for args in ((None, ctypes.byref(prm), ctypes.byref(dc), xp, None, ip, 1, ctypes.byref(h)),
                 (b.h, None, ctypes.byref(dc), xp, None, ip, 1, ctypes.byref(h)),
                 (b.h, ctypes.byref(prm), None, xp, None, ip, 1, ctypes.byref(h)),
                 (b.h, ctypes.byref(prm), ctypes.byref(dc), None, None, ip, 1, ctypes.byref(h)),
                 (b.h, ctypes.byref(prm), ctypes.byref(dc), xp, None, None, 1, ctypes.byref(h)),
                 (b.h, ctypes.byref(prm), ctypes.byref(dc), xp, None, ip, 1, None)):
        assert lib.x3d_particles_mp_create(*args) != 0
        assert "null argument" in lib.x3d_last_error().decode() and not h.value
    small = make_tgv(8, poisson="CG").solver.backend  # another backend: its block is not the one the decomposition names
    assert lib.x3d_particles_mp_create(small.h, ctypes.byref(prm), ctypes.byref(dc), xp, None, ip, 1, ctypes.byref(h)) != 0
    assert "not this backend's part" in lib.x3d_last_error().decode() and not h.value
    rows18, i4 = (ctypes.c_double * (18 * 4))(), (ctypes.c_int * 4)()
    buf = (ctypes.c_double * 64)()
    q = (ctypes.c_int * 2)()
    dims = _lib.ints(16, 16, 16)
    u, v, w = s.u.ptr, s.v.ptr, s.w.ptr
    other = make_tgv(16, poisson="CG").solver.backend
    for handle, bk, text in ((None, b, "null argument"), (p.h, b, "live on one rank"), (p.h, other, "another backend")):
        calls = [lambda: lib.x3d_particles_mp_ghost_pack(bk.h, handle, 3, u, v, w, dims, buf, buf),
                 lambda: lib.x3d_particles_mp_ghost_unpack(bk.h, handle, 3, buf, buf),
                 lambda: lib.x3d_particles_mp_prime(bk.h, handle, u, v, w, dims),
                 lambda: lib.x3d_particles_mp_move(bk.h, handle, 1e-3),
                 lambda: lib.x3d_particles_mp_sample(bk.h, handle, u, v, w, dims),
                 lambda: lib.x3d_particles_mp_emigrate(bk.h, handle, 3, buf, buf),
                 lambda: lib.x3d_particles_mp_immigrate(bk.h, handle, 3, buf, buf),
                 lambda: lib.x3d_particles_mp_sort(bk.h, handle),
                 lambda: lib.x3d_particles_mp_query(bk.h, handle, q),
                 lambda: lib.x3d_particles_mp_pack(bk.h, handle, buf, 512),
                 lambda: lib.x3d_particles_mp_download(bk.h, handle, rows18, i4, i4, q, q, q),
                 lambda: lib.x3d_particles_mp_upload(bk.h, handle, None, None, None, 0, 0)]
        for call in calls:
            assert call() != 0
            assert text in lib.x3d_last_error().decode(), lib.x3d_last_error().decode()
    assert p.raw_state()[0].tobytes() == before


# ---------------------------------------------------------------- 8. FP32
def test_fp32_flavour_on_two_ranks(tmp):
    """one case of test 1 on 4-byte fields: the restatement takes the float32 fields widened to double, the FP64 bounds hold"""
    c = dict(name="box", order=4, inertial=True)
    parts = spawn("fixed", "box", (1, 1, 2), json.dumps([c]), tmp, sp=True)
    assert str(parts[0]["dtype"]) == "float32"
    axes = ref.axes_of(box_mesh())
    fields = [f.astype(np.float32).astype(np.float64) for f in global_fields(axes)]
    cfg = particle_config("box", True, DT["box"])
    rows, masks = check_steps("fp32 box (1, 1, 2)", case_of(parts, 0), axes, (1, 1, 2), lambda s: fields, cfg.x0, DT["box"], 4, cfg.tau_p,
                              cfg.gravity, "reflect", STEPS)
    check_rows(rows)
    assert max(float(np.mean(m["changed"])) for m in masks) >= 0.10
