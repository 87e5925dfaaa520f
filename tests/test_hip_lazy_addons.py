"""Deferred execution (HipBackend(lazy=True), csrc/lazy.hip) under the add-ons that run AT ONCE on translated handles:
active scalars, explicit LES, particles, snapshots, probes (X3D_LAZY_IN / X3D_LAZY_OUT / X3D_LAZY_EAGER of csrc/common.h in
scalars.hip, les.hip, particles.hip, snapshot.hip, probe.hip) and the restart that unpacks onto handles (checkpoint.hip).

Every comparison is against the same driver executing call by call (lazy=False), bit for bit unless stated.  The feature test
files hold that eager path to their high-precision restatements (scalars_ref, les_ref, particles_ref, snapshot_ref,
loads_ref): equality with it carries those references over to the deferred mode.

Layer 1 -- each entry point behind a queue that holds ALIASES.  veccopy moves nothing while the mode is on: the destination
becomes another name of the source's buffer.  A handle an entry point writes in place (full = false) must then get a buffer of
its own and a copy first (`materialised`), and the other name must keep its data; a handle whose data live in another handle's
buffer is only found through the translation -- its own memory holds stale values.  A wrong or missing translation faults
nothing, it silently touches some other field: the bystanders are read back with everything else.  `materialised` is
read right before and right after the entry point, and no recorded call behind the aliasing veccopy updates an aliased block,
so the difference is the entry point's own copy-on-write.

Layer 2 -- whole steps of the op-granular driver with the add-ons attached, through BaseCase.run, eager against deferred, with
the engagement of the rewrites read from lazy_stats() next to the bare case's figures of the same test, and a restart.

The 16-ulp bound of the channel runs with the default rules is that of tests/test_hip_lazy.py
(test_deferred_channel_steps_are_bit_identical): the pair and accumulating-solve rewrites reassociate.  Measured with these
add-ons, two RK3 steps at (32, 33, 24): 1.627 ulp with Scalars, 2.008 ulp with WALE (the docstrings of the two channel tests)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2
BETA = 0.259065151
RULES_EXACT = str(255 - 2 - 4 - 8)  # X3D_LAZY_RULES without the pair rewrites and the accumulating solve


# ---------------------------------------------------------------- helpers
def make_backend(dims, ybc=PER, lazy=False):
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    st = ("uniform", "top-bottom" if ybc == WALL else "uniform", "uniform")
    mesh = Mesh(tuple(dims), (1, 1, 1), (4.0, 2.0, 2.0), PER, ybc, PER, st, (1.0, BETA, 1.0))
    return HipBackend(mesh, lazy=lazy)


def arrays_of(dims, n, seed):
    """n standard_normal fields [nz, ny, nx], exactly representable in both flavours"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(n)]


def blocks_of(b, arrays):
    from x3d2_amd.common import DIR_X, VERT
    out = []
    for a in arrays:
        f = b.allocator.get_block(DIR_X, VERT)
        f.fill(0.0)
        b.set_field_data(f, a)
        out.append(f)
    return out


def read(b, named):
    """{name: host copy} of the named blocks (the first read runs the queue)"""
    return {k: b.get_field_data(f) for k, f in named.items()}


def materialised(b):
    return b.lazy_stats()["materialised"] if b.lazy else 0


def report(label, b):
    st = b.lazy_stats()
    print("lazy_stats %-40s %s" % (label, " ".join("%s=%d" % kv for kv in st.items() if kv[1])))
    return st


def same_bits(label, eager, lazy):
    """two dicts of host arrays: the same names, the same bytes"""
    assert sorted(eager) == sorted(lazy), label
    differ = []
    for k in eager:
        a, c = np.ascontiguousarray(eager[k]), np.ascontiguousarray(lazy[k])
        if not (a.shape == c.shape and a.dtype == c.dtype and a.tobytes() == c.tobytes()):
            differ.append(k)
    assert not differ, "%s: %s differ" % (label, ", ".join(differ))


def set_species(s, fn):
    """what Scalars(init=[fn]) does to species 0, for a bare case"""
    from x3d2_amd.common import VERT
    m = s.mesh
    x, y, z = (np.asarray(m.vert_coords[0])[None, None, :], np.asarray(m.vert_coords[1])[None, :, None],
               np.asarray(m.vert_coords[2])[:, None, None])
    s.species[0].set_data_loc(VERT)
    s.backend.set_field_data(s.species[0], np.broadcast_to(fn(x, y, z), tuple(int(n) for n in m.vert_dims)[::-1]))


def set_fields(case, seed, scale=1.0):
    s = case.solver
    dims = [int(n) for n in s.mesh.vert_dims]
    for f, a in zip((s.u, s.v, s.w), arrays_of(dims, 3, seed)):
        s.backend.set_field_data(f, scale * a)


# ================================================================ Layer 1
# ---------------------------------------------------------------- 1. x3d_scalars_couple
# i: the aliased momentum derivative (up[i] != 0: updated in place); sp: the aliased species derivative; sq: the aliased input.
# dphi_is_dst: veccopy(dphi[sp], outside) -- its data then live in the outside block's buffer -- else veccopy(outside, dphi[sp])
COUPLE = {
    # buoyancy only, up along y: the `axis` form, phi and d[1] alone are touched
    "axis": dict(ns=1, up=(0.0, 1.0, 0.0), ri=[0.7], ref=[0.25], grad=None, i=1, sp=0, sq=0, dphi_is_dst=True, fresh=None),
    # buoyancy and an imposed gradient, general up, one passive species; dphi[2] is a block fresh from the allocator
    "general": dict(ns=3, up=(0.6, 0.8, 0.0), ri=[0.7, 0.0, -0.2], ref=[0.25, 0.75, 1.25],
                    grad=[(0.3, -0.2, 0.05), (0.0, 0.0, 0.0), (0.5, -0.2, 0.15)], i=0, sp=0, sq=2, dphi_is_dst=False, fresh=2),
    # nine active species: the wide buoyancy launch (d[0..2] translated there), then two groups of imposed-gradient terms
    # (8 + 1: dphi and the velocity translated per group)
    "wide": dict(ns=9, up=(0.6, 0.0, -2.0), ri=[0.7 - 0.15 * s for s in range(9)], ref=[0.25 + 0.5 * s for s in range(9)],
                 grad=[(0.3 + 0.1 * s, -0.2, 0.05 * (s + 1)) for s in range(9)], i=2, sp=8, sq=3, dphi_is_dst=True, fresh=None),
}


def couple_run(cfg, lazy):
    from x3d2_amd.common import DIR_X, VERT
    dims, ns = (30, 12, 10), cfg["ns"]
    b = make_backend(dims, lazy=lazy)
    al = b.allocator
    blk = blocks_of(b, arrays_of(dims, 11 + 2 * ns, 40 + ns))
    d, vel, (by_d, out_p, out_q, extra, extra2), dphi, phi = blk[0:3], blk[3:6], blk[6:11], blk[11:11 + ns], blk[11 + ns:]
    i, sp, sq = cfg["i"], cfg["sp"], cfg["sq"]
    if cfg["fresh"] is not None:
        # a block that went back to the pool and is handed out again: the release is recorded, and once it has run the
        # handle has no buffer until something writes it
        al.release_block(dphi[cfg["fresh"]])
        dphi[cfg["fresh"]] = al.get_block(DIR_X, VERT)
        dphi[cfg["fresh"]].fill(0.375)  # recorded while the mode is on: both modes define the block
    b.vecadd(0.5, vel[1], 1.0, d[0])  # recorded, not run, while the mode is on
    b.vecmult(d[1], vel[2])
    b.field_scale(phi[0], 1.25)
    b.vecadd(-0.25, vel[0], 1.0, dphi[sp])
    b.field_scale(d[2], 0.75)
    b.veccopy(by_d, d[i])             # an output shared with a block outside the call
    if cfg["dphi_is_dst"]:
        b.veccopy(dphi[sp], out_p)    # an output whose data live in an outside block's buffer
    else:
        b.veccopy(out_p, dphi[sp])
    b.veccopy(phi[sq], out_q)         # an input whose data live in an outside block's buffer
    m0 = materialised(b)
    b.scalars_couple(d, dphi, vel, phi, cfg["up"], cfg["ri"], cfg["ref"], cfg["grad"])
    m1 = materialised(b)
    b.vecadd(1.0, d[i], 1.0, extra)   # reads the outputs
    b.vecadd(1.0, dphi[sp], 1.0, extra2)
    named = {"by_d": by_d, "out_p": out_p, "out_q": out_q, "extra": extra, "extra2": extra2}
    for k, fs in (("d", d), ("vel", vel), ("dphi", dphi), ("phi", phi)):
        named.update({"%s%d" % (k, n): f for n, f in enumerate(fs)})
    out = read(b, named)
    if lazy:
        st = report("scalars_couple", b)
        assert st["recorded"] > 0 and m1 - m0 >= 1, (st, m0, m1)  # d[i] was shared and is updated in place
    return out


@pytest.mark.parametrize("name", sorted(COUPLE))
def test_scalars_couple_behind_a_queue_with_aliases(name):
    cfg = COUPLE[name]
    out = {lazy: couple_run(cfg, lazy) for lazy in (False, True)}
    same_bits(name, out[False], out[True])
    e = out[False]
    # the call did something, and the block that shared d[i]'s buffer kept the values from before it
    assert not np.array_equal(e["d%d" % cfg["i"]], e["by_d"]) and np.all(np.isfinite(e["d%d" % cfg["i"]]))
    if cfg["grad"] is not None:
        assert not np.array_equal(e["dphi%d" % cfg["sp"]], e["out_p"])
    else:
        assert np.array_equal(e["dphi%d" % cfg["sp"]], e["out_p"])  # no gradient: the derivative is not touched


# ---------------------------------------------------------------- 2. x3d_scalars_apply_bc
def test_scalars_apply_bc_stamps_the_species_and_not_the_block_that_shared_its_buffer():
    dims = (30, 17, 10)
    vals = [[0.0, 0.0, 1.0, -2.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.5, 0.0, 0.0]]  # y walls: both of species 0, the upper of species 1
    out = {}
    for lazy in (False, True):
        b = make_backend(dims, WALL, lazy)
        phi0, phi1, by, src, extra = blocks_of(b, arrays_of(dims, 5, 7))
        b.vecadd(0.5, phi1, 1.0, phi0)
        b.field_scale(src, 1.25)
        b.vecmult(extra, phi1)
        b.veccopy(by, phi0)    # the stamped species shares its buffer with a bystander
        b.veccopy(phi1, src)   # ... and the other one's data live in a bystander's buffer
        m0 = materialised(b)
        b.scalars_apply_bc([phi0, phi1], [0b001100, 0b001000], vals, 63)
        m1 = materialised(b)
        b.vecadd(1.0, phi0, 1.0, extra)
        out[lazy] = read(b, dict(phi0=phi0, phi1=phi1, by=by, src=src, extra=extra))
        if lazy:
            st = report("scalars_apply_bc", b)
            assert st["recorded"] > 0 and m1 - m0 >= 1, (st, m0, m1)
    same_bits("apply_bc", out[False], out[True])
    for o in out.values():
        assert np.all(o["phi0"][:, 0, :] == 1.0) and np.all(o["phi0"][:, -1, :] == -2.0) and np.all(o["phi1"][:, -1, :] == 0.5)
        # the bystanders keep their unstamped faces, and everything else
        assert np.array_equal(o["by"][:, 1:-1, :], o["phi0"][:, 1:-1, :]) and not np.any(o["by"][:, 0, :] == 1.0)
        assert not np.any(o["by"][:, -1, :] == -2.0) and not np.any(o["src"][:, -1, :] == 0.5)
        assert np.array_equal(o["src"][:, :-1, :], o["phi1"][:, :-1, :])


# ---------------------------------------------------------------- 3. x3d_scalars_profile_sums
@pytest.mark.parametrize("profile_dir", [2, 3])
def test_scalars_profile_sums_behind_queued_updates(profile_dir):
    import torch
    from x3d2_amd import _lib
    dims = (30, 12, 10)
    out = {}
    for lazy in (False, True):
        b = make_backend(dims, lazy=lazy)
        u, v, w, p0, p1, src = blocks_of(b, arrays_of(dims, 6, 9))
        nk = dims[profile_dir - 1]
        sums = torch.zeros(2 * 5 * nk, dtype=_lib.torch_real(), device=b.device)
        minmax = torch.zeros(4, dtype=_lib.torch_real(), device=b.device)
        b.vecadd(0.5, v, 1.0, u)
        b.vecmult(w, u)
        b.field_scale(p0, 1.25)
        b.veccopy(v, src)   # v's data live in another block's buffer
        b.veccopy(p1, w)    # a species that is an alias of w
        b.scalars_profile_sums(u, v, w, [p0, p1], profile_dir, sums, minmax)
        b.vecadd(1.0, u, 1.0, src)
        o = read(b, dict(u=u, v=v, w=w, p0=p0, p1=p1, src=src))
        torch.cuda.synchronize()
        o["sums"], o["minmax"] = sums.cpu().numpy(), minmax.cpu().numpy()
        out[lazy] = o
        if lazy:
            assert report("scalars_profile_sums dir %d" % profile_dir, b)["recorded"] > 0
    same_bits("profile_sums", out[False], out[True])
    e = out[False]
    assert np.array_equal(e["p1"], e["w"]) and np.all(e["sums"] != 0.0)
    assert e["minmax"][2] == e["w"].min() and e["minmax"][3] == e["w"].max()


# ---------------------------------------------------------------- 4. x3d_les_stress
@pytest.mark.parametrize("model", ["smagorinsky", "wale"])
def test_les_stress_on_recorded_gradients_with_aliases(model):
    """the nine gradients as Les.add forms them (Solver.velocity_gradients: solves that run at once on translated handles), the
    three x derivatives then once more by recorded tds_solve calls; slot 6 (read only) and slot 2 (updated in place) each
    share their buffer with a block outside the call"""
    import torch
    from x3d2_amd import make_channel
    from x3d2_amd.les import Les, LesConfig
    dims = (24, 33, 16)
    out = {}
    for lazy in (False, True):
        case = make_channel(dims, fused=False, poisson="CG", lazy=lazy)
        s = case.solver
        b = s.backend
        set_fields(case, 21)
        les = Les(s, LesConfig(model=model))
        by_r, by_w, extra = blocks_of(b, arrays_of(dims, 3, 22))
        grads = s.velocity_gradients()
        b.vecadd(0.5, s.v, 1.0, s.u)
        b.field_scale(s.w, 1.25)
        for k, f in zip((0, 3, 6), (s.u, s.v, s.w)):  # the x derivatives again, of the updated velocity: recorded solves
            b.tds_solve(grads[k], f, s.xdirps.der1st)
        b.veccopy(by_r, grads[6])
        b.veccopy(by_w, grads[2])
        m0 = materialised(b)
        les.stress(grads)
        m1 = materialised(b)
        b.vecadd(1.0, grads[3], 1.0, extra)
        named = dict(by_r=by_r, by_w=by_w, extra=extra, u=s.u, v=s.v, w=s.w)
        named.update({"g%d" % k: g for k, g in enumerate(grads)})
        o = read(b, named)
        torch.cuda.synchronize()
        o["row"] = les.row.cpu().numpy()
        out[lazy] = o
        if lazy:
            st = report("les_stress " + model, b)
            assert st["recorded"] > 0 and m1 - m0 >= 1, (st, m0, m1)
    same_bits(model, out[False], out[True])
    e = out[False]
    assert np.array_equal(e["g6"], e["by_r"]) and not np.array_equal(e["g2"], e["by_w"])  # by_w holds dudz, g2 tau_13
    assert np.all(e["row"] > 0.0) and np.all(e["g3"] >= 0.0) and np.any(e["g3"] > 0.0)


# ---------------------------------------------------------------- 5. x3d_particles_prime / _advance / _interpolate
@pytest.mark.parametrize("inertial", [False, True], ids=["tracer", "inertial"])
@pytest.mark.parametrize("order", [2, 4])
def test_particles_behind_queued_updates_with_u_an_alias(order, inertial):
    from x3d2_amd import make_tgv
    from x3d2_amd.particles import Particles, ParticlesConfig, by_id, seed_uniform
    dims = (20, 12, 16)
    out = {}
    for lazy in (False, True):
        case = make_tgv(dims, L=(2.0 * np.pi, np.pi, 3.0), poisson="CG", fused=False, lazy=lazy)
        s = case.solver
        b = s.backend
        set_fields(case, 31)
        src1, src2, src3 = blocks_of(b, arrays_of(dims, 3, 32))
        x0 = seed_uniform(s.mesh, 300, seed=5)
        assert 2.0 * s.dt < 0.05
        cfg = ParticlesConfig(x0, order=order, tau_p=0.05 if inertial else 0.0, gravity=(0.0, 0.0, -0.3) if inertial else (0.0,) * 3)

        def queue(src):
            b.vecadd(0.5, s.w, 1.0, s.v)
            b.vecmult(s.w, src)
            b.field_scale(s.v, 1.25)
            b.veccopy(s.u, src)  # u: another name of src's buffer

        o = {}
        queue(src1)
        p = Particles(s, cfg)    # (primes from the solver's fields)
        rows, id_, _, _ = p.raw_state()
        (o["primed"],) = by_id(id_, rows)
        queue(src2)
        p.advance(s.u, s.v, s.w, 0.01)
        queue(src3)
        p.advance(s.u, s.v, s.w, 0.01)
        rows, id_, status, hist = p.raw_state()
        o["rows"], o["status"] = by_id(id_, rows, status)
        assert hist and np.all(status == 1)
        queue(src1)
        o["interp"] = p.interpolate(seed_uniform(s.mesh, 64, seed=6), s.u, s.v, s.w)
        b.vecadd(1.0, s.u, 1.0, src2)
        o.update(read(b, dict(u=s.u, v=s.v, w=s.w, src1=src1, src2=src2, src3=src3)))
        out[lazy] = o
        if lazy:
            assert report("particles order %d %s" % (order, "inertial" if inertial else "tracer"), b)["recorded"] > 0
    same_bits("particles", out[False], out[True])
    e = out[False]
    assert e["rows"].shape[0] == (18 if inertial else 12) and not np.array_equal(e["rows"][:3], e["primed"][:3])
    assert np.all(np.isfinite(e["rows"])) and np.all(e["interp"] != 0.0)


# ---------------------------------------------------------------- 6. x3d_snapshot_pack
def test_snapshot_pack_behind_a_queue_writes_the_same_file_and_moves_no_field(tmp_path):
    """u, a species, |omega|, Q and the vertex pressure, every other / every third point: up to nine translated sources per
    variable, all temporaries of the queue's making"""
    from x3d2_amd import make_tgv
    from x3d2_amd.common import VERT
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots, load_snapshot
    n, out = 32, {}
    for lazy in (False, True):
        case = make_tgv(n, fused=False, lazy=lazy, n_species=1, pr_species=[0.7])
        s = case.solver
        b, m = s.backend, s.mesh
        x, y, z = m.vert_coords[0][None, None, :], m.vert_coords[1][None, :, None], m.vert_coords[2][:, None, None]
        s.species[0].set_data_loc(VERT)
        b.set_field_data(s.species[0], np.cos(x) * np.sin(y) * np.cos(2 * z) + 0.3)
        prefix = str(tmp_path / ("lazy" if lazy else "eager"))
        snap = Snapshots(s, SnapshotConfig(snapshot_freq=1, snapshot_prefix=prefix, output_stride=(2, 1, 3),
                                           output_fields=("pressure", "vorticity", "qcriterion", "species")))
        # ... and one of u, v, w and the species alone: no operator runs between the queue and its pack
        plain = Snapshots(s, SnapshotConfig(snapshot_freq=1, snapshot_prefix=prefix + "_plain", output_stride=(3, 2, 1),
                                            output_fields=("species",)))
        case.step(1)  # (leaves the pressure of its last sub-step)
        by, src, extra = blocks_of(b, arrays_of((n, n, n), 3, 41))
        b.vecadd(0.5, s.v, 1.0, s.u)
        b.field_scale(s.w, 1.25)
        b.veccopy(s.species[0], src)  # the species' data live in another block's buffer
        solver_fields = dict(u=s.u, v=s.v, w=s.w, phi=s.species[0], p=s.pressure)
        before = read(b, solver_fields)
        b.veccopy(by, s.u)            # recorded: u shares its buffer when the snapshot is taken
        b.vecmult(extra, s.v)
        assert plain.write(1) and snap.write(1)
        plain.finalise()
        snap.finalise()
        after = read(b, solver_fields)
        same_bits("the solver's fields across the snapshot", before, after)
        o = {k: v for k, v in load_snapshot(prefix, 1).items() if k != "vtk.xml"}
        o.update({"plain_" + k: v for k, v in load_snapshot(prefix + "_plain", 1).items() if k != "vtk.xml"})
        assert np.array_equal(o["plain_phi_1"], after["phi"][:, ::2, ::3]) and np.array_equal(o["plain_w"], after["w"][:, ::2, ::3])
        assert sorted(k for k in o if o[k].ndim == 3 and not k.startswith("plain_")) == ["p", "phi_1", "qcrit", "u", "v", "vort", "w"]
        assert o["u"].shape == (11, 32, 16) and np.array_equal(o["u"], after["u"][::3, :, ::2])
        o.update(read(b, dict(by=by, src=src, extra=extra)))
        o.update({"field_" + k: v for k, v in after.items()})
        out[lazy] = o
        if lazy:
            assert report("snapshot_pack", b)["recorded"] > 0
    same_bits("snapshot", out[False], out[True])
    e = out[False]
    assert np.all(e["vort"] >= 0.0) and np.any(e["vort"] > 0.0) and np.any(e["p"] != 0.0) and np.any(e["qcrit"] != 0.0)
    assert np.array_equal(e["phi_1"], e["src"][::3, :, ::2])


# ---------------------------------------------------------------- 7. x3d_probe_sample
def test_probes_update_behind_queued_calls(tmp_path):
    from test_hip_loads import Stub, probe_points
    from x3d2_amd.probes import Probes, ProbesConfig
    dims = (33, 16, 8)
    out = {}
    for lazy in (False, True):
        b = make_backend(dims, lazy=lazy)
        s = Stub(b)
        pts, idx = probe_points(b.mesh)  # the first and the last vertex of every axis among them
        pr = Probes(s, ProbesConfig(pts, prefix=str(tmp_path / ("p%d" % lazy)), flush_every=2))
        a = arrays_of(dims, 4, 51)
        for f, x in zip((s.u, s.v, s.w), a):
            f.fill(0.0)
            b.set_field_data(f, x)
        (src,) = blocks_of(b, a[3:])
        for it in range(1, 4):
            b.vecadd(0.5, s.v, 1.0, s.u)
            b.vecmult(s.w, s.u)
            b.field_scale(s.v, 1.25)
            b.veccopy(s.w if it == 2 else src, src if it == 2 else s.u)  # u shares its buffer; w lives in src's
            assert pr.update(it)
            pr.poll()
        b.vecadd(1.0, s.u, 1.0, src)
        pr.finalise()
        o = read(b, dict(u=s.u, v=s.v, w=s.w, src=src))
        o["rows"] = pr.raw_rows()
        out[lazy] = o
        if lazy:
            assert report("probe_sample", b)["recorded"] > 0
    same_bits("probes", out[False], out[True])
    e = out[False]
    assert e["rows"].shape == (3, 21) and len({r.tobytes() for r in e["rows"]}) == 3 and np.all(e["rows"] != 0.0)


# ================================================================ Layer 2
def counting(b, names):
    """wrap the named backend methods of this one backend so that their calls are counted"""
    calls = {n: 0 for n in names}
    for n in names:
        inner = getattr(b, n)

        def wrapped(*a, _inner=inner, _n=n, **kw):
            calls[_n] += 1
            return _inner(*a, **kw)

        setattr(b, n, wrapped)
    return calls


def fields_of(case):
    s = case.solver
    s.flush_grad()
    named = dict(u=s.u, v=s.v, w=s.w)
    named.update({"phi_%d" % (k + 1): f for k, f in enumerate(s.species)})
    return read(s.backend, named)


def worst_ulp(eager, other):
    """max over the fields of max|x - y| / (2^-52 max(max|y|, 1)): the measure of tests/test_hip_lazy.py"""
    return max(float(np.max(np.abs(eager[k] - other[k])) / (2.0 ** -52 * max(np.max(np.abs(eager[k])), 1.0))) for k in eager)


def check_engaged(label, st, bare, nsub, in_place_calls):
    """the layer did not fall back to call by call around the add-on; both sides counted on the spot"""
    print("engagement %-28s materialised %d (bare %d)  declined %d (bare %d)  in-place add-on calls %d"
          % (label, st["materialised"], bare["materialised"], st["declined"], bare["declined"], in_place_calls))
    assert st["transeq_acc"] + st["transeq_stage"] == 2 * nsub, st
    assert st["solve_000"] == nsub, st
    assert st["pairs"] == bare["pairs"], (st, bare)
    assert st["sync_copies"] == 0, st
    assert st["materialised"] <= bare["materialised"] + in_place_calls, (st, bare)
    assert st["declined"] <= bare["declined"] + in_place_calls, (st, bare)


# ---------------------------------------------------------------- TGV 32^3 with scalars, particles, snapshots, probes
def TGV_PHI(x, y, z):
    return np.cos(x) * np.sin(y) * np.cos(2 * z) + 0.3


def tgv_case(time_intg, lazy, where=None, checkpoint_freq=0):
    """where = None: the bare case"""
    from x3d2_amd import make_tgv
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints
    from x3d2_amd.particles import Particles, ParticlesConfig, seed_uniform
    from x3d2_amd.probes import Probes, ProbesConfig
    from x3d2_amd.scalars import Scalars, ScalarsConfig
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots
    case = make_tgv(32, time_intg=time_intg, fused=False, lazy=lazy, n_species=1, pr_species=[0.7])
    s = case.solver
    if where is None:
        set_species(s, TGV_PHI)
        return case
    where.mkdir(exist_ok=True)
    case.calls = counting(s.backend, ("scalars_couple", "scalars_apply_bc"))
    s.scalars = Scalars(s, ScalarsConfig(ri=[0.4], ref=[0.3], up=(0.0, 0.6, 0.8), grad=[(0.3, -0.2, 0.1)],
                                         init=[TGV_PHI], profile_dir=3, initstat=1))
    case.particles = Particles(s, ParticlesConfig(seed_uniform(s.mesh, 256, seed=3), order=4, tau_p=0.05,
                                                  gravity=(0.0, 0.0, -0.3), sort_every=2))
    case.snapshots = Snapshots(s, SnapshotConfig(snapshot_freq=1, snapshot_prefix=str(where / "snapshot"), output_stride=(2, 2, 2),
                                                 output_fields=("pressure", "vorticity", "qcriterion", "species")))
    c = [np.asarray(a) for a in s.mesh.vert_coords]
    pts = [[c[0][0], c[1][5], c[2][7]], [c[0][-1], c[1][9], c[2][2]], [c[0][3], c[1][0], c[2][11]], [c[0][8], c[1][-1], c[2][4]],
           [c[0][13], c[1][6], c[2][0]], [c[0][21], c[1][17], c[2][-1]], [c[0][16] + 0.01, c[1][16] - 0.02, c[2][16] + 0.03]]
    case.probes = Probes(s, ProbesConfig(pts, prefix=str(where / "probes"), flush_every=4))
    if checkpoint_freq:
        case.checkpoints = Checkpoints(s, CheckpointConfig(checkpoint_freq=checkpoint_freq,
                                                           checkpoint_prefix=str(where / "checkpoint")), case)
    return case


def tgv_outputs(case, snapshots=()):
    """everything the add-ons leave, as one dict of host arrays"""
    from x3d2_amd.particles import by_id
    from x3d2_amd.snapshot import load_snapshot
    s = case.solver
    o = fields_of(case)
    o.update({"mean_" + k: np.asarray(v) for k, v in s.scalars.profiles().items()})
    rows, id_, status, hist = case.particles.raw_state()
    o["particle_rows"], o["particle_status"] = by_id(id_, rows, status)
    o["particle_hist"] = np.array(hist)
    o["probe_rows"] = case.probes.raw_rows()
    for it in snapshots:
        snap = load_snapshot(case.snapshots.cfg.snapshot_prefix, it)
        o.update({"snapshot%d_%s" % (it, k): v for k, v in snap.items() if k != "vtk.xml"})
    o.update({"monitor_" + k: np.asarray(v) for k, v in s.scalars.monitor().items()})  # (last: it takes a sample of its own)
    return o


@pytest.mark.parametrize("time_intg", ["RK3", "AB3"])
def test_tgv_steps_with_scalars_particles_snapshots_probes_are_bit_identical(time_intg, tmp_path):
    out = {}
    for lazy in (False, True):
        case = tgv_case(time_intg, lazy, tmp_path / ("lazy" if lazy else "eager"))
        case.run(n_iters=2)
        out[lazy] = tgv_outputs(case, snapshots=(1, 2))
        if lazy:
            st, calls = report("tgv %s with add-ons" % time_intg, case.solver.backend), case.calls
            nsub = 2 * case.solver.time_integrator.nstage
    same_bits("tgv " + time_intg, out[False], out[True])
    e = out[False]
    assert e["probe_rows"].shape == (2, 21) and e["mean_count"] == 2 and np.all(e["particle_status"] == 1)
    assert np.any(e["snapshot2_p"] != 0.0) and np.any(e["mean_wphi"] != 0.0)
    bare = tgv_case(time_intg, True)
    bare.run(n_iters=2)
    assert calls["scalars_couple"] == nsub and calls["scalars_apply_bc"] == 0  # (no wall: nothing to stamp)
    check_engaged("tgv " + time_intg, st, report("tgv %s bare" % time_intg, bare.solver.backend), nsub, calls["scalars_couple"])


# ---------------------------------------------------------------- restart
def test_deferred_restart_with_the_addons_equals_the_uninterrupted_deferred_run(tmp_path):
    """AB3, deferred: checkpoint after step 2, restore into a fresh deferred case with the same add-ons, steps 3-4.
    x3d_checkpoint_unpack writes with full = true onto handles; the species, the profile means and the particle state go
    through that path with the mode on"""
    from x3d2_amd.checkpoint import restore
    whole = tgv_case("AB3", True, tmp_path / "whole")
    whole.run(n_iters=4)
    first = tgv_case("AB3", True, tmp_path / "first", checkpoint_freq=2)
    first.run(n_iters=2)
    again = tgv_case("AB3", True, tmp_path / "again")
    assert restore(again, str(tmp_path / "first" / "checkpoint_000002.npz")) == 2 and again.restarted
    again.run(n_iters=4)
    a, c = tgv_outputs(whole, snapshots=(3, 4)), tgv_outputs(again, snapshots=(3, 4))
    a["probe_rows"] = a["probe_rows"][2:]  # (the restarted series starts at step 3)
    same_bits("restart", a, c)
    assert c["mean_count"] == 4 and c["probe_rows"].shape == (2, 21)
    report("restarted run", again.solver.backend)


# ---------------------------------------------------------------- channel (32, 33, 24), stretched, RK3
CHANNEL = dict(stretching="top-bottom", beta=BETA, fused=False, rotation=True, omega_rot=0.12, n_rotate=2)
CHANNEL_DIMS = (32, 33, 24)


def CHANNEL_PHI(x, y, z):
    return 1.0 - y / 2.0 + 0.05 * np.sin(2.0 * x) * np.cos(3.0 * z)


def channel_scalars_case(lazy, addon=True):
    from x3d2_amd import make_channel
    from x3d2_amd.scalars import Scalars, ScalarsConfig
    case = make_channel(CHANNEL_DIMS, lazy=lazy, n_species=1, pr_species=[0.71], **CHANNEL)
    s = case.solver
    if addon:
        case.calls = counting(s.backend, ("scalars_couple", "scalars_apply_bc"))
        s.scalars = Scalars(s, ScalarsConfig(ri=[0.1], up=(0.0, 1.0, 0.0), wall=[{"y": (1.0, 0.0)}],
                                             init=[CHANNEL_PHI], profile_dir=2, initstat=1))
    else:
        set_species(s, CHANNEL_PHI)
    return case


def scalar_outputs(case):
    s = case.solver
    o = {"mean_" + k: np.asarray(v) for k, v in s.scalars.profiles().items()}
    o.update({"monitor_" + k: np.asarray(v) for k, v in s.scalars.monitor().items()})
    return o


def test_channel_steps_with_scalars(monkeypatch):
    """y wall values, buoyancy along y, profiles along y.  Default rules: fields within 16 ulp of the field maximum (measured on
    an MI355X: 1.627, printed at every run); X3D_LAZY_RULES=255-2-4-8: fields and every scalar output bit for bit"""
    eager = channel_scalars_case(False)
    eager.run(n_iters=2)
    fe, se = fields_of(eager), scalar_outputs(eager)
    lazy = channel_scalars_case(True)
    lazy.run(n_iters=2)
    st, calls = report("channel + scalars", lazy.solver.backend), lazy.calls
    worst = worst_ulp(fe, fields_of(lazy))
    print("channel + scalars, default rules: worst distance %.3f ulp of the field maximum (bound 16)" % worst)
    bare = channel_scalars_case(True, addon=False)
    bare.run(n_iters=2)
    bare_st = report("channel bare (one species)", bare.solver.backend)
    monkeypatch.setenv("X3D_LAZY_RULES", RULES_EXACT)
    exact = channel_scalars_case(True)
    exact.run(n_iters=2)
    report("channel + scalars, rules %s" % RULES_EXACT, exact.solver.backend)
    same_bits("channel + scalars without the reassociating rewrites", dict(fe, **se), dict(fields_of(exact), **scalar_outputs(exact)))
    assert worst <= 16.0
    nsub = 2 * lazy.solver.time_integrator.nstage
    assert calls["scalars_couple"] == nsub and calls["scalars_apply_bc"] == nsub + 1  # (+ 1: the initial values' walls)
    check_engaged("channel + scalars", st, bare_st, nsub, calls["scalars_couple"] + calls["scalars_apply_bc"])
    assert np.all(fe["phi_1"][:, 0, :] == 1.0) and np.all(fe["phi_1"][:, -1, :] == 0.0) and se["mean_count"] == 2
    assert np.all(np.isfinite(se["monitor_nu_vol"]))


def channel_les_case(lazy, addon=True):
    from x3d2_amd import make_channel
    from x3d2_amd.les import Les, LesConfig
    case = make_channel(CHANNEL_DIMS, lazy=lazy, **CHANNEL)
    s = case.solver
    # a three-dimensional start that vanishes on the walls: WALE's eddy viscosity is zero in the pure shear of the case's own
    m = s.mesh
    x, y, z = (np.asarray(m.vert_coords[0])[None, None, :], np.asarray(m.vert_coords[1])[None, :, None] - 1.0,
               np.asarray(m.vert_coords[2])[:, None, None])
    kx, kz, env = 2.0 * np.pi / m.L[0], 2.0 * np.pi / m.L[2], 1.0 - y * y
    env[:, [0, -1], :] = 0.0
    for f, a in zip((s.u, s.v, s.w), (env * (1.0 + 0.3 * np.sin(kx * x) * np.cos(kz * z)), 0.2 * env * np.sin(2 * kx * x) * np.sin(kz * z),
                                      0.2 * env * np.cos(kx * x) * np.sin(2 * kz * z))):
        s.backend.set_field_data(f, a + 0.0 * (x + z))
    if addon:
        case.calls = counting(s.backend, ("les_stress",))
        s.les = Les(s, LesConfig(model="wale"))
    return case


def les_row(case):
    import torch
    torch.cuda.synchronize()
    return {"les_row": case.solver.les.row.cpu().numpy()}


def test_channel_steps_with_wale(monkeypatch):
    """the subgrid term between transeq and the stage.  Default rules: fields within 16 ulp of the field maximum (measured on an
    MI355X: 2.008, printed at every run; max nu_t 1.9e-3 on the three-dimensional start); X3D_LAZY_RULES=255-2-4-8: fields and
    Les.row bit for bit.  Les.add forms its gradients and adds its nine derivatives through x3d_tds_solve_acc, which
    runs at once: sync_copies == 0 holds since that entry point translates its two handles (it restored the identity map
    before: 35 block copies in these two steps)"""
    eager = channel_les_case(False)
    eager.run(n_iters=2)
    fe, re_ = fields_of(eager), les_row(eager)
    lazy = channel_les_case(True)
    lazy.run(n_iters=2)
    st, calls = report("channel + wale", lazy.solver.backend), lazy.calls
    worst = worst_ulp(fe, fields_of(lazy))
    print("channel + wale, default rules: worst distance %.3f ulp of the field maximum (bound 16)" % worst)
    row_lazy = les_row(lazy)["les_row"]
    print("channel + wale, default rules: Les.row eager %s deferred %s" % (re_["les_row"], row_lazy))
    bare = channel_les_case(True, addon=False)
    bare.run(n_iters=2)
    bare_st = report("channel bare", bare.solver.backend)
    monkeypatch.setenv("X3D_LAZY_RULES", RULES_EXACT)
    exact = channel_les_case(True)
    exact.run(n_iters=2)
    report("channel + wale, rules %s" % RULES_EXACT, exact.solver.backend)
    same_bits("channel + wale without the reassociating rewrites", dict(fe, **re_), dict(fields_of(exact), **les_row(exact)))
    assert worst <= 16.0
    nsub = 2 * lazy.solver.time_integrator.nstage
    assert calls["les_stress"] == nsub and np.all(re_["les_row"] > 0.0)
    check_engaged("channel + wale", st, bare_st, nsub, calls["les_stress"])
