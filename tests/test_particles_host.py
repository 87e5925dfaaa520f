"""Host side of the particles (x3d2_amd/particles.py) and the numpy restatement the GPU tests compare with
(tests/particles_ref.py): the restatement is checked against what the rules must give (partition of unity, polynomial
reproduction, the cell rule at its edge cases, wrap and reflect arithmetic, the AB2 coefficients, the self-consistency of one
update), then the configuration errors, the file round trip and the checkpoint dictionary.  No GPU."""
import numpy as np
import pytest

import particles_ref as ref
from x3d2_amd import Mesh
from x3d2_amd.common import X3dError
from x3d2_amd.particles import (Particles, ParticlesConfig, ab2_coefficients, by_id, check_state_dict, file_name,  # noqa: F401
                                load_particles, seed_uniform, unpack)

PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2


def channel_mesh():
    """make_channel((24, 33, 16))'s mesh: periodic x and z, y stretched towards its walls"""
    return Mesh((24, 33, 16), (1, 1, 1), (4.0, 2.0, 2.0), PER, WALL, PER, ("uniform", "top-bottom", "uniform"),
                (1.0, 0.259065151, 1.0))


def box_mesh():
    return Mesh((20, 12, 16), (1, 1, 1), (2 * np.pi, np.pi, 3.0), PER, PER, PER)


def cylinder_mesh():
    return Mesh((33, 16, 8), (1, 1, 1), (20.0, 12.0, 6.0), WALL, PER, PER)


MESHES = {"box": box_mesh, "channel": channel_mesh, "cylinder": cylinder_mesh}


def special_points(axes, rng):
    """hand-placed coordinates per direction: first / last cell, the periodic wrap cell, vertices, x = L, next to a wall, on it"""
    cols = []
    for ax in axes:
        c = ax.c
        pts = [0.5 * (c[0] + c[1]), 0.5 * (c[-2] + c[-1]), c[0], c[1], c[ax.n // 2], c[-1], c[1] + 0.25 * (c[2] - c[1]),
               c[-2] - 0.25 * (c[-2] - c[-3])]
        if ax.periodic:
            pts += [0.5 * (c[-1] + ax.L), c[-1] + 0.9 * (ax.L - c[-1]), ax.L, np.nextafter(ax.L, 0.0)]
        else:
            pts += [ax.lo, ax.hi, np.nextafter(ax.hi, ax.lo), np.nextafter(ax.lo, ax.hi)]
        cols.append(np.array(pts))
    m = max(len(c) for c in cols)
    out = np.empty((3 * m, 3))
    for d, ax in enumerate(axes):  # every special value of a direction with random partners in the other two
        lo, hi = (0.0, ax.L) if ax.periodic else (ax.lo, ax.hi)
        out[:, d] = lo + (hi - lo) * rng.random(3 * m) * 0.999
    for d in range(3):
        out[d * m:d * m + len(cols[d]), d] = cols[d]
    return out


@pytest.mark.parametrize("name", sorted(MESHES))
@pytest.mark.parametrize("order", [2, 4])
def test_weights_sum_to_one_and_nodes_bracket_the_point(name, order):
    axes = ref.axes_of(MESHES[name]())
    rng = np.random.default_rng(3)
    pts = np.vstack([seed_uniform(MESHES[name](), 500, seed=4), special_points(axes, rng)])
    for d, ax in enumerate(axes):
        x = ref.wrap(pts[:, d], ax.L) if ax.periodic else pts[:, d]
        idx, xi = ref.nodes(ax, x, order)
        w = ref.weights(xi, x, order)
        assert np.max(np.abs(w.sum(axis=1) - 1.0)) < 1e-13
        assert idx.min() >= 0 and idx.max() < ax.n
        assert np.all(np.diff(xi, axis=1) > 0.0)  # ascending, also through the periodic wrap
        assert np.all((xi[:, 0] <= x) & (x <= xi[:, -1]))  # never extrapolates


@pytest.mark.parametrize("name", ["channel", "cylinder"])
def test_order_4_reproduces_cubics_on_stretched_and_one_sided_stencils(name):
    """a polynomial of degree 3 in each variable comes back to 1e-13 (of its size), in the non-periodic directions where
    it is well defined: the stretched y of the channel, the x of the cylinder, points next to and on the walls included"""
    mesh = MESHES[name]()
    axes = ref.axes_of(mesh)
    d = 1 if name == "channel" else 0
    ax = axes[d]

    def poly(t):
        s = (t - ax.lo) / (ax.hi - ax.lo)
        return 1.0 + s - 2.0 * s * s + 0.5 * s * s * s

    shape = [1, 1, 1]
    shape[2 - d] = ax.n
    f = np.broadcast_to(poly(ax.c).reshape(shape), (axes[2].n, axes[1].n, axes[0].n))
    rng = np.random.default_rng(5)
    pts = np.vstack([seed_uniform(mesh, 400, seed=6), special_points(axes, rng)])
    got = ref.interpolate(axes, [f], pts, 4)[:, 0]
    err = float(np.max(np.abs(got - poly(pts[:, d]))))
    print("cubic along one direction, %s: err %.3e  bound %.3e" % (name, err, 1e-13 * float(np.max(np.abs(poly(ax.c))))))
    assert err <= 1e-13 * float(np.max(np.abs(poly(ax.c))))
    # ... and the restatement's own two switches bite: without the one-sided shift the wall cells are wrong
    near = pts[:, d] < ax.c[1]
    assert near.any()
    idx, xi = ref.nodes(ax, pts[near, d], 4, shift_stencil=False)
    assert np.any(np.diff(xi, axis=1) <= 0.0)  # (clipped indices: a repeated node)


@pytest.mark.parametrize("name", ["channel", "cylinder", "box"])
def test_order_4_reproduces_a_field_cubic_in_x_y_and_z_at_once(name):
    """the three-direction tensor product of the restatement (the fancy indexing, the order of the three sums) against the
    closed form: f = p_x(x) p_y(y) p_z(z) with three different cubics comes back to 1e-13 max|f|.  A cubic is not periodic,
    so in a periodic direction the points keep to the cells whose four nodes do not wrap, [c[1], c[n - 2]); a walled
    direction is covered whole, the one-sided stencils next to the walls and the walls themselves included."""
    mesh = MESHES[name]()
    axes = ref.axes_of(mesh)
    coef = [(0.3, 1.0, -0.7, 0.4), (1.0, -0.5, 0.25, 0.6), (-0.2, 0.8, 0.5, -0.9)]

    def poly(d, t):
        s = t / axes[d].L
        a, b, c, e = coef[d]
        return a + b * s + c * s * s + e * s * s * s

    px, py, pz = (poly(d, axes[d].c) for d in range(3))
    f = pz[:, None, None] * py[None, :, None] * px[None, None, :]
    rng = np.random.default_rng(11)
    pts = np.vstack([seed_uniform(mesh, 600, seed=12), special_points(axes, rng)])
    for d, ax in enumerate(axes):
        if ax.periodic:
            lo, hi = ax.c[1], ax.c[ax.n - 2]
            pts[:, d] = lo + (hi - lo) * rng.random(pts.shape[0]) * 0.999
            pts[0, d], pts[1, d] = lo, ax.c[ax.n - 3]  # (on the first and the last vertex that is allowed)
    want = poly(0, pts[:, 0]) * poly(1, pts[:, 1]) * poly(2, pts[:, 2])
    got = ref.interpolate(axes, [f, 2.0 * f], pts, 4)
    fmax = float(np.max(np.abs(f)))
    err = float(np.max(np.abs(got[:, 0] - want)))
    print("cubic in x, y and z, %s: err %.3e  bound %.3e" % (name, err, 1e-13 * fmax))
    assert err <= 1e-13 * fmax
    assert np.array_equal(got[:, 1], 2.0 * got[:, 0])  # (the second field goes the same way)
    # the directions are not interchangeable in f: a transposed indexing would not pass
    swapped = ref.interpolate(axes, [np.ascontiguousarray(f[:, ::-1, :])], pts, 4)[:, 0]
    assert float(np.max(np.abs(swapped - want))) > 1e-3 * fmax


def test_order_4_reproduces_cubics_through_the_periodic_wrap_only_with_wrapped_coordinates():
    ax = ref.Axis(np.arange(8) * 0.5, 4.0, True)
    x = np.array([3.6, 3.9, 0.1, 0.45])  # the wrap cell and the first cell: stencils reach across
    idx, xi = ref.nodes(ax, x, 4)
    assert idx.tolist() == [[6, 7, 0, 1], [6, 7, 0, 1], [7, 0, 1, 2], [7, 0, 1, 2]]
    assert np.allclose(xi[0], [3.0, 3.5, 4.0, 4.5]) and np.allclose(xi[2], [-0.5, 0.0, 0.5, 1.0])
    w = ref.weights(xi, x, 4)
    g = lambda t: 0.3 + t - 0.2 * t ** 2 + 0.05 * t ** 3  # noqa: E731  (values taken at the UNWRAPPED node coordinates)
    assert np.max(np.abs((w * g(xi)).sum(axis=1) - g(x))) < 1e-13
    _, bad = ref.nodes(ax, x, 4, wrap_coords=False)
    assert np.max(np.abs((ref.weights(bad, x, 4) * g(xi)).sum(axis=1) - g(x))) > 1e-2


def test_cell_rule_on_vertices_at_L_and_in_the_wrap_cell():
    per = ref.Axis(np.arange(8) * 0.5, 4.0, True)
    assert ref.cell(per, np.array([0.0, 0.5, 0.49999, 3.5, 3.75, np.nextafter(4.0, 0.0)])).tolist() == [0, 1, 0, 7, 7, 7]
    assert ref.wrap(np.array([4.0, -0.0, 8.0, -4.0, 4.25, -0.25]), 4.0).tolist() == [0.0, 0.0, 0.0, 0.0, 0.25, 3.75]
    assert ref.wrap(np.array([-1e-300]), 4.0).tolist() == [0.0]  # (x + L rounds to L: becomes 0)
    wall = ref.Axis(np.array([0.0, 0.1, 0.3, 0.6, 1.0]), 1.0, False)
    assert ref.cell(wall, np.array([0.0, 0.1, 0.29, 0.6, 0.99, 1.0])).tolist() == [0, 1, 1, 3, 3, 3]  # the wall itself: n - 2
    idx, _ = ref.nodes(wall, np.array([0.05, 0.2, 0.7, 1.0]), 4)
    assert idx.tolist() == [[0, 1, 2, 3], [0, 1, 2, 3], [1, 2, 3, 4], [1, 2, 3, 4]]
    idx, _ = ref.nodes(wall, np.array([0.05, 1.0]), 2)
    assert idx.tolist() == [[0, 1], [3, 4]]


def test_wrap_reflect_and_absorb_arithmetic():
    axes = [ref.Axis(np.arange(4) * 1.0, 4.0, True), ref.Axis(np.array([0.0, 0.5, 1.5, 2.0]), 2.0, False),
            ref.Axis(np.arange(4) * 1.0, 4.0, True)]
    x = np.array([[4.5, -0.25, -0.5], [1.0, 2.125, 3.0], [1.0, 1.0, 1.0], [1.0, -2.5, 1.0]])
    v = np.array([[1.0, -2.0, 3.0]] * 4)
    xr, vr, absorbed, reflected, clamped = ref.boundaries(axes, x, v, "reflect")
    assert xr.tolist() == [[0.5, 0.25, 3.5], [1.0, 1.875, 3.0], [1.0, 1.0, 1.0], [1.0, 2.0, 1.0]]
    assert vr[:, 1].tolist() == [2.0, 2.0, -2.0, 2.0] and np.array_equal(vr[:, [0, 2]], v[:, [0, 2]])
    assert reflected.tolist() == [True, True, False, True] and clamped.tolist() == [False, False, False, True]
    assert not absorbed.any()
    xa, va, absorbed, reflected, _ = ref.boundaries(axes, x, v, "absorb")
    assert xa[:, 1].tolist() == [0.0, 2.0, 1.0, 0.0] and np.array_equal(va, v)
    assert absorbed.tolist() == [True, True, False, True] and not reflected.any()


def test_ab2_coefficients_first_and_later():
    assert ab2_coefficients(True) == (1.0, 0.0) == ref.ab2(True)
    assert ab2_coefficients(False) == (1.5, -0.5) == ref.ab2(False)


@pytest.mark.parametrize("tau", [0.0, 0.1])
def test_one_update_of_the_restatement_is_self_consistent(tau):
    """in a uniform flow U the exact path is known: tracers move by U dt per step whatever (c1, c0); inertial particles
    starting at the fluid's velocity with g = 0 do the same; with g they follow AB2 on dv/dt = -(v - U) / tau + g"""
    mesh = channel_mesh()
    axes = ref.axes_of(mesh)
    U = np.array([0.7, 0.0, -0.3])
    shape = (axes[2].n, axes[1].n, axes[0].n)
    fields = [np.full(shape, U[c]) for c in range(3)]
    x0 = seed_uniform(mesh, 50, seed=2)
    x0[:, 1] = 0.5 + x0[:, 1] * 0.5
    dt, g = 5e-3, (0.0, -0.5, 0.0)
    st = ref.prime(axes, fields, x0, 4, tau, g)
    assert np.allclose(st["a"], U[None, :], rtol=0, atol=1e-14) and np.array_equal(st["v"], st["a"])
    x, v, first = st["x"].copy(), st["v"].copy(), True
    F = (U[None, :] - v) / tau + np.asarray(g)[None, :] if tau else None
    v_prev, F_prev = v.copy(), None if F is None else F.copy()
    for step in range(3):
        c1, c0 = ref.ab2(first)
        st, info = ref.update(axes, fields, st, dt, 4, first, tau, g)
        x_new = x + dt * (c1 * v + c0 * v_prev)
        if tau:
            v_new = v + dt * (c1 * F + c0 * F_prev)
            F_prev, F = F, (U[None, :] - v_new) / tau + np.asarray(g)[None, :]
        else:
            v_new = np.broadcast_to(U, v.shape).copy()
        v_prev, v, x, first = v, v_new, x_new, False
        want = x.copy()
        for d in (0, 2):
            want[:, d] = ref.wrap(want[:, d], axes[d].L)
        assert not info["reflected"].any() and not info["absorbed"].any()
        assert np.max(np.abs(st["x"] - want)) < 1e-14 and np.max(np.abs(st["v"] - v)) < 1e-14
        assert np.array_equal(st["v_prev"], v_prev) or np.max(np.abs(st["v_prev"] - v_prev)) < 1e-14
        assert np.max(np.abs(st["a"] - U[None, :])) < 1e-14
    dead = {k: val.copy() for k, val in st.items()}
    dead["status"][:10] = 0
    after, _ = ref.update(axes, fields, dead, dt, 4, False, tau, g)
    for k in after:
        assert np.array_equal(after[k][:10], dead[k][:10]), k  # frozen


def test_cell_keys_follow_the_cell_rule():
    axes = ref.axes_of(box_mesh())
    x = np.array([[0.0, 0.0, 0.0], [np.nextafter(2 * np.pi, 0), np.nextafter(np.pi, 0), np.nextafter(3.0, 0)]])
    assert ref.cell_keys(axes, x).tolist() == [0, 20 * 12 * 16 - 1]


# ---------------------------------------------------------------- configuration, files, checkpoint dictionary
def test_every_configuration_error():
    ok = np.zeros((4, 3))
    ParticlesConfig(ok)
    for bad in (np.zeros((0, 3)), np.zeros(3), np.zeros((4, 2)), np.full((4, 3), np.nan), np.full((4, 3), np.inf)):
        with pytest.raises(X3dError):
            ParticlesConfig(bad)
    for kw in (dict(order=3), dict(order=1), dict(tau_p=-1.0), dict(tau_p=float("nan")), dict(gravity=(0, 0)),
               dict(gravity=(0, float("inf"), 0)), dict(wall="stick"), dict(v0=np.zeros((4, 3))),
               dict(tau_p=0.1, v0=np.zeros((3, 3))), dict(tau_p=0.1, v0=np.full((4, 3), np.nan)), dict(ipartout=-1),
               dict(sort_every=-2)):
        with pytest.raises(X3dError):
            ParticlesConfig(ok, **kw)
    cfg = ParticlesConfig(ok, tau_p=0.1, v0=np.ones((4, 3)), ipartout=5, sort_every=2, initpart=3)
    assert cfg.n == 4 and cfg.inertial and cfg.output_due(10) and not cfg.output_due(7)
    assert cfg.sort_due(4) and not cfg.sort_due(5) and not ParticlesConfig(ok).sort_due(4) and not ParticlesConfig(ok).output_due(4)


def test_seed_uniform_stays_inside_and_repeats():
    for name in MESHES:
        mesh = MESHES[name]()
        axes = ref.axes_of(mesh)
        x = seed_uniform(mesh, 1000, seed=1)
        assert x.shape == (1000, 3) and np.array_equal(x, seed_uniform(mesh, 1000, seed=1))
        for d, ax in enumerate(axes):
            lo, hi = (0.0, ax.L) if ax.periodic else (ax.lo, ax.hi)
            assert x[:, d].min() >= lo and (x[:, d].max() < hi if ax.periodic else x[:, d].max() <= hi)


def packed(n, rng):
    rows = rng.normal(size=(9, n))
    ids = rng.permutation(n).astype(np.int32)
    status = rng.integers(0, 3, n).astype(np.int32)
    raw = np.concatenate([rows.reshape(-1).view(np.uint8), ids.view(np.uint8), status.view(np.uint8)])
    return raw, rows, ids, status


def test_unpack_brings_device_order_into_id_order():
    raw, rows, ids, status = packed(37, np.random.default_rng(8))
    out = unpack(raw, 37)
    assert out["id"].tolist() == list(range(37))
    for q in range(37):
        t = int(np.flatnonzero(ids == q)[0])
        assert out["x"][q].tolist() == rows[0:3, t].tolist() and out["v"][q].tolist() == rows[3:6, t].tolist()
        assert out["a"][q].tolist() == rows[6:9, t].tolist() and out["status"][q] == status[t]
        assert out["alive"][q] == int(status[t] == 1)
    a, = by_id(ids, np.arange(37)[ids])
    assert a.tolist() == list(range(37))


def test_npz_round_trip_of_load_particles(tmp_path):
    raw, _, _, _ = packed(11, np.random.default_rng(9))
    out = unpack(raw, 11)
    out["iteration"], out["time"] = np.int64(500), np.float64(0.5)
    prefix = str(tmp_path / "particles")
    assert file_name(prefix, 500).endswith("particles_000500.npz")
    with open(file_name(prefix, 500), "wb") as fh:
        np.savez(fh, **out)
    back = load_particles(prefix, 500)
    assert sorted(back) == sorted(out)
    for k in out:
        assert np.array_equal(back[k], out[k]) and back[k].dtype == np.asarray(out[k]).dtype
    with pytest.raises(X3dError):
        load_particles(prefix, 501)  # no such file
    with open(file_name(prefix, 7), "wb") as fh:
        np.savez(fh, x=out["x"])
    with pytest.raises(X3dError):
        load_particles(prefix, 7)  # not a particle file


def test_state_dict_checks():
    n = 5
    z = {"particles_n": np.int64(n), "particles_order": np.int64(4), "particles_tau_p": np.float64(0.0),
         "particles_iteration": np.int64(3), "particles_has_history": np.bool_(True),
         "particles_rows": np.zeros((12, n)), "particles_status": np.ones(n, dtype=np.int32)}
    check_state_dict(z, n, 4, 0.0)
    for args in ((n + 1, 4, 0.0), (n, 2, 0.0), (n, 4, 0.1)):
        with pytest.raises(X3dError):
            check_state_dict(z, *args)
    with pytest.raises(X3dError, match="holds none"):
        check_state_dict({"timestep": 3}, n, 4, 0.0)
    with pytest.raises(X3dError):
        check_state_dict(dict(z, particles_rows=np.zeros((18, n))), n, 4, 0.0)
    zi = dict(z, particles_tau_p=np.float64(0.1), particles_rows=np.zeros((18, n)))
    check_state_dict(zi, n, 4, 0.1)
