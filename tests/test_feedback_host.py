"""tests/feedback_ref.py, the numpy restatement of the two-way coupling, pinned on the host: dual volumes, weights, conservation,
the cell colouring, and the refusals of ParticlesConfig and of the mesh check.  No GPU."""
import numpy as np
import pytest

import feedback_ref as R
import particles_ref as P
from x3d2_amd import Mesh
from x3d2_amd.common import X3dError
from x3d2_amd.particles import ParticlesConfig, check_two_way, dual_widths, mass_for_loading, seed_uniform

PER, WALL = ("periodic", "periodic"), ("dirichlet", "dirichlet")


def box_mesh(dims=(16, 12, 10)):
    return Mesh(dims, (1, 1, 1), (2 * np.pi, np.pi, 3.0), PER, PER, PER)


def channel_mesh(dims=(16, 17, 8)):
    return Mesh(dims, (1, 1, 1), (4.0, 2.0, 2.0), PER, WALL, PER, ("uniform", "top-bottom", "uniform"), (1.0, 0.259065151, 1.0))


MESHES = {"box": box_mesh, "channel": channel_mesh}


def random_state(mesh, n, seed, dead=0):
    rng = np.random.default_rng(seed)
    x = seed_uniform(mesh, n, seed=seed)
    st = {"x": x, "v": rng.standard_normal((n, 3)), "a": rng.standard_normal((n, 3)), "status": np.ones(n, dtype=np.int32)}
    if dead:
        st["status"][:dead] = np.arange(dead) % 2 * 2  # 0 and 2
        st["v"][:dead] = 1e300
    return st


@pytest.mark.parametrize("name", ["box", "channel"])
def test_dual_volumes_fill_the_domain(name):
    mesh = MESHES[name]()
    axes = P.axes_of(mesh)
    vol = 1.0 / R.inverse_volumes(axes)
    want = float(mesh.L[0]) * float(mesh.L[1]) * float(mesh.L[2])
    assert abs(float(vol.sum()) - want) <= 1e-13 * want
    for d, ax in enumerate(axes):  # the library's own tables are the same numbers
        assert np.array_equal(dual_widths(ax.c, ax.periodic, ax.L), R.dual_widths(ax))
    if name == "channel":
        c, d = axes[1].c, R.dual_widths(axes[1])
        assert d[0] == 0.5 * (c[1] - c[0]) and d[-1] == 0.5 * (c[-1] - c[-2]) and d[3] == 0.5 * (c[4] - c[2])


@pytest.mark.parametrize("name", ["box", "channel"])
def test_weights_sum_to_one_and_lie_in_the_unit_interval(name):
    mesh = MESHES[name]()
    axes = P.axes_of(mesh)
    x = seed_uniform(mesh, 2000, seed=3)
    for d, ax in enumerate(axes):  # vertices, the seam cell and the last vertex of a wall direction
        x[:ax.n, d] = ax.c
        x[ax.n, d] = 0.5 * (ax.c[-1] + (ax.L if ax.periodic else ax.c[-2]))
    i, j, k, w = R.corner_weights(axes, x)
    assert np.max(np.abs(w.sum(axis=1) - 1.0)) <= 4e-16
    assert w.min() >= 0.0 and w.max() <= 1.0
    on_vertex = x[:axes[0].n, 0] == axes[0].c
    assert on_vertex.all() and np.all(R.linear_weights(axes[0], x[:axes[0].n, 0])[1][:, 0] == 1.0)
    assert np.any(i == axes[0].n - 1) and np.all(j <= axes[1].n - (1 if axes[1].periodic else 2))


@pytest.mark.parametrize("name", ["box", "channel"])
def test_the_fluid_receives_minus_the_total_drag(name):
    mesh = MESHES[name]()
    axes = P.axes_of(mesh)
    st = random_state(mesh, 1500, 5, dead=20)
    mass, tau = 0.37, 0.05
    f = R.field(axes, st, mass, tau)
    got, want = R.integral(axes, f), -R.total_drag(st, mass, tau)
    scale = float(np.sum(np.abs(R.drag(st, mass, tau))))
    assert np.max(np.abs(got - want)) <= 1e-12 * scale
    assert np.max(np.abs(want)) > 1e-3 * scale / np.sqrt(1500.0)
    # the particles that are not alive contribute nothing, whatever they hold
    alive = st["status"] == 1
    only = {k: v[alive] for k, v in st.items()}
    g = R.field(axes, only, mass, tau, ids=np.nonzero(alive)[0])
    assert all(np.array_equal(a, b) for a, b in zip(f, g))


@pytest.mark.parametrize("dims,mesh_of", [((16, 12, 10), box_mesh), ((4, 2, 6), box_mesh), ((16, 17, 8), channel_mesh),
                                          ((8, 6, 4), channel_mesh), ((8, 2, 4), channel_mesh)])
def test_within_a_colour_no_vertex_is_touched_twice(dims, mesh_of):
    axes = P.axes_of(mesh_of(dims))
    nx, ny, nz = dims
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny if axes[1].periodic else ny - 1), np.arange(nz), indexing="ij")
    cells = ((k * ny + j) * nx + i).ravel()  # every cell there is
    assert not R.touched_twice(axes, cells)
    if dims[1] > 2:  # ((8, 2, 4) has one row of cells between its walls)
        assert sorted(set(R.colour_of(axes, cells))) == list(range(8))


@pytest.mark.parametrize("dims", [(15, 12, 10), (16, 11, 10), (16, 12, 9)])
def test_an_odd_periodic_count_touches_a_vertex_twice(dims):
    """cells n - 1 and 0 of the odd direction have the same parity and share the vertex 0: why the case is refused"""
    mesh = box_mesh(dims)
    axes = P.axes_of(mesh)
    nx, ny, nz = dims
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    assert R.touched_twice(axes, ((k * ny + j) * nx + i).ravel())
    with pytest.raises(X3dError, match="even vertex count"):
        check_two_way(mesh, 1)


def test_mesh_and_communicator_refusals():
    check_two_way(box_mesh(), 1)
    check_two_way(channel_mesh((16, 17, 8)), 1)  # (an odd count in a non-periodic direction is served)
    with pytest.raises(X3dError, match="several ranks"):
        check_two_way(box_mesh(), 2)
    cut = Mesh((16, 12, 10), (1, 1, 2), (2 * np.pi, np.pi, 3.0), PER, PER, PER)
    with pytest.raises(X3dError, match="several ranks"):
        check_two_way(cut, 2)


def test_config_refusals_and_the_loading_helper():
    x0 = np.zeros((4, 3))
    cfg = ParticlesConfig(x0, tau_p=0.1, two_way=True, mass=2.5e-3)
    assert cfg.two_way and cfg.mass == 2.5e-3
    plain = ParticlesConfig(x0, tau_p=0.1)
    assert not plain.two_way and plain.mass is None
    for kw in (dict(tau_p=0.0, two_way=True, mass=1.0), dict(tau_p=0.1, two_way=True), dict(tau_p=0.1, two_way=True, mass=0.0),
               dict(tau_p=0.1, two_way=True, mass=-1.0), dict(tau_p=0.1, two_way=True, mass=float("nan")),
               dict(tau_p=0.1, two_way=True, mass=float("inf")), dict(tau_p=0.1, two_way=True, mass="1"),
               dict(tau_p=0.1, two_way=True, mass=(1.0, 2.0))):
        with pytest.raises(X3dError):
            ParticlesConfig(x0, **kw)
    mesh = box_mesh()
    want = 0.2 * (2 * np.pi) * np.pi * 3.0 / 1000
    assert abs(mass_for_loading(mesh, 1000, 0.2) - want) <= 1e-15 * want
    for n, phi in ((0, 0.1), (10, 0.0), (10, float("nan"))):
        with pytest.raises(X3dError):
            mass_for_loading(mesh, n, phi)


def test_records_are_summed_in_id_order_whatever_the_slot_order():
    mesh = box_mesh()
    axes = P.axes_of(mesh)
    st = random_state(mesh, 400, 8)
    st["x"][:150] = st["x"][0] + 1e-3 * np.random.default_rng(1).random((150, 3))  # one crowded cell
    cells, rec = R.records(axes, st, 0.3, 0.1)
    perm = np.random.default_rng(2).permutation(400)
    shuffled = {k: v[perm] for k, v in st.items()}
    cells2, rec2 = R.records(axes, shuffled, 0.3, 0.1, ids=perm)
    assert np.array_equal(cells, cells2) and rec.tobytes() == rec2.tobytes()
    assert np.max(np.bincount(np.searchsorted(cells, P.cell_keys(axes, st["x"])))) >= 150
