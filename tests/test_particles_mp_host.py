"""Host checks of particles on several ranks: the ownership rule (x3d2_amd.particles.owner_index, the rule csrc/particles.hip
states in pmp_owns) against its restatement in tests/particles_mp_ref.py, the restated compaction, and the assembly of the rank
files.  No GPU."""
import numpy as np
import pytest

import particles_mp_ref as mref
import particles_ref as ref
from x3d2_amd import Mesh
from x3d2_amd.common import X3dError
from x3d2_amd.particles import ParticlesConfig, file_name, load_particles, owner_index, seed_uniform, wrap

TWOPI = 6.283185307179586
LAYOUTS = [(1, 2, 1), (1, 1, 2), (1, 2, 2)]


def box_mesh(layout=(1, 1, 1), rank=0):
    return Mesh((32, 32, 32), layout, (TWOPI,) * 3, ("periodic",) * 2, ("periodic",) * 2, ("periodic",) * 2, nrank=rank)


def channel_mesh(layout=(1, 1, 1), rank=0):
    return Mesh((32, 33, 24), layout, (4.0, 2.0, 2.0), ("periodic",) * 2, ("dirichlet",) * 2, ("periodic",) * 2,
                ("uniform", "top-bottom", "uniform"), (1.0, 0.259065151, 1.0), nrank=rank)


def wall_mesh():
    """a non-periodic direction that CAN be cut: 32 vertices between two walls in z"""
    return Mesh((32, 32, 32), (1, 1, 1), (TWOPI,) * 3, ("periodic",) * 2, ("periodic",) * 2, ("dirichlet",) * 2)


def points_with_edges(axes, layout, rng, n=4000):
    """random in-domain points plus, per direction, every rank boundary vertex, its two neighbours in the doubles, 0, and the
    last double below L (periodic) or the last vertex itself (walls)"""
    pts = np.empty((n, 3))
    for d, ax in enumerate(axes):
        lo, hi = (0.0, ax.L) if ax.periodic else (ax.lo, ax.hi)
        pts[:, d] = lo + (hi - lo) * rng.random(n)
        if ax.periodic:
            pts[:, d] = np.where(pts[:, d] >= hi, 0.0, pts[:, d])
    extra = []
    for d in (1, 2):
        ax, P = axes[d], int(layout[d])
        nl = ax.n // P
        vals = [0.0 if ax.periodic else ax.lo, np.nextafter(ax.L, 0.0) if ax.periodic else ax.hi]
        for r in range(1, P):
            b = ax.c[r * nl]
            vals += [b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf)]
        for v in vals:
            row = pts[rng.integers(n)].copy()
            row[d] = v
            extra.append(row)
    return np.vstack([pts, np.array(extra)])


@pytest.mark.parametrize("mesh_of,layout", [(box_mesh, lay) for lay in LAYOUTS] + [(channel_mesh, (1, 1, 2))])
def test_every_in_domain_point_has_exactly_one_owner(mesh_of, layout):
    axes = ref.axes_of(mesh_of())
    pts = points_with_edges(axes, layout, np.random.default_rng(5))
    claims = np.zeros(pts.shape[0], dtype=np.int64)
    for rank in range(int(np.prod(layout))):
        m = mesh_of(layout, rank)
        mine = np.ones(pts.shape[0], dtype=bool)
        for d in (1, 2):  # the library's host rule with this rank's mesh
            if layout[d] > 1:
                mine &= owner_index(axes[d].c, layout[d], axes[d].periodic, axes[d].L, pts[:, d]) == int(m.nrank_dir[d])
        # ... written out once more on the mesh's own offsets
        want = np.ones(pts.shape[0], dtype=bool)
        for d in (1, 2):
            off, nl, c = int(m.n_offset[d]), int(m.vert_dims[d]), axes[d].c
            last = off + nl == axes[d].n
            upper = ((pts[:, d] < axes[d].L) if axes[d].periodic else (pts[:, d] <= c[-1])) if last else (pts[:, d] < c[min(off + nl, axes[d].n - 1)])
            want &= (pts[:, d] >= c[off]) & upper
        assert np.array_equal(mine, want)
        assert np.array_equal(mine, mref.owner(axes, layout, pts) == rank)
        claims += mine
    assert np.all(claims == 1)


def test_a_cut_wall_direction_gives_the_last_vertex_to_the_last_rank():
    axes = ref.axes_of(wall_mesh())
    z = axes[2]
    x = np.array([z.lo, z.c[16], np.nextafter(z.c[16], -np.inf), z.hi])
    assert list(owner_index(z.c, 2, False, z.L, x)) == [0, 1, 0, 1]
    own, count = mref.owner_1d(z, 2, x)
    assert list(own) == [0, 1, 0, 1] and np.all(count == 1)
    # a wall direction has no neighbour beyond its ends: nothing leaves through them
    assert list(mref.classify(z, 2, 0, x, np.ones(4))) == [0, 2, 0, 2]
    assert list(mref.classify(z, 2, 1, x, np.ones(4))) == [1, 0, 1, 0]


def test_the_host_wrap_is_the_restatement_and_idempotent():
    rng = np.random.default_rng(6)
    x = np.concatenate([rng.uniform(-20.0, 20.0, 1000), [0.0, -0.0, TWOPI, -TWOPI, np.nextafter(TWOPI, 0.0), -1e-300]])
    w = wrap(x, TWOPI)
    assert np.array_equal(w, ref.wrap(x, TWOPI)) and np.all((w >= 0.0) & (w < TWOPI))
    assert np.array_equal(wrap(w, TWOPI), w)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_restated_compaction_conserves_ids_and_puts_everyone_where_it_belongs(layout):
    axes = ref.axes_of(box_mesh())
    rng = np.random.default_rng(7)
    n = 3000
    x0 = seed_uniform(box_mesh(), n, seed=8)
    order = mref.initial_order(axes, layout, x0)
    assert np.array_equal(np.sort(np.concatenate(order)), np.arange(n))
    assert all(np.all(np.diff(o) > 0) for o in order)
    status = np.ones(n, dtype=np.int32)
    status[rng.integers(n, size=20)] = 0
    status[rng.integers(n, size=5)] = 2
    x = x0.copy()
    for _ in range(4):
        moved = ref.wrap(x + rng.normal(scale=0.8, size=x.shape), TWOPI)  # less than a slab: face neighbours only
        x = np.where((status == 2)[:, None], x, moved)
        before = [o.copy() for o in order]
        order = mref.migrate(axes, layout, order, x, status)
        assert np.array_equal(np.sort(np.concatenate(order)), np.arange(n))
        own = mref.owner(axes, layout, x)
        for rank, ids in enumerate(order):
            live = status[ids] != 2
            assert np.all(own[ids][live] == rank)
            stayers = [i for i in before[rank] if i in set(ids.tolist())]
            assert list(ids[:len(stayers)]) == stayers  # the stayers come first, in their previous order
        for rank, ids in enumerate(before):  # a particle whose position is not finite any more never leaves
            dead = set(ids[status[ids] == 2].tolist())
            assert dead <= set(order[rank].tolist())


def test_rank_files_assemble_in_id_order(tmp_path):
    rng = np.random.default_rng(9)
    n = 100
    full = {"id": np.arange(n, dtype=np.int64), "x": rng.normal(size=(n, 3)), "v": rng.normal(size=(n, 3)),
            "a": rng.normal(size=(n, 3)), "alive": rng.integers(2, size=n).astype(np.int32)}
    full["status"] = full["alive"].copy()
    full["x"][3, 1] = -0.0
    holder = rng.integers(3, size=n)
    prefix = str(tmp_path / "p")
    for r in range(3):
        ids = np.nonzero(holder == r)[0]
        np.savez(file_name(prefix, 4, r), iteration=np.int64(4), time=np.float64(0.5), **{k: v[ids] for k, v in full.items()})
    assert file_name(prefix, 4, 1).endswith("p_000004.r1.npz")
    got = load_particles(prefix, 4)
    for k, v in full.items():
        assert got[k].tobytes() == v.tobytes(), k
    assert int(got["iteration"]) == 4 and float(got["time"]) == 0.5
    assert mref.assemble([{k: v[holder == r] for k, v in full.items()} for r in range(3)])["x"].tobytes() == full["x"].tobytes()
    np.savez(file_name(prefix, 5, 0), iteration=np.int64(5), time=np.float64(0.5), **{k: v[:60] for k, v in full.items()})
    np.savez(file_name(prefix, 5, 1), iteration=np.int64(5), time=np.float64(0.5), **{k: v[50:] for k, v in full.items()})
    with pytest.raises(X3dError, match="each once"):
        load_particles(prefix, 5)


def test_capacities_default_and_given():
    cfg = ParticlesConfig(np.zeros((3000, 3)))
    assert cfg.capacities(2) == (2250 + 1024, 1024) and cfg.capacities(4) == (1125 + 1024, 1024)
    assert ParticlesConfig(np.zeros((100000, 3))).capacities(2) == (76024, 9503)
    assert ParticlesConfig(np.zeros((10, 3)), capacity=64, mig_capacity=1).capacities(2) == (64, 1)
    assert ParticlesConfig(np.zeros((10, 3)), capacity=8, mig_capacity=100).capacities(2) == (8, 100)
    for kw in (dict(capacity=0), dict(mig_capacity=0)):
        with pytest.raises(X3dError):
            ParticlesConfig(np.zeros((10, 3)), **kw)
