"""Host side of the explicit LES (x3d2_amd/les.py) and its restatement (tests/les_ref.py): configuration, width tables, the
energy identity of the conservative form on a periodic box, and a mutation check of the bound the GPU test uses."""
import types

import numpy as np
import pytest

import les_ref

PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2
MODELS = [("smagorinsky", 0.17 ** 2), ("wale", 0.5 ** 2)]


def test_config_defaults_and_validation():
    from x3d2_amd.common import X3dError
    from x3d2_amd.les import LesConfig
    c = LesConfig()
    assert (c.model, c.cs, c.cw) == ("smagorinsky", 0.17, 0.5) and c.c2 == 0.17 * 0.17
    w = LesConfig(model="WALE", cw=0.4)
    assert w.model == "wale" and w.constant == 0.4 and w.c2 == 0.4 * 0.4
    assert LesConfig(cs=0.0).c2 == 0.0
    with pytest.raises(X3dError, match="unknown model"):
        LesConfig(model="dynamic")
    for kw in (dict(cs=-0.1), dict(cw=-1.0), dict(cs=float("nan"))):
        with pytest.raises(X3dError, match="negative"):
            LesConfig(**kw)


def test_species_and_neumann_are_refused_before_anything_is_built():
    from x3d2_amd import Mesh
    from x3d2_amd.common import X3dError
    from x3d2_amd.les import check_served
    box = Mesh((16, 9, 8), (1, 1, 1), (1.0,) * 3, PER, WALL, PER)
    check_served(types.SimpleNamespace(nspecies=0, mesh=box))
    with pytest.raises(X3dError, match="species"):
        check_served(types.SimpleNamespace(nspecies=1, mesh=box))
    neu = Mesh((16, 9, 8), (1, 1, 1), (1.0,) * 3, PER, ("neumann",) * 2, PER)
    with pytest.raises(X3dError, match="Neumann"):
        check_served(types.SimpleNamespace(nspecies=0, mesh=neu))
    half = Mesh((16, 9, 8), (1, 1, 1), (1.0,) * 3, PER, PER, ("dirichlet", "neumann"))
    with pytest.raises(X3dError, match="Neumann"):
        check_served(types.SimpleNamespace(nspecies=0, mesh=half))


@pytest.mark.parametrize("nproc,rank", [((1, 1, 1), 0), ((1, 1, 2), 1), ((1, 2, 1), 1)])
def test_width_tables_are_the_two_thirds_power_of_the_spacings(nproc, rank):
    from x3d2_amd import Mesh
    from x3d2_amd.diagnostics import spacing_tables
    from x3d2_amd.les import width_tables
    mesh = Mesh((16, 34, 8), nproc, (4.0, 2.0, 2.0), PER, WALL, PER, ("uniform", "top-bottom", "uniform"),
                (1.0, 0.259065151, 1.0), nrank=rank)
    a, ih = width_tables(mesh), spacing_tables(mesh)
    for d in range(3):
        assert a[d].dtype == np.float64 and a[d].shape == (int(mesh.vert_dims[d]),) and a[d].flags["C_CONTIGUOUS"]
        want = np.cbrt((1.0 / np.asarray(ih[d], dtype=np.longdouble)) ** 2)
        assert np.max(np.abs(a[d] - want) / want) <= 4 * 2.0 ** -52
    assert np.ptp(a[1]) > 0.1 * a[1].max()  # the stretched y: the table varies
    d2 = les_ref.width_squared(a)
    h3 = 1.0 / (ih[0][None, None, :] * ih[1][None, :, None] * ih[2][:, None, None])
    assert np.max(np.abs(np.asarray(d2, dtype=np.float64) ** 1.5 / h3 - 1.0)) <= 1e-14


@pytest.mark.parametrize("model,c2", MODELS)
def test_energy_identity_and_momentum_conservation_on_a_periodic_box(model, c2):
    """the periodic der1st is antisymmetric with zero column sums, so sum u_i sgs_i = - sum 2 nu_t S:S and sum sgs_i = 0"""
    from x3d2_amd.common import BC_PERIODIC
    dims = (12, 10, 8)
    rng = np.random.default_rng(0)
    u, v, w = (rng.standard_normal((dims[2], dims[1], dims[0])) for _ in range(3))
    deltas = [1.0 / n for n in dims]
    ops = les_ref.dense_der1st(dims, deltas, [(BC_PERIODIC,) * 2] * 3)
    tables = [np.full(n, d ** (2.0 / 3.0)) for n, d in zip(dims, deltas)]
    sgs, nt, ss = les_ref.dense_term(u, v, w, ops, tables, model, c2)
    eps = float(np.sum(2.0 * nt * ss))
    work = float(np.sum(u * sgs[0] + v * sgs[1] + w * sgs[2]))
    assert eps > 0.0 and abs(work + eps) <= 1e-12 * eps
    scale = sum(float(np.sum(np.abs(f))) for f in sgs)
    assert all(abs(float(np.sum(f))) <= 1e-12 * scale for f in sgs)


@pytest.mark.parametrize("model,c2", MODELS)
def test_the_gpu_bound_sees_a_missing_gradient(model, c2):
    """dropping g_32 from the restatement moves nu_t by more than 100 x the pointwise bound of tests/test_hip_les.py at
    most points (all but those where g_32 happens to be small)"""
    dims = (35, 9, 6)
    rng = np.random.default_rng(3)
    grads = [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(9)]
    tables = [rng.uniform(0.5, 2.0, n) for n in dims]
    full = les_ref.nut(grads, tables, model, c2)
    cut = les_ref.nut(grads, tables, model, c2, drop=7)
    bound, _ = les_ref.bounds(grads, tables, model, c2)
    moved = np.asarray(np.abs(full - cut), dtype=np.float64)
    assert np.max(moved / bound) > 1e6 and np.mean(moved > 100.0 * bound) > 0.99


def test_restatement_special_points():
    """all-zero gradients: nu_t = 0 with no NaN; pure shear (only g_12): WALE's nu_t = 0 exactly, Smagorinsky's is not"""
    z = np.zeros((2, 3, 4))
    shear = [z.copy() for _ in range(9)]
    shear[1] = np.full(z.shape, 1.5)
    tables = [np.ones(4), np.ones(3), np.ones(2)]
    for model, c2 in MODELS:
        assert not np.any(les_ref.nut([z] * 9, tables, model, c2))
    assert not np.any(les_ref.nut(shear, tables, "wale", 0.25))
    assert np.all(les_ref.nut(shear, tables, "smagorinsky", 1.0) == 1.5)
