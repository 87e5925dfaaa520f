"""Host side of the eddy diffusivity of the explicit LES (x3d2_amd/les.py with LesConfig(prt=...), x3d2_amd/scalars.py) and its
restatement (tests/les_scalar_ref.py): configuration, what is served, the two identities of the conservative form on a
periodic box, and a mutation check of the pointwise bound the GPU test uses.

Where a prt list of the wrong length is refused: LesConfig cannot know the solver, so check_served(solver, cfg) -- which
Les.__init__ calls before anything is allocated -- refuses it."""
import types

import numpy as np
import pytest

import les_ref
import les_scalar_ref
import util
from test_scalars_host import fake_solver

PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2


def test_prt_refusals_and_acceptance():
    from x3d2_amd.common import X3dError
    from x3d2_amd.les import LesConfig
    assert LesConfig().prt is None and LesConfig().prt_of(2) is None
    for bad in (0, 0.0, -0.85, float("nan"), float("inf"), "0.85", [0.85, -1.0], [0.85, "x"], [], {"a": 1}, True):
        with pytest.raises(X3dError):
            LesConfig(prt=bad)
    c = LesConfig(model="wale", prt=0.85)
    assert c.prt == 0.85 and c.prt_of(3) == [0.85] * 3 and c.model == "wale"
    assert LesConfig(prt=1).prt_of(1) == [1.0]
    l = LesConfig(prt=[0.85, 0.4])
    assert l.prt == [0.85, 0.4] and l.prt_of(2) == [0.85, 0.4]
    assert LesConfig(prt=(0.7,)).prt_of(1) == [0.7]


def test_check_served_with_and_without_prt():
    from x3d2_amd import Mesh
    from x3d2_amd.common import X3dError
    from x3d2_amd.les import LesConfig, check_served
    box = Mesh((16, 9, 8), (1, 1, 1), (1.0,) * 3, PER, WALL, PER)
    one, two, none = (types.SimpleNamespace(nspecies=n, mesh=box) for n in (1, 2, 0))
    with pytest.raises(X3dError, match="species"):
        check_served(one)
    with pytest.raises(X3dError, match="species"):
        check_served(one, LesConfig())
    check_served(one, LesConfig(prt=0.85))
    check_served(two, LesConfig(prt=0.85))
    check_served(two, LesConfig(prt=[0.85, 0.4]))
    check_served(none, LesConfig(prt=0.85))  # (nothing to serve: the number is not used)
    for solver, prt in ((one, [0.85, 0.4]), (two, [0.85]), (two, [0.85, 0.4, 0.7])):  # a list of the wrong length: here
        with pytest.raises(X3dError, match="entries"):
            check_served(solver, LesConfig(prt=prt))
    neu = Mesh((16, 9, 8), (1, 1, 1), (1.0,) * 3, PER, ("neumann",) * 2, PER)
    with pytest.raises(X3dError, match="Neumann"):
        check_served(types.SimpleNamespace(nspecies=1, mesh=neu), LesConfig(prt=0.85))


def test_scalars_accept_a_model_that_serves_species_and_no_other():
    from x3d2_amd.common import X3dError
    from x3d2_amd.scalars import Scalars, ScalarsConfig
    sc = Scalars(fake_solver(1, les=types.SimpleNamespace(serves_species=True)), ScalarsConfig())
    assert sc.ns == 1 and not sc.coupled
    for les in (object(), types.SimpleNamespace(serves_species=False)):
        with pytest.raises(X3dError, match="LES"):
            Scalars(fake_solver(1, les=les), ScalarsConfig())


# ---------------------------------------------------------------- the restatement on a periodic 40^3 box
DIMS = (40, 40, 40)
INV_PRT = 1.0 / 0.85


@pytest.fixture(scope="module")
def box():
    from x3d2_amd.common import BC_PERIODIC
    u, v, w = util.noisy_tgv(DIMS, (0, 0, 0), DIMS)
    deltas = [2 * np.pi / n for n in DIMS]
    ops = les_ref.dense_der1st(DIMS, deltas, [(BC_PERIODIC,) * 2] * 3)
    tables = [np.full(n, d ** (2.0 / 3.0)) for n, d in zip(DIMS, deltas)]
    _, nut, _ = les_ref.dense_term(u, v, w, ops, tables, "smagorinsky", 0.17 ** 2)
    phi = les_scalar_ref.noisy_phi(DIMS)
    sgs, g, k = les_scalar_ref.dense_scalar_term(phi, nut, ops, INV_PRT)
    return dict(phi=phi, nut=np.asarray(nut, dtype=np.float64), sgs=sgs, g=g, k=k)


def test_the_term_conserves_the_scalar_and_dissipates_its_variance(box):
    """the periodic der1st is antisymmetric with zero column sums: sum sgs_phi = 0 and sum phi sgs_phi = - sum kappa |grad phi|^2"""
    sgs, phi, g, k = box["sgs"], box["phi"], box["g"], box["k"]
    assert np.min(box["nut"]) >= 0.0 and np.max(box["nut"]) > 0.0
    assert abs(float(np.sum(sgs))) <= 1e-12 * float(np.sum(np.abs(sgs)))
    eps = float(np.sum(k * ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])))
    work = float(np.sum(phi * sgs))
    assert eps > 0.0 and abs(work + eps) <= 1e-12 * eps
    want = les_scalar_ref.row(box["nut"], g, INV_PRT)
    assert abs(eps - want) <= 1e-12 * want  # row() is the same sum, exactly rounded


@pytest.mark.parametrize("drop", [0, 1, 2])
def test_the_gpu_bound_sees_a_missing_gradient_component(box, drop):
    full = les_scalar_ref.flux(box["nut"], box["g"], INV_PRT)
    cut = les_scalar_ref.flux(box["nut"], box["g"], INV_PRT, drop=drop)
    bound = les_scalar_ref.flux_bound(box["nut"], box["g"], INV_PRT)
    moved = np.asarray(np.abs(full[drop] - cut[drop]), dtype=np.float64)
    ok = bound[drop] > 0.0
    assert np.mean(ok) > 0.99 and np.min(moved[ok] / bound[drop][ok]) > 1e6
    for j in range(3):
        if j != drop:
            assert not np.any(full[j] != cut[j])
