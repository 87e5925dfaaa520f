"""Active scalars, host side (x3d2_amd/scalars.py): what is refused before anything is allocated, `coupled`, the Nusselt
formulas, and the physics of the restatement the GPU tests are held against (tests/scalars_ref.py).  No GPU."""
import types

import numpy as np
import pytest

from tests import scalars_ref as R
from x3d2_amd import Mesh
from x3d2_amd.common import NULL_LOC, VERT, X3dError
from x3d2_amd.scalars import Scalars, ScalarsConfig, nusselt


class _Field:
    def __init__(self, loc=VERT):
        self.data_loc = loc


def fake_solver(ns=2, periodic_y=False, les=None, loc=VERT):
    """what Scalars looks at before it allocates: no backend behind it, so a refusal that came late would fail loudly"""
    by = ("periodic",) * 2 if periodic_y else ("dirichlet",) * 2
    mesh = Mesh((8, 9 if not periodic_y else 8, 8), (1, 1, 1), (1.0, 1.0, 1.0), ("periodic",) * 2, by, ("periodic",) * 2)
    return types.SimpleNamespace(nspecies=ns, mesh=mesh, les=les, backend=None, u=_Field(loc), v=_Field(), w=_Field(),
                                 species=[_Field() for _ in range(ns)], nu_species=[0.1] * ns)


@pytest.mark.parametrize("kw", [dict(ri=[1.0]), dict(ref=[0.0, 0.0, 0.0]), dict(grad=[(0, 0, 1)]), dict(wall=[None]),
                                dict(init=[None, None, None])])
def test_a_list_of_the_wrong_length_is_refused(kw):
    with pytest.raises(X3dError):
        Scalars(fake_solver(2), ScalarsConfig(**kw))


@pytest.mark.parametrize("kw", [dict(ri=[1.0, float("nan")]), dict(ref=[float("inf"), 0.0]), dict(up=(0, float("nan"), 0)),
                                dict(grad=[(0, 0, float("inf")), None]), dict(wall=[{"y": (1.0, float("nan"))}, None]),
                                dict(up=(0, 1)), dict(wall=[{"q": (1.0, 0.0)}, None])])
def test_a_value_that_is_not_finite_is_refused(kw):
    with pytest.raises(X3dError):
        ScalarsConfig(**kw)


@pytest.mark.parametrize("pd", [1, 0, 4, "y"])
def test_profile_dir_other_than_2_or_3_is_refused(pd):
    with pytest.raises(X3dError):
        ScalarsConfig(profile_dir=pd)


def test_no_species_les_periodic_wall_and_data_loc_are_refused():
    with pytest.raises(X3dError):
        Scalars(fake_solver(0), ScalarsConfig())
    with pytest.raises(X3dError):
        Scalars(fake_solver(1, les=object()), ScalarsConfig())
    with pytest.raises(X3dError):  # x is periodic
        Scalars(fake_solver(1), ScalarsConfig(wall=[{"x": (1.0, 0.0)}]))
    with pytest.raises(X3dError):  # y is periodic on this mesh
        Scalars(fake_solver(1, periodic_y=True), ScalarsConfig(wall=[{"y": (None, 0.0)}]))
    with pytest.raises(X3dError):
        Scalars(fake_solver(1, loc=NULL_LOC), ScalarsConfig())
    with pytest.raises(X3dError):  # an init array of another shape: refused before the first upload
        Scalars(fake_solver(1), ScalarsConfig(init=[np.zeros((3, 3, 3))]))


def test_coupled():
    mk = lambda **kw: Scalars(fake_solver(2), ScalarsConfig(**kw))
    assert not mk().coupled
    assert not mk(ri=[0.0, 0.0], wall=[{"y": (1.0, 0.0)}, None]).coupled
    assert mk(ri=[0.0, 2.0]).coupled
    assert not mk(ri=[1.0, 1.0], up=(0, 0, 0)).coupled
    assert mk(ri=[0.0, 0.0], grad=[None, (0.0, 0.0, 1e-300)]).coupled
    assert not mk(grad=[(0, 0, 0), (0, 0, 0)]).coupled
    # masks: bit 2 d + side
    s = mk(wall=[{"y": (1.0, None)}, {1: (None, 0.5)}])
    assert s.mask == [4, 8] and s.value[0][2] == 1.0 and s.value[1][3] == 0.5 and s.own_mask == 63


def _coords(kind):
    if kind == "uniform":
        return np.linspace(0.0, 2.0, 33)
    m = Mesh((8, 33, 8), (1, 1, 1), (1.0, 2.0, 1.0), ("periodic",) * 2, ("dirichlet",) * 2, ("periodic",) * 2,
             ("uniform", "top-bottom", "uniform"), (1.0, 0.259065151, 1.0))
    return np.asarray(m.vert_coords[1])


@pytest.mark.parametrize("kind", ["uniform", "stretched"])
@pytest.mark.parametrize("fn", [nusselt, R.nusselt], ids=["library", "restatement"])
def test_nusselt_numbers_of_the_conduction_state_are_one(kind, fn):
    c = _coords(kind)
    H = c[-1] - c[0]
    got = fn(c, 1.0 - (c - c[0]) / H, np.zeros_like(c), 0.037, 1.0)
    assert np.max(np.abs(np.array(got) - 1.0)) < 1e-13, got
    # ... and scale with the wall values: 3 at y = 0, 1 at y = H is the same state with dphi = 2
    got = fn(c, 3.0 - 2.0 * (c - c[0]) / H, np.zeros_like(c), 0.037, 2.0)
    assert np.max(np.abs(np.array(got) - 1.0)) < 1e-13, got


def test_nusselt_library_and_restatement_agree_on_a_convecting_profile():
    c = _coords("stretched")
    eta = (c - c[0]) / (c[-1] - c[0])
    p = 1.0 - eta + 0.2 * np.sin(2 * np.pi * eta)
    q = 0.01 * np.sin(np.pi * eta) ** 2
    a, b = np.array(nusselt(c, p, q, 0.002, 1.0)), np.array(R.nusselt(c, p, q, 0.002, 1.0))
    assert np.max(np.abs(a - b)) < 1e-12 * np.max(np.abs(b)), (a, b)
    assert b[0] < 0.0 and b[2] > 1.0


def _roll_factor(Ra, dt, nsteps):
    dims, L = (32, 17, 16), (2.0, 1.0, 1.0)
    x = np.arange(dims[0]) * (L[0] / dims[0])
    y = np.linspace(0.0, 1.0, dims[1])
    v0 = 1e-6 * np.sin(np.pi * y)[None, :, None] * np.cos(2 * np.pi * x / L[0])[None, None, :] * np.ones(dims[::-1])
    r = R.RayleighBenardRef(dims, L, Ra=Ra, Pr=1.0, dt=dt, noise=0.0, vel0=(0.0 * v0, v0, 0.0 * v0))
    ke = []
    for _ in range(nsteps):
        r.step()
        ke.append(r.kinetic_energy())
    return ke[-1] / ke[nsteps // 2 - 1]


def test_restatement_straddles_the_rigid_rigid_threshold():
    """Rayleigh-Benard between rigid walls sets in at Ra = 1708 (wavelength 2.016 H).  A roll v ~ sin(pi y) cos(2 pi x / L_x)
    of amplitude 1e-6 on the conduction state, L_x = 2 H, Pr = 1: over the second half of the run the kinetic energy of the
    composed restatement falls by more than a factor 4 at Ra = 1000 and grows by more than a factor 4 at Ra = 5000.

    Grid 32 x 17 x 16 on L = (2, 1, 1), not 32 x 17 x 4 on (2, 1, 0.25): the same spacing and -- the roll does not depend on
    z -- the same physics, but four planes are fewer than the reference's periodic operators can serve (their distributed
    tridiagonal solve truncates a tail that decays like rho^n: the oracle's pressure correction of v = 0.01 (1 - y), which
    should leave nothing, leaves max |v| = 5.7e-2 at nz = 4, 3.9e-6 at nz = 8 and 5.2e-10 at nz = 16).
    dt is bound by the explicit diffusion at Ra = 1000 (kappa = Ra^-1/2).  Measured on the CPU: Ra = 1000, dt = 0.0125,
    640 steps: factor 0.214 (about 14 s); Ra = 5000, dt = 0.025, 320 steps: factor 8.46 (about 7 s)."""
    decay = _roll_factor(1000.0, 0.0125, 640)
    growth = _roll_factor(5000.0, 0.025, 320)
    print("kinetic energy, second half over first: Ra = 1000: %.4f   Ra = 5000: %.4f" % (decay, growth))
    assert decay < 0.25, decay
    assert growth > 4.0, growth
