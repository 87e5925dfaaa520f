"""Host checks of the band forcing: the numpy restatement tests/forcing_ref.py is right (its separable direct sums against
rfftn, Parseval's identity for the injected power, the zero mean, the solenoidal projection), the initial field of the isotropic
turbulence case follows its recipe, and every refusal of the configuration raises before anything else happens.  No GPU.

Bounds: 1e-13 relative for sums of a few thousand FP64 terms whose rounding stays near 1e-15 (a prototype gave 3e-15, 1e-16,
5e-18 and 2e-15 for the four properties of the restatement)."""
import types

import numpy as np
import pytest

import forcing_ref as R
import spectra_ref

TWOPI = 2.0 * np.pi
BOXES = [((20, 12, 18), (TWOPI, TWOPI, TWOPI)), ((33, 10, 9), (TWOPI, np.pi, 4.0))]


def velocity(dims, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((dims[2], dims[1], dims[0])) for _ in range(3)]


@pytest.mark.parametrize("dims,L", BOXES, ids=["20x12x18", "33x10x9"])
def test_direct_sums_equal_rfftn(dims, L):
    M = R.mode_box(L, 2.5)
    assert M == ((2, 2, 2) if dims[0] == 20 else (2, 1, 1))
    for a in velocity(dims):
        want = R.box_of(np.fft.rfftn(a, axes=R.AXES), dims, M)
        got = R.direct_sums(a, M)
        err = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
        print("direct sums against rfftn on %s: %.3e" % (dims, err))
        assert err <= 1e-13


@pytest.mark.parametrize("solenoidal", [True, False])
@pytest.mark.parametrize("dims,L", BOXES, ids=["20x12x18", "33x10x9"])
def test_power_mean_and_divergence(dims, L, solenoidal):
    vel = velocity(dims)
    P = 0.1
    r = R.forcing(vel, L, scheme="power", power=P, k_hi=2.5, solenoidal=solenoidal)
    assert r["band"].sum() > 0 and r["d"] > 0.0
    fu = float(np.mean(sum(f * u for f, u in zip(r["f"], vel))))
    print("<f.u> / P - 1 on %s solenoidal=%s: %.3e" % (dims, solenoidal, fu / P - 1.0))
    assert abs(fu - P) <= 1e-13 * P
    assert abs(r["power"] - P) <= 1e-13 * P
    fmax = max(float(np.max(np.abs(f))) for f in r["f"])
    for f in r["f"]:
        assert abs(float(np.mean(f))) <= 1e-13 * fmax
    if solenoidal:
        assert R.spectral_divergence(r["f"], L) <= 1e-13
    else:
        assert R.spectral_divergence(r["f"], L) > 1e-3  # (the unprojected band of white noise is not solenoidal)


def test_linear_scheme_and_guard():
    dims, L = BOXES[0]
    vel = velocity(dims)
    r = R.forcing(vel, L, scheme="linear", coeff=0.3, k_lo=0.5, k_hi=2.5)
    assert r["coeff"] == 0.3 and abs(r["power"] - 0.3 * r["d"]) <= 1e-15 * r["d"]
    for F, g in zip(r["F"], r["g"]):
        assert np.array_equal(F, 0.3 * g)
    z = R.forcing([np.zeros_like(a) for a in vel], L)
    assert z["coeff"] == 0.0 and z["power"] == 0.0 and all(not f.any() for f in z["f"])


def test_initial_field_follows_the_recipe():
    from x3d2_amd.case import hit_initial_field
    dims, L = (32, 32, 32), (TWOPI,) * 3
    f = R.initial_field(dims, L, k0=4.0, ke0=0.5, seed=0)
    ke = 0.5 * float(np.mean(f[0] ** 2 + f[1] ** 2 + f[2] ** 2))
    assert abs(ke - 0.5) <= 1e-14
    for a in f:
        assert abs(float(np.mean(a))) <= 1e-15
    assert R.spectral_divergence(f, L) <= 1e-13
    e = sum(spectra_ref.shell(a, L) for a in f)
    assert int(np.argmax(e)) == 4
    again = R.initial_field(dims, L, k0=4.0, ke0=0.5, seed=0)
    other = R.initial_field(dims, L, k0=4.0, ke0=0.5, seed=1)
    for a, b, c in zip(f, again, other):
        assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    # the library's generator is the same recipe (its own code: compared, not shared)
    lib = hit_initial_field(dims, L, k0=4.0, ke0=0.5, seed=0)
    for a, b in zip(f, lib):
        assert float(np.max(np.abs(a - b))) <= 1e-14
    # an anisotropic box with odd extents goes through the same steps
    g = R.initial_field((33, 10, 9), (TWOPI, np.pi, 4.0), k0=3.0, ke0=0.25, seed=5)
    assert abs(0.5 * float(np.mean(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)) - 0.25) <= 1e-14
    assert R.spectral_divergence(g, (TWOPI, np.pi, 4.0)) <= 1e-13


def test_band_tables_agree_with_the_restatement():
    from x3d2_amd.forcing import band_tables, twiddle_table
    for dims, L in BOXES:
        for k_lo, k_hi in ((0.0, 2.5), (1.2, 2.5), (0.0, 4.1)):
            M, band, kvec = band_tables(dims, L, k_lo, k_hi)
            assert M == R.mode_box(L, k_hi)
            want = R.box_of(R.band_mask(dims, L, k_lo, k_hi), dims, M)
            assert np.array_equal(band.reshape(want.shape).astype(bool), want)
            # no mode of the band lies outside the box
            assert int(band.sum()) == int(R.band_mask(dims, L, k_lo, k_hi).sum())
            kx, ky, kz = R.wave_numbers(dims, L)
            full = np.broadcast_arrays(kx, ky, kz)
            for c in range(3):
                assert np.array_equal(kvec[:, c].reshape(want.shape), R.box_of(full[c], dims, M))
    t = twiddle_table(33, 2)
    g = (np.arange(33)[:, None] * np.arange(3)[None, :]) % 33  # (the angle reduced in integers: no rounding before the cosine)
    assert np.max(np.abs(t[..., 0] - np.cos(TWOPI * g / 33))) <= 1e-15 and np.max(np.abs(t[..., 1] + np.sin(TWOPI * g / 33))) <= 1e-15


def fake_solver(dims=(32, 32, 32), L=(TWOPI,) * 3, periodic=(True,) * 3, stretched=(False,) * 3, nproc_dir=(1, 1, 1)):
    """a solver with a mesh and nothing else: a constructor that touches the backend before it refuses fails on it"""
    mesh = types.SimpleNamespace(periodic_BC=list(periodic), stretched=list(stretched), nproc_dir=np.array(nproc_dir),
                                 L=np.array(L, dtype=np.float64), get_global_dims=lambda loc: np.array(dims))
    return types.SimpleNamespace(mesh=mesh)


def test_config_refusals():
    from x3d2_amd.common import X3dError
    from x3d2_amd.forcing import Forcing, ForcingConfig
    nan, inf = float("nan"), float("inf")
    for kw in (dict(scheme="stochastic"), dict(power=nan), dict(coeff=inf), dict(k_lo=-1.0), dict(k_lo=3.0, k_hi=2.0),
               dict(k_hi=nan), dict(d_min=-1.0), dict(d_min=nan), dict(power="1")):
        with pytest.raises(X3dError):
            ForcingConfig(**kw)
    ok = ForcingConfig()
    assert ok.scheme == "power" and ok.solenoidal and ok.d_min == 1e-300 and ok.value == ok.power
    assert ForcingConfig(scheme="linear", coeff=0.3).value == 0.3
    cases = [(fake_solver(periodic=(True, False, True)), ok, "not periodic"),
             (fake_solver(stretched=(False, True, False)), ok, "not uniform"),
             (fake_solver(nproc_dir=(2, 1, 1)), ok, "never cut"),
             (fake_solver(dims=(64, 64, 64)), ForcingConfig(k_hi=9.0), "at most 8"),  # M = 9
             (fake_solver(dims=(8, 32, 32)), ForcingConfig(k_hi=4.0), "Nyquist"),     # M = 4 = n / 2
             (fake_solver(), ForcingConfig(k_lo=0.1, k_hi=0.9), "no mode"),           # M = 0: the box holds the mean alone
             (fake_solver(), ForcingConfig(k_lo=1.1, k_hi=1.3), "no mode")]           # an empty shell inside the box
    for solver, cfg, match in cases:
        with pytest.raises(X3dError, match=match):
            Forcing(solver, cfg)
    # M = 8 on 32 points: 2 M = 16 < 32 is served by the tables (the constructor then goes on to the backend)
    from x3d2_amd.forcing import band_tables
    M, band, _ = band_tables((32, 32, 32), (TWOPI,) * 3, 0.0, 8.5)
    assert M == (8, 8, 8) and band.sum() > 0
    with pytest.raises(X3dError):
        Forcing(fake_solver(), "power")
