"""The write-time algebra of the budget profiles (x3d2_amd/budgets.py: derive, ddn, the state and the file) on the host;
no GPU.  The references are tests/budgets_ref.py's longdouble restatements."""
import numpy as np
import pytest

import budgets_ref
from x3d2_amd import budgets
from x3d2_amd.budgets import BudgetsConfig, MOMENT_NAMES, PAIR_NAMES, TERMS, ddn, derive
from x3d2_amd.common import X3dError

SHAPE = (6, 9, 35)  # [nz, ny, nx]
NU = 1.0 / 4200.0


def random_fields(seed=7):
    """thirteen default_rng fields; U offset by 1 and v scaled by 0.1, so that the raw moments cancel"""
    rng = np.random.default_rng(seed)
    f = [rng.standard_normal(SHAPE) for _ in range(13)]
    f[0] = f[0] + 1.0
    f[1] = 0.1 * f[1]
    return f[0], f[1], f[2], f[3], f[4:]


def raw_moments(d, p_scale=1.0, pressure=True):
    u, v, w, p, grads = random_fields()
    m = budgets_ref.moments41(u, v, w, p if pressure else None, grads, d, p_scale).astype(np.float64)
    return dict(zip(MOMENT_NAMES, m))


def coords_of(d):
    n = SHAPE[2 - d]
    return np.sort(np.random.default_rng(3).random(n)) if d == 1 else np.arange(n) * (2.0 / n)


def test_moment_names_are_41_distinct_and_start_with_the_statistics_names():
    from x3d2_amd.stats import MEAN_NAMES
    assert len(MOMENT_NAMES) == len(set(MOMENT_NAMES)) == budgets.NMOM == 41
    assert MOMENT_NAMES[:3] == MEAN_NAMES[:3] and MOMENT_NAMES[4:10] == MEAN_NAMES[3:]
    assert MOMENT_NAMES[3] == "pmean" and MOMENT_NAMES[10] == "ppmean" and MOMENT_NAMES[11:14] == ("pumean", "pvmean", "pwmean")
    assert tuple(budgets.PRESSURE_MOMENTS) == budgets_ref.PRESSURE_MOMENTS


@pytest.mark.parametrize("d", [1, 2])
def test_derive_on_raw_moments_agrees_with_the_central_moments(d):
    """differences of raw moments against moments of fluctuations: 1e-12 max|term| (measured at this shape: 9e-16)"""
    u, v, w, p, grads = random_fields()
    p_scale = 1.0 / 5e-3
    got = derive(raw_moments(d, p_scale), coords_of(d), NU, d == 2, 2.0, d)
    want = budgets_ref.central(u, v, w, p, grads, d, NU, p_scale)
    assert len(want) == 1 + 3 + 5 * 6
    for name, ref in want.items():
        scale = float(np.max(np.abs(ref)))
        err = float(np.max(np.abs(got[name] - ref)))
        print("budgets check:", name, err, 1e-12 * scale)
        assert got[name].shape == (SHAPE[2 - d],) and scale > 0.0
        assert err <= 1e-12 * scale, name


def test_ddn_is_exact_on_quadratic_profiles():
    from x3d2_amd.mesh import Mesh
    per, wall = ("periodic",) * 2, ("dirichlet",) * 2
    mesh = Mesh((8, 33, 8), (1, 1, 1), (4.0, 2.0, 2.0), per, wall, per, ("uniform", "top-bottom", "uniform"),
                (1.0, 0.259065151, 1.0))
    y = np.asarray(mesh.vert_coords[1], dtype=np.float64)[:33]
    assert y.shape == (33,) and np.ptp(np.diff(y)) > 1e-3  # (stretched)
    quad = lambda x: 0.7 * x * x - 1.3 * x + 0.25
    for x in (y, np.sort(np.random.default_rng(1).random(17))):
        f = quad(x)
        d1, d2 = ddn(f, x), ddn(ddn(f, x), x)
        assert np.max(np.abs(d1 - (1.4 * x - 1.3))) <= 1e-8 * np.max(np.abs(d1))
        assert np.max(np.abs(d2 - 1.4)) <= 1e-8 * 1.4
    # a periodic uniform line: exact on a quadratic away from the seam, zero on a constant, and the two seam points
    # take their neighbours from the other end
    n, L = 16, 2.0
    x = np.arange(n) * (L / n)
    f = quad(x)
    d1 = ddn(f, x, True, L)
    assert np.max(np.abs(d1[1:-1] - (1.4 * x[1:-1] - 1.3))) <= 1e-8 * np.max(np.abs(d1))
    d2 = ddn(d1, x, True, L)
    assert np.max(np.abs(d2[2:-2] - 1.4)) <= 1e-8 * 1.4
    assert not np.any(ddn(np.full(n, 3.5), x, True, L))
    g = np.random.default_rng(2).standard_normal(n)
    dg = ddn(g, x, True, L)
    h = L / n
    assert abs(dg[0] - (g[1] - g[-1]) / (2 * h)) <= 1e-14 * np.max(np.abs(dg))
    assert abs(dg[-1] - (g[0] - g[-2]) / (2 * h)) <= 1e-14 * np.max(np.abs(dg))
    assert abs(dg[5] - (g[6] - g[4]) / (2 * h)) <= 1e-14 * np.max(np.abs(dg))
    with pytest.raises(X3dError):
        ddn(g, x[:-1])
    with pytest.raises(X3dError):
        ddn(g, x, True)


@pytest.mark.parametrize("d", [1, 2])
def test_residual_is_the_signed_sum_and_k_is_the_half_trace(d):
    got = derive(raw_moments(d), coords_of(d), NU, d == 2, 2.0, d)
    for n in PAIR_NAMES + ("k",):
        t = {term: got["%s_%s" % (term, n)] for term in TERMS}
        want = (t["production"] + t["convection"] + t["turbulent_transport"] + t["pressure_diffusion"]
                + t["pressure_strain"] + t["viscous_diffusion"] - t["dissipation"])
        scale = max(float(np.max(np.abs(v))) for v in t.values())
        assert np.max(np.abs(t["residual"] - want)) <= 8 * np.finfo(np.float64).eps * scale, n
    for term in TERMS + ("R",):
        half = 0.5 * (got[term + "_uu"] + got[term + "_vv"] + got[term + "_ww"])
        assert np.array_equal(got[term + "_k"], half), term
    # pressure diffusion acts where a component is the kept one: uu and (y kept) ww see none
    assert not np.any(got["pressure_diffusion_uu"])
    other = "ww" if d == 1 else "vv"
    assert not np.any(got["pressure_diffusion_" + other]) and np.any(got["pressure_diffusion_" + ("vv" if d == 1 else "ww")])


def test_without_pressure_the_pressure_terms_are_absent():
    m = raw_moments(1, pressure=False)
    for k in budgets.PRESSURE_MOMENTS:
        assert not np.any(m[MOMENT_NAMES[k]])
    with_p = derive(raw_moments(1), coords_of(1), NU, False, 2.0, 1)
    got = derive(m, coords_of(1), NU, False, 2.0, 1, pressure=False)
    gone = sorted(set(with_p) - set(got))
    want = ["p_rms"] + ["q_" + c for c in "uvw"] + ["%s_%s" % (t, n) for t in ("pressure_diffusion", "pressure_strain")
                                                    for n in PAIR_NAMES + ("k",)]
    assert gone == sorted(want) and not set(got) - set(with_p)
    for n in PAIR_NAMES + ("k",):
        want = (got["production_" + n] + got["convection_" + n] + got["turbulent_transport_" + n]
                + got["viscous_diffusion_" + n] - got["dissipation_" + n])
        scale = max(float(np.max(np.abs(got["%s_%s" % (t, n)]))) for t in TERMS if t not in budgets.PRESSURE_TERMS)
        assert np.max(np.abs(got["residual_" + n] - want)) <= 8 * np.finfo(np.float64).eps * scale
    with pytest.raises(X3dError):
        derive(m, coords_of(1), NU, False, 2.0, 0)


def test_state_and_file_round_trips_keep_the_bits(tmp_path):
    m = raw_moments(1)
    state = budgets.state_from_moments(2, True, 5, m)
    assert sorted(state) == sorted(["budgets_sample_count", "budgets_profile_dir", "budgets_pressure"]
                                   + ["budgets_" + n for n in MOMENT_NAMES])
    np.savez(str(tmp_path / "state.npz"), **state)
    with np.load(str(tmp_path / "state.npz")) as z:
        count, raw = budgets.moments_from_state({k: z[k] for k in z.files}, 2, True, SHAPE[1])
    assert count == 5 and raw.dtype == np.float64 and raw.shape == (41, SHAPE[1])
    for k, n in enumerate(MOMENT_NAMES):
        assert raw[k].tobytes() == m[n].tobytes(), n
    with pytest.raises(X3dError, match="profile_dir"):
        budgets.moments_from_state(state, 3, True)
    with pytest.raises(X3dError, match="pressure"):
        budgets.moments_from_state(state, 2, False)
    with pytest.raises(X3dError, match="holds none"):
        budgets.moments_from_state({}, 2, True)
    with pytest.raises(X3dError, match="values"):
        budgets.moments_from_state(state, 2, True, SHAPE[1] + 1)
    terms = derive(m, coords_of(1), NU, False, 2.0, 1)
    prefix = str(tmp_path / "budgets")
    name = budgets.save_budgets(prefix, 12, 2, True, coords_of(1), 5, m, terms)
    assert name == prefix + "_000012.npz"
    back = budgets.load_budgets(prefix, 12)
    assert (back["sample_count"], back["iteration"], back["profile_dir"], back["pressure"]) == (5, 12, 2, True)
    assert np.array_equal(back["coord"], coords_of(1))
    assert sorted(back["moments"]) == sorted(MOMENT_NAMES) and sorted(back["budgets"]) == sorted(terms)
    for n in MOMENT_NAMES:
        assert back["moments"][n].tobytes() == m[n].tobytes()
    for n in terms:
        assert back["budgets"][n].tobytes() == terms[n].tobytes()


def test_config_validation():
    cfg = BudgetsConfig()
    assert not cfg.active and not cfg.sample_due(1) and not cfg.output_due(4)
    assert (cfg.profile_dir, cfg.pressure, cfg.prefix) == (2, True, "budgets")
    cfg = BudgetsConfig(initbud=3, ibudfreq=2, ibudout=4, profile_dir=3, pressure=False)
    assert cfg.active and [it for it in range(1, 10) if cfg.sample_due(it)] == [3, 5, 7, 9]
    assert [it for it in range(1, 10) if cfg.output_due(it)] == [4, 8]
    with pytest.raises(X3dError, match="not built"):
        BudgetsConfig(profile_dir=1)
    for bad in (dict(profile_dir=0), dict(profile_dir=None), dict(ibudfreq=0), dict(ibudout=-1)):
        with pytest.raises(X3dError):
            BudgetsConfig(**bad)
