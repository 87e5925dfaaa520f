"""Statistics, host side (no GPU): the sampling schedule, the ABI names, and the numpy checker of the GPU tests
(tests/stats_ref.py) against the reference's own known-answer series (tests/unit/test_statistics.f90)."""
import os
import re

import numpy as np
import pytest

import stats_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("x3d_stats_update_uvw", "x3d_stats_update_scalar", "x3d_stats_derive", "x3d_stats_profile_sums",
                "x3d_stats_profile_accumulate")


@pytest.mark.parametrize("initstat", [0, 1, 5])
@pytest.mark.parametrize("istatfreq", [1, 3])
def test_sample_schedule_restates_the_reference(initstat, istatfreq):
    """StatsConfig.sample_due == src/io/stats.f90:129-131 for it = 0..20; inactive when initstat <= 0 (:83)"""
    from x3d2_amd.stats import StatsConfig
    cfg = StatsConfig(initstat=initstat, istatfreq=istatfreq)
    assert cfg.active == (initstat > 0)
    for it in range(21):
        want = True
        if not initstat > 0:           # .not. self%is_active
            want = False
        elif it < initstat:            # iter < initstat
            want = False
        elif (it - initstat) % istatfreq != 0:
            want = False
        assert cfg.sample_due(it) == want, (initstat, istatfreq, it)
        assert stats_ref.sample_due(initstat, istatfreq, it) == want


def test_output_schedule_and_config_checks():
    from x3d2_amd.common import X3dError
    from x3d2_amd.stats import StatsConfig
    cfg = StatsConfig(initstat=1, istatout=4)
    assert [it for it in range(1, 13) if cfg.output_due(it)] == [4, 8, 12]
    assert not StatsConfig(initstat=1, istatout=0).output_due(4)  # src/io/stats.f90:212
    assert not StatsConfig(initstat=0, istatout=4).output_due(4)  # :211
    with pytest.raises(X3dError):
        StatsConfig(initstat=1, profile_dir=4)


def test_header_and_fortran_module_name_the_five_entry_points():
    header = open(os.path.join(ROOT, "include", "x3d2_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    capi = open(os.path.join(ROOT, "fortran", "m_x3d2_hip_capi.f90")).read()
    from x3d2_amd import _lib
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert re.search(r"bind\s*\(\s*C\s*,\s*name\s*=\s*['\"]%s['\"]\s*\)" % name, capi, flags=re.I), name
        assert name in _lib.PROTOTYPES


@pytest.mark.parametrize("name", sorted(stats_ref.SERIES))
def test_checker_reproduces_the_reference_known_answers(name):
    """the numpy restatement of accumulate_mean and of the write-time formulas passes the reference's four tests
    (constant field; 1..N; alternating -1 / +1; u = v and u = -v) at that file's tolerances: 1e-12, 1e-12, 1e-10 and
    1e-10 relative"""
    n, fu, fv = stats_ref.SERIES[name]
    means = stats_ref.running_means((np.array([fu(k)]), np.array([fv(k)]), np.array([0.0])) for k in range(1, n + 1))
    stats_ref.check_series(name, means, stats_ref.derive(means))


def test_checker_rounding_stays_inside_the_derived_recurrence_bound():
    """the GPU tests allow (n + 4) eps max|val|, twice the bound derived for the recurrence itself,
    ((n + 1) / 2 + 2) eps max|val|.  The checker's own rounding -- float64 against longdouble, float32 against float64,
    n up to 200 -- must stay inside the derived bound; the measured ratios err / (eps max|val|) are printed (0.0-0.46 on
    these samples: one rounded product alone is up to 0.5), so the GPU bound is loose for rounding while a defect, at
    1 / n of a sample, is orders of magnitude outside it"""
    rng = np.random.default_rng(7)
    samples = [tuple(rng.standard_normal(512) for _ in range(3)) for _ in range(200)]
    for lo, hi in ((np.float64, np.longdouble), (np.float32, np.float64)):
        if np.finfo(hi).eps >= np.finfo(lo).eps:
            continue  # (a platform whose longdouble is float64: the float32 pair still runs)
        eps = float(np.finfo(lo).eps)
        # (the wider run samples the values as the narrower kind holds them)
        cast = [tuple(a.astype(lo) for a in s) for s in samples]
        for n in (1, 7, 40, 200):
            got = stats_ref.running_means(cast[:n], dtype=lo)
            want = stats_ref.running_means(cast[:n], dtype=hi)
            for k, (g, w) in enumerate(zip(got, want)):
                vmax = max(float(np.max(np.abs(stats_ref.moments(*s)[k]))) for s in cast[:n])
                ratio = float(np.max(np.abs(g.astype(hi) - w))) / (eps * vmax)
                print("checker rounding:", lo.__name__, n, stats_ref.MOMENTS[k], "%.3f" % ratio)
                assert ratio <= (n + 1) / 2 + 2, (lo, n, k, ratio)


def test_stats_objects_need_no_device_until_used():
    """importing the module and building a config touches no GPU"""
    import x3d2_amd.stats as st
    assert st.MEAN_NAMES == stats_ref.MEAN_NAMES
    assert st.FLUCT_NAMES == ("uprime", "vprime", "wprime", "uvmean", "uwmean", "vwmean")
    m = {n: np.full(3, v) for n, v in zip(st.MEAN_NAMES, (1.0, 2.0, 3.0, 5.0, 4.0, 9.5, 2.5, 3.0, 6.5))}
    got = st.derive_host(m)
    want = stats_ref.derive([m[n] for n in st.MEAN_NAMES])
    for n, w in zip(st.FLUCT_NAMES, want):
        assert np.array_equal(got[n], w)
