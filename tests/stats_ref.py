"""numpy restatement of the reference's statistics (src/io/stats.f90): the checker of tests/test_stats_host.py (which pins it
against the reference's own known-answer series) and of tests/test_hip_stats.py (which holds the kernels to it)."""
import numpy as np

MOMENTS = ("u", "v", "w", "uu", "vv", "ww", "uv", "uw", "vw")
MEAN_NAMES = tuple(m + "mean" for m in MOMENTS)


def sample_due(initstat, istatfreq, it):
    """src/io/stats.f90:129-131, with is_active of :83"""
    if initstat <= 0:
        return False
    if it < initstat:
        return False
    if (it - initstat) % istatfreq != 0:
        return False
    return True


def accumulate_mean(mean, val, stat_inc):
    """src/io/stats.f90:61-70"""
    return mean + (val - mean) * stat_inc


def moments(u, v, w):
    """the nine sampled values in the order of src/io/stats.f90:151-159"""
    return [u, v, w, u * u, v * v, w * w, u * v, u * w, v * w]


def running_means(samples, dtype=np.float64):
    """samples: iterable of (u, v, w); returns the nine running means after the last one, computed in `dtype`"""
    means, n = None, 0
    for u, v, w in samples:
        vals = moments(*(np.asarray(a, dtype=dtype) for a in (u, v, w)))
        if means is None:
            means = [np.zeros_like(x) for x in vals]
        n += 1
        inc = dtype(1.0) / dtype(n)
        means = [accumulate_mean(m, x, inc) for m, x in zip(means, vals)]
    return means


def derive(means):
    """src/io/stats.f90:232-237: uprime, vprime, wprime, <u'v'>, <u'w'>, <v'w'>"""
    u, v, w, uu, vv, ww, uv, uw, vw = means
    return [np.sqrt(np.maximum(0.0, uu - u ** 2)), np.sqrt(np.maximum(0.0, vv - v ** 2)),
            np.sqrt(np.maximum(0.0, ww - w ** 2)), uv - u * v, uw - u * w, vw - v * w]


# the four known-answer series of the reference's tests/unit/test_statistics.f90: name -> (n_samples, u_n, v_n)
SERIES = {
    "constant": (100, lambda n: 1.0, lambda n: 1.0),
    "one_to_n": (50, lambda n: float(n), lambda n: float(n)),
    "alternating": (200, lambda n: 1.0 if n % 2 == 0 else -1.0, lambda n: 1.0 if n % 2 == 0 else -1.0),
    "correlated": (100, lambda n: float(n), lambda n: float(n)),
    "anticorrelated": (100, lambda n: float(n), lambda n: -float(n)),
}


def check_series(name, means, fl):
    """the reference's assertions (tests/unit/test_statistics.f90) with its tolerances, on arrays or scalars:
    means = the nine running means, fl = derive(means)"""
    umean, uprime, uv = np.asarray(means[0]), np.asarray(fl[0]), np.asarray(fl[3])
    var = np.asarray(means[3]) - umean ** 2
    if name == "constant":  # :46-54
        assert np.all(np.abs(umean - 1.0) <= 1e-12) and np.all(np.abs(uprime) <= 1e-12)
    elif name == "one_to_n":  # :74
        assert np.all(np.abs(umean - 25.5) <= 1e-12)
    elif name == "alternating":  # :101-109
        assert np.all(np.abs(umean) <= 1e-10) and np.all(np.abs(uprime - 1.0) <= 1e-10)
    elif name == "correlated":  # :140
        assert np.all(np.abs(uv - var) <= 1e-10 * np.abs(var))
    elif name == "anticorrelated":  # :164
        assert np.all(np.abs(uv + var) <= 1e-10 * np.abs(var))
    else:
        raise KeyError(name)
