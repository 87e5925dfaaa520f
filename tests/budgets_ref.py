"""numpy restatement of the budget moments (csrc/budget.hip, x3d2_amd/budgets.py) for the tests.

moments41   the 41 plane means of one sample in longdouble, in the order of include/x3d2_hip.h
terms41     the 41 sampled products themselves (float64 [nz, ny, nx]): what the tests' bounds take max|term| of
central     the budget ingredients that need no derivative along the kept direction, formed DIRECTLY from fluctuations about
            the plane means -- what derive() reaches as differences of raw moments

Arrays are [nz, ny, nx]; d is 0-based (1 = y, 2 = z); grads holds nine arrays in compute_vorticity's order
(dudx, dudy, dudz, dvdx, ...); p may be None (the pressure moments are then 0)."""
import numpy as np

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
PAIR_NAMES = ("uu", "vv", "ww", "uv", "uw", "vw")
PRESSURE_MOMENTS = (3, 10, 11, 12, 13, 35, 36, 37, 38, 39, 40)


def plane_axes(d):
    """the axes of a [z, y, x] array that a profile along direction d (0-based) is a mean over"""
    return tuple(a for a in range(3) if a != 2 - d)


def terms41(u, v, w, p, grads, d, p_scale=1.0, dtype=np.float64):
    vel = [np.asarray(f, dtype=dtype) for f in (u, v, w)]
    g = [[np.asarray(grads[3 * i + j], dtype=dtype) for j in range(3)] for i in range(3)]
    zero = np.zeros_like(vel[0])
    pp = zero if p is None else dtype(p_scale) * np.asarray(p, dtype=dtype)
    out = [vel[0], vel[1], vel[2], pp]
    out += [vel[i] * vel[j] for i, j in PAIRS]
    out += [pp * pp] + [pp * vel[i] for i in range(3)]
    out += [vel[i] * vel[j] * vel[d] for i, j in PAIRS]
    out += [g[i][j] for i in range(3) for j in range(3)]
    out += [g[i][0] * g[j][0] + g[i][1] * g[j][1] + g[i][2] * g[j][2] for i, j in PAIRS]
    out += [pp * (g[i][j] + g[j][i]) for i, j in PAIRS]
    assert len(out) == 41
    return out


def moments41(u, v, w, p, grads, d, p_scale=1.0):
    """[41, n_keep] longdouble: the plane means of the 41 moments"""
    ax = plane_axes(d)
    return np.stack([t.mean(axis=ax, dtype=np.longdouble) for t in terms41(u, v, w, p, grads, d, p_scale, np.longdouble)])


def central(u, v, w, p, grads, d, nu, p_scale=1.0):
    """R_<pair>, T_<pair>, q_<c>, p_rms, production_<pair>, dissipation_<pair>, pressure_strain_<pair> from the
    fluctuations about the plane means, in longdouble"""
    ax = plane_axes(d)
    ld = np.longdouble
    mean = lambda f: f.mean(axis=ax, dtype=ld, keepdims=True)
    prof = lambda f: f.mean(axis=ax, dtype=ld)
    vel = [np.asarray(f, dtype=ld) for f in (u, v, w)]
    g = [[np.asarray(grads[3 * i + j], dtype=ld) for j in range(3)] for i in range(3)]
    pp = ld(p_scale) * np.asarray(p, dtype=ld)
    U = [mean(f) for f in vel]
    G = [[mean(g[i][j]) for j in range(3)] for i in range(3)]
    P = mean(pp)
    uf = [f - m for f, m in zip(vel, U)]
    gf = [[g[i][j] - G[i][j] for j in range(3)] for i in range(3)]
    pf = pp - P
    pidx = lambda i, j: PAIRS.index((min(i, j), max(i, j)))
    R = [prof(uf[i] * uf[j]) for i, j in PAIRS]
    out = {"p_rms": np.sqrt(prof(pf * pf))}
    for i, c in enumerate("uvw"):
        out["q_" + c] = prof(pf * uf[i])
    for k, (i, j) in enumerate(PAIRS):
        n = PAIR_NAMES[k]
        out["R_" + n] = R[k]
        out["T_" + n] = prof(uf[i] * uf[j] * uf[d])
        out["production_" + n] = -(R[pidx(i, d)] * prof(g[j][d]) + R[pidx(j, d)] * prof(g[i][d]))
        out["dissipation_" + n] = 2 * ld(nu) * prof(gf[i][0] * gf[j][0] + gf[i][1] * gf[j][1] + gf[i][2] * gf[j][2])
        out["pressure_strain_" + n] = prof(pf * (gf[i][j] + gf[j][i]))
    return out


def running_means(samples):
    """the recurrence mean += (x - mean) / k over a list of [41, n] longdouble arrays"""
    ref = np.zeros_like(samples[0])
    for k, x in enumerate(samples, 1):
        ref += (x - ref) / np.longdouble(k)
    return ref
