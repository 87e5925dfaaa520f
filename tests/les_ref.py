"""Restatements of the explicit LES (x3d2_amd/les.py, csrc/les.hip) for the tests: eddy viscosity, stress and the four scalars
in numpy.longdouble from nine gradient arrays [nz, ny, nx] and the three width tables, and the whole subgrid term from u, v,
w with the dense operators of tests/util.py (uniform grids only, as util.dense_operator states)."""
import numpy as np

LD = np.longdouble
# the gradient that holds tau_ij after the kernel (compute_vorticity's order); nu_t is in 3; 6 and 7 keep their gradients
TAU_BLOCK = ((0, 1, 2), (1, 4, 5), (2, 5, 8))
NUT_BLOCK = 3


def width_squared(tables, dtype=LD):
    """D2[k, j, i] = a_x[i] a_y[j] a_z[k]"""
    ax, ay, az = (np.asarray(t, dtype=dtype) for t in tables)
    return ax[None, None, :] * ay[None, :, None] * az[:, None, None]


def strain(grads, dtype=LD):
    """S[i][j] and S:S"""
    g = [[np.asarray(grads[3 * i + j], dtype=dtype) for j in range(3)] for i in range(3)]
    S = [[(g[i][j] + g[j][i]) / dtype(2) for j in range(3)] for i in range(3)]
    ss = sum(S[i][j] * S[i][j] for i in range(3) for j in range(3))
    return g, S, ss


def frobenius(grads, dtype=LD):
    return np.sqrt(sum(np.asarray(a, dtype=dtype) ** 2 for a in grads))


def nut(grads, tables, model, c2, dtype=LD, drop=None):
    """the eddy viscosity; drop = an index 0..8 of a gradient that is left out (the mutation check)"""
    grads = [np.zeros_like(np.asarray(a, dtype=dtype)) if m == drop else a for m, a in enumerate(grads)]
    g, S, ss = strain(grads, dtype)
    cd = dtype(c2) * width_squared(tables, dtype)
    if model == "smagorinsky":
        return cd * np.sqrt(dtype(2) * ss)
    if model != "wale":
        raise ValueError(model)
    G = [[sum(g[i][k] * g[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    tr = (G[0][0] + G[1][1] + G[2][2]) / dtype(3)
    Sd = [[(G[i][j] + G[j][i]) / dtype(2) - (tr if i == j else 0) for j in range(3)] for i in range(3)]
    dd = sum(Sd[i][j] * Sd[i][j] for i in range(3) for j in range(3))
    den = ss ** 2 * np.sqrt(ss) + dd * np.sqrt(np.sqrt(dd))
    out = np.zeros_like(den)
    ok = den > 0
    out[ok] = (cd * dd * np.sqrt(dd))[ok] / den[ok]
    return out


def stress(grads, tables, model, c2, dtype=LD):
    """(nu_t, tau[i][j], S:S)"""
    _, S, ss = strain(grads, dtype)
    nt = nut(grads, tables, model, c2, dtype)
    return nt, [[dtype(2) * nt * S[i][j] for j in range(3)] for i in range(3)], ss


def scalars(grads, tables, ih, model, c2, dtype=LD):
    """the row of x3d_les_stress: sum nu_t, sum 2 nu_t S:S, max nu_t, max nu_t (ih_x^2 + ih_y^2 + ih_z^2)"""
    nt, _, ss = stress(grads, tables, model, c2, dtype)
    hx, hy, hz = (np.asarray(t, dtype=dtype) for t in ih)
    q = hx[None, None, :] ** 2 + hy[None, :, None] ** 2 + hz[:, None, None] ** 2
    return np.array([nt.sum(), (dtype(2) * nt * ss).sum(), nt.max(), (nt * q).max()], dtype=dtype)


# ---------------------------------------------------------------- the whole term, dense operators
def dense_der1st(dims, deltas, bcs):
    """[(A, B)] of der1st for x, y, z; bcs = three (start, end) pairs of BC codes"""
    import util
    return [util.dense_operator(int(n), float(d), "first-deriv", "compact6", int(bc[0]), int(bc[1]))
            for n, d, bc in zip(dims, deltas, bcs)]


def dense_term(u, v, w, ops, tables, model, c2):
    """(sgs[3], nu_t, S:S) in float64 from vertex fields [nz, ny, nx]: gradients, model, divergence of the stress, all with
    the dense der1st operators ops = [x, y, z]; array axis of direction d is 2 - d"""
    import util
    der = lambda f, d: util.dense_apply(ops[d], f, 2 - d)
    grads = [der(f, d) for f in (u, v, w) for d in range(3)]
    nt, tau, ss = stress(grads, tables, model, c2, dtype=np.float64)
    sgs = [sum(der(tau[i][j], j) for j in range(3)) for i in range(3)]
    return sgs, nt, ss


# ---------------------------------------------------------------- the pointwise bound of the GPU tests
# |nu_t - ref| <= K 2^-52 c2 D2 |g|_F and |tau_ij - ref| <= K 2^-52 c2 D2 |g|_F^2; K counted in tests/test_hip_les.py's docstring
K_BOUND = {"smagorinsky": 18.0, "wale": 288.0}


def bounds(grads, tables, model, c2):
    """(bound of nu_t, bound of tau_ij) per point, float64"""
    n = frobenius(grads)
    b = LD(K_BOUND[model]) * LD(2.0) ** -52 * LD(c2) * width_squared(tables) * n
    return np.asarray(b, dtype=np.float64), np.asarray(b * n, dtype=np.float64)
