"""numpy restatement of the particle rules of x3d2_amd/particles.py (csrc/particles.hip): the interpolation rule of one
direction, the tensor-product value, and ONE update of tracers or inertial particles.  Vectorised over the particles; nothing
here is shared with the code under test."""
import numpy as np


class Axis:
    """one direction: c the n global vertex coordinates, L the period, periodic the flag"""

    def __init__(self, c, L, periodic):
        self.c = np.asarray(c, dtype=np.float64)
        self.n, self.L, self.periodic = int(self.c.size), float(L), bool(periodic)
        self.lo, self.hi = float(self.c[0]), float(self.c[-1])


def axes_of(mesh):
    from x3d2_amd.diagnostics import global_vert_coords
    return [Axis(global_vert_coords(mesh, d), float(mesh.L[d]), bool(mesh.periodic_BC[d])) for d in range(3)]


def wrap(x, L):
    x = np.asarray(x, dtype=np.float64)
    y = x - L * np.floor(x / L)
    y = np.where(y >= L, 0.0, y)
    return np.where(y < 0.0, 0.0, y)  # (x one rounding below a multiple of L)


def cell(ax, x):
    """the largest i with c[i] <= x; periodic: the last cell n - 1 runs to L; otherwise clamped to n - 2"""
    i = np.searchsorted(ax.c, np.asarray(x, dtype=np.float64), side="right") - 1
    i = np.maximum(i, 0)
    return i if ax.periodic else np.minimum(i, ax.n - 2)


def nodes(ax, x, order, shift_stencil=True, wrap_coords=True):
    """(idx [m, order] the field indices, xi [m, order] the node coordinates); the two flags exist for the tests of this
    restatement only (what a dropped one-sided shift or a dropped coordinate wrap would give)"""
    i = cell(ax, x)
    s = i if order == 2 else i - 1
    if not ax.periodic and shift_stencil:
        s = np.clip(s, 0, ax.n - order)
    m = s[:, None] + np.arange(order)[None, :]
    idx = np.mod(m, ax.n) if ax.periodic else np.clip(m, 0, ax.n - 1)
    xi = ax.c[idx]
    if ax.periodic and wrap_coords:
        xi = xi + ax.L * np.floor_divide(m, ax.n)
    return idx, xi


def weights(xi, x, order):
    """w_a = prod_{b != a} (x - xi_b) / (xi_a - xi_b), b ascending"""
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(xi.shape)
    for a in range(order):
        for b in range(order):
            if b != a:
                w[:, a] *= (x - xi[:, b]) / (xi[:, a] - xi[:, b])
    return w


def stencil(ax, x, order):
    idx, xi = nodes(ax, x, order)
    return idx, weights(xi, x, order)


def interpolate(axes, fields, pts, order):
    """fields: [nz, ny, nx] arrays (any float type, widened to double); pts [m, 3] inside the domain (periodic coordinates
    are wrapped here) -> [m, len(fields)]"""
    pts = np.array(pts, dtype=np.float64)
    for d in range(3):
        if axes[d].periodic:
            pts[:, d] = wrap(pts[:, d], axes[d].L)
    (ix, wx), (iy, wy), (iz, wz) = (stencil(axes[d], pts[:, d], order) for d in range(3))
    out = np.zeros((pts.shape[0], len(fields)))
    for c, f in enumerate(fields):
        f = np.asarray(f, dtype=np.float64)
        vals = f[iz[:, :, None, None], iy[:, None, :, None], ix[:, None, None, :]]  # [m, k, j, i]
        sx = np.einsum("mkji,mi->mkj", vals, wx)
        sy = np.einsum("mkj,mj->mk", sx, wy)
        out[:, c] = np.einsum("mk,mk->m", sy, wz)
    return out


def ab2(first):
    return (1.0, 0.0) if first else (1.5, -0.5)


def boundaries(axes, x, v, wall):
    """x [n, 3] after the advance, v [n, 3] or None (tracers) -> (x, v, absorbed [n], reflected [n], clamped [n])"""
    x = x.copy()
    v = None if v is None else v.copy()
    n = x.shape[0]
    absorbed, reflected, clamped = (np.zeros(n, dtype=bool) for _ in range(3))
    for d, ax in enumerate(axes):
        if ax.periodic:
            x[:, d] = wrap(x[:, d], ax.L)
            continue
        below, above = x[:, d] < ax.lo, x[:, d] > ax.hi
        out = below | above
        if wall == "absorb":
            absorbed |= out
        else:
            x[:, d] = np.where(below, 2.0 * ax.lo - x[:, d], np.where(above, 2.0 * ax.hi - x[:, d], x[:, d]))
            if v is not None:
                v[:, d] = np.where(out, -v[:, d], v[:, d])
            reflected |= out
            clamped |= (x[:, d] < ax.lo) | (x[:, d] > ax.hi)
        x[:, d] = np.clip(x[:, d], ax.lo, ax.hi)
    return x, v, absorbed, reflected, clamped


def update(axes, fields, st, dt, order, first, tau=0.0, g=(0.0, 0.0, 0.0), wall="reflect"):
    """ONE update from the state `st` (dict of x, v, a, v_prev [n, 3], status [n]; inertial: F, F_prev too) with the fields
    u^it -> (the new state, info dict of reflected / clamped / absorbed masks).  A particle that is not alive keeps everything."""
    c1, c0 = ab2(first)
    inertial = tau > 0.0
    alive = st["status"] == 1
    x = st["x"] + dt * (c1 * st["v"] + c0 * st["v_prev"])
    vn = st["v"] + dt * (c1 * st["F"] + c0 * st["F_prev"]) if inertial else None
    x, vn, absorbed, reflected, clamped = boundaries(axes, x, vn, wall)
    a = interpolate(axes, fields, x, order)
    new = {k: np.array(val, copy=True) for k, val in st.items()}
    moved = alive & ~absorbed
    gone = alive & absorbed

    def put(key, val, mask):
        new[key][mask] = val[mask]

    put("x", x, alive)  # (an absorbed particle rests on the boundary it crossed)
    put("a", a, moved)
    put("v_prev", st["v"], moved)
    if inertial:
        put("v", vn, moved)
        put("F_prev", st["F"], moved)
        put("F", (a - vn) / tau + np.asarray(g, dtype=np.float64)[None, :], moved)
    else:
        put("v", a, moved)
    new["status"][gone] = 0
    return new, {"reflected": reflected & alive, "clamped": clamped & alive, "absorbed": gone}


def prime(axes, fields, x0, order, tau=0.0, g=(0.0, 0.0, 0.0), v0=None):
    x0 = np.array(x0, dtype=np.float64)
    for d in range(3):
        if axes[d].periodic:
            x0[:, d] = wrap(x0[:, d], axes[d].L)
    a = interpolate(axes, fields, x0, order)
    v = a.copy() if (tau == 0.0 or v0 is None) else np.array(v0, dtype=np.float64)
    st = {"x": x0, "v": v, "a": a, "v_prev": np.zeros_like(v), "status": np.ones(x0.shape[0], dtype=np.int32)}
    if tau > 0.0:
        st["F"] = (a - v) / tau + np.asarray(g, dtype=np.float64)[None, :]
        st["F_prev"] = np.zeros_like(v)  # (the history starts empty: the first advance weighs it with 0)
    return st


def cell_keys(axes, x):
    i, j, k = (cell(axes[d], x[:, d]) for d in range(3))
    return (k * axes[1].n + j) * axes[0].n + i
