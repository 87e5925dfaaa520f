"""numpy restatement of the two-way coupling of x3d2_amd/particles.py (csrc/particles.hip): the drag reaction of inertial
particles spread onto the vertices.  Built on tests/particles_ref.py (Axis, cell, wrap, update); nothing is taken from the
library.

    D_p      mass (a_p - v_p) / tau_p, per component, of every particle with status 1 (no gravity)
    cell     (i, j, k) of particles_ref.cell; the last periodic cell runs to L with node i + 1 -> 0
    weights  per direction w_1 = (x - c[i]) / (c[i + 1] - c[i]) (the periodic image of c[0] at L), w_0 = 1 - w_1
    record   of an occupied cell: R[corner = a + 2 b + 4 g][component] = the sum of wx_a wy_b wz_g D_p over the cell's
             particles in ascending id
    vertex   f[vertex] += -R / (dx_i dy_j dz_k), the cells taken colour by colour ((i mod 2) + 2 (j mod 2) + 4 (k mod 2),
             ascending), within a colour in ascending cell index
    dual     periodic direction d = L / n; otherwise d_0 = (c_1 - c_0) / 2, d_{n-1} = (c_{n-1} - c_{n-2}) / 2 and
             d_i = (c_{i+1} - c_{i-1}) / 2 between them

Arrays are [nz, ny, nx], as the library's get_field_data returns them.  FeedbackHit is the isotropic-turbulence case of
tests/forcing_ref.py (the oracle's transeq, stage and pressure correction) with the particles of tests/particles_ref.py and the
term added to the derivatives of every sub-step."""
import numpy as np

import particles_ref as P


def dual_widths(ax):
    """d_i of one direction"""
    if ax.periodic:
        return np.full(ax.n, ax.L / ax.n)
    c = ax.c
    d = np.empty(ax.n)
    d[0] = 0.5 * (c[1] - c[0])
    d[-1] = 0.5 * (c[-1] - c[-2])
    d[1:-1] = 0.5 * (c[2:] - c[:-2])
    return d


def linear_weights(ax, x):
    """(i [m], w [m, 2]) of one direction: the cell and the two trilinear weights"""
    x = np.asarray(x, dtype=np.float64)
    i = P.cell(ax, x)
    lo = ax.c[i]
    hi = np.where(i + 1 < ax.n, ax.c[np.minimum(i + 1, ax.n - 1)], ax.L)  # (i + 1 == n only in a periodic direction)
    w1 = (x - lo) / (hi - lo)
    return i, np.stack([1.0 - w1, w1], axis=1)


def corner_weights(axes, x):
    """(i, j, k [m], w [m, 8]) with corner a + 2 b + 4 g"""
    (i, wx), (j, wy), (k, wz) = (linear_weights(axes[d], x[:, d]) for d in range(3))
    w = np.empty((x.shape[0], 8))
    for g in range(2):
        for b in range(2):
            for a in range(2):
                w[:, a + 2 * b + 4 * g] = wx[:, a] * wy[:, b] * wz[:, g]
    return i, j, k, w


def drag(st, mass, tau):
    """D [n, 3]; zero for a particle that is not alive (its a and v are never looked at)"""
    alive = np.asarray(st["status"]) == 1
    D = np.zeros((alive.size, 3))
    D[alive] = mass * (np.asarray(st["a"])[alive] - np.asarray(st["v"])[alive]) / tau
    return D


def records(axes, st, mass, tau, ids=None):
    """(cells [q] ascending, R [q, 8, 3]): the records of the occupied cells, each summed in ascending id"""
    status = np.asarray(st["status"])
    n = status.size
    ids = np.arange(n) if ids is None else np.asarray(ids)
    alive = np.nonzero(status == 1)[0]
    x = np.asarray(st["x"], dtype=np.float64)[alive]
    D = drag(st, mass, tau)[alive]
    i, j, k, w = corner_weights(axes, x)
    key = (k * axes[1].n + j) * axes[0].n + i
    order = np.lexsort((ids[alive], key))
    cells, inverse = np.unique(key, return_inverse=True)
    R = np.zeros((cells.size, 8, 3))
    for p in order:  # (one particle after the other: the order of the sum is the order of the ids)
        R[inverse[p]] += w[p][:, None] * D[p][None, :]
    return cells, R


def colour_of(axes, cells):
    nx, ny = axes[0].n, axes[1].n
    i, j, k = cells % nx, (cells // nx) % ny, cells // (nx * ny)
    return (i % 2) + 2 * (j % 2) + 4 * (k % 2)


def corner_vertices(axes, cells):
    """[q, 8] flat vertex indices (k ny + j) nx + i of the corners, node n of a periodic direction being node 0"""
    nx, ny, nz = (ax.n for ax in axes)
    i, j, k = cells % nx, (cells // nx) % ny, cells // (nx * ny)
    out = np.empty((cells.size, 8), dtype=np.int64)
    for g in range(2):
        for b in range(2):
            for a in range(2):
                node = []
                for v, ax in ((i + a, axes[0]), (j + b, axes[1]), (k + g, axes[2])):
                    assert ax.periodic or np.all(v < ax.n)  # (a non-periodic direction's last cell is n - 2)
                    node.append(v % ax.n)
                out[:, a + 2 * b + 4 * g] = (node[2] * ny + node[1]) * nx + node[0]
    return out


def touched_twice(axes, cells):
    """does any colour touch a vertex more than once?"""
    col = colour_of(axes, cells)
    verts = corner_vertices(axes, cells)
    for c in range(8):
        v = verts[col == c].ravel()
        if np.unique(v).size != v.size:
            return True
    return False


def inverse_volumes(axes):
    """[nz, ny, nx] of 1 / (dx_i dy_j dz_k)"""
    dx, dy, dz = (dual_widths(ax) for ax in axes)
    return 1.0 / (dx[None, None, :] * dy[None, :, None] * dz[:, None, None])


def field(axes, st, mass, tau, ids=None):
    """the three [nz, ny, nx] arrays of f, vertex sums in colour order"""
    nx, ny, nz = (ax.n for ax in axes)
    cells, R = records(axes, st, mass, tau, ids)
    col = colour_of(axes, cells)
    verts = corner_vertices(axes, cells)
    inv = inverse_volumes(axes).ravel()
    f = np.zeros((3, nz * ny * nx))
    for c in range(8):
        sel = np.nonzero(col == c)[0]
        for q in sel:
            for comp in range(3):
                f[comp][verts[q]] += -R[q, :, comp] * inv[verts[q]]
    return [f[c].reshape(nz, ny, nx) for c in range(3)]


def contributions(axes, st, mass, tau):
    """sum over the cells of |R| / V per vertex and component: what the FP32 bound of an add is made of"""
    nx, ny, nz = (ax.n for ax in axes)
    cells, R = records(axes, st, mass, tau)
    verts = corner_vertices(axes, cells)
    inv = inverse_volumes(axes).ravel()
    f = np.zeros((3, nz * ny * nx))
    for q in range(cells.size):
        for comp in range(3):
            np.add.at(f[comp], verts[q], np.abs(R[q, :, comp]) * inv[verts[q]])
    return [f[c].reshape(nz, ny, nx) for c in range(3)]


def total_drag(st, mass, tau):
    return drag(st, mass, tau).sum(axis=0)


def integral(axes, f):
    """sum f V per component"""
    vol = 1.0 / inverse_volumes(axes)
    return np.array([float(np.sum(a * vol)) for a in f])


# ---------------------------------------------------------------- the composed step
class FeedbackHit:
    """forcing_ref.HitRef without band forcing, with inertial particles: a step is the sub-step loop with f of the particle
    state of the previous iteration added to the derivatives, then the particles' update from the new fields"""

    def __init__(self, dims, L, x0, tau, mass, order=4, two_way=True, v0=None, **hit_kw):
        import forcing_ref as F
        self.h = F.HitRef(dims, L, forcing_kw=None, **hit_kw)
        self.orc = self.h.orc
        o = self.h.o
        self.axes = [P.Axis(np.arange(n) * (float(l) / n), float(l), True) for n, l in zip(dims, L)]
        self.tau, self.mass, self.order, self.two_way = float(tau), float(mass), int(order), bool(two_way)
        self.dt = float(o.dt)
        self.st = P.prime(self.axes, self.h.fields(), x0, self.order, tau=self.tau, v0=v0)
        self.first = True
        self.f = self._term()

    def _term(self):
        return field(self.axes, self.st, self.mass, self.tau) if self.two_way else None

    def fields(self):
        return self.h.fields()

    def step(self):
        o, orc = self.h.o, self.orc
        b = o.backend
        curr = [o.u, o.v, o.w]
        for _ in range(o.time_integrator.nstage):
            deriv = [b.get_block(orc.DIR_X) for _ in range(3)]
            o.transeq(deriv, curr)
            if self.f is not None:
                for d, f in zip(deriv, self.f):
                    a = self.h.get(d) + f
                    d.data_loc = orc.VERT
                    b.set_field_data(d, a)
            o.time_integrator.step(curr, deriv, o.dt)
            o.pressure_correction(o.u, o.v, o.w)
            del deriv
        self.st, _ = P.update(self.axes, self.h.fields(), self.st, self.dt, self.order, self.first, tau=self.tau)
        self.first = False
        self.f = self._term()
