"""numpy restatement of the diagnostics series (x3d2_amd/diagnostics.py, csrc/diagnostics.hip): the sixteen raw slots of a
row in float64 with exactly rounded sums (math.fsum), the derived columns, the spacing tables and the file format.  Written
from the definitions, not from the product's code; tests/test_diagnostics_host.py pins it to closed forms."""
import math

import numpy as np

NSLOT = 16
GRAD_NAMES = ("ux", "uy", "uz", "vx", "vy", "vz", "wx", "wy", "wz")


def fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).reshape(-1).tolist())


def row(u, v, w, grads, ih, flags):
    """the raw row of arrays [nz, ny, nx]; grads in GRAD_NAMES' order; ih = (ih_x[nx], ih_y[ny], ih_z[nz]); flags =
    (first_y, last_y).  Slots 7 and 13 (the divergence's) stay 0."""
    u, v, w = (np.asarray(a, dtype=np.float64) for a in (u, v, w))
    ux, uy, uz, vx, vy, vz, wx, wy, wz = (np.asarray(g, dtype=np.float64) for g in grads)
    r = np.zeros(NSLOT)
    r[0], r[1], r[2] = fsum(u * u), fsum(v * v), fsum(w * w)
    w2 = (wy - vz) ** 2 + (uz - wx) ** 2 + (vx - uy) ** 2
    r[3] = fsum(w2)
    r[4] = fsum(ux ** 2 + vy ** 2 + wz ** 2 + 0.5 * ((uy + vx) ** 2 + (uz + wx) ** 2 + (vz + wy) ** 2))
    r[5] = fsum(uy[:, 0, :]) if flags[0] else 0.0
    r[6] = fsum(uy[:, -1, :]) if flags[1] else 0.0
    r[8], r[9], r[10] = np.abs(u).max(), np.abs(v).max(), np.abs(w).max()
    r[11] = w2.max()
    ihx, ihy, ihz = (np.asarray(t, dtype=np.float64) for t in ih)
    r[12] = (np.abs(u) * ihx[None, None, :] + np.abs(v) * ihy[None, :, None] + np.abs(w) * ihz[:, None, None]).max()
    return r


def grad_square_sum(grads):
    """A = sum over the points of sum_ij g_ij^2: the scale of the bounds on slots 3 and 4"""
    return fsum(sum(np.asarray(g, dtype=np.float64) ** 2 for g in grads))


def max_sum(f):
    f = np.abs(np.asarray(f, dtype=np.float64))
    return float(f.max()), fsum(f)


def column_names(divergence=True, y_walls=False):
    names = ["ke", "enstrophy", "dissipation", "u_max", "v_max", "w_max", "vort_max", "cfl"]
    if divergence:
        names += ["div_u_max", "div_u_mean"]
    if y_walls:
        names += ["tau_w_lo", "tau_w_hi"]
    return tuple(names)


def derive(r, n_vert, n_cell, n_plane, nu, dt, divergence=True, y_walls=False):
    out = {"ke": 0.5 * (r[0] + r[1] + r[2]) / n_vert, "enstrophy": 0.5 * r[3] / n_vert,
           "dissipation": 2.0 * nu * r[4] / n_vert, "u_max": r[8], "v_max": r[9], "w_max": r[10],
           "vort_max": math.sqrt(r[11]), "cfl": dt * r[12]}
    if divergence:
        out["div_u_max"], out["div_u_mean"] = r[13], r[7] / n_cell
    if y_walls:
        out["tau_w_lo"], out["tau_w_hi"] = nu * r[5] / n_plane, -nu * r[6] / n_plane
    return out


def inverse_spacing(y, periodic, length):
    """1 / h, h[j] = (y[j+1] - y[j-1]) / 2 with the neighbours taken around a periodic direction, one-sided at the ends of
    any other"""
    y = [float(c) for c in y]
    n = len(y)
    out = []
    for j in range(n):
        if 0 < j < n - 1:
            h = (y[j + 1] - y[j - 1]) / 2
        elif periodic:
            h = ((y[1] - (y[n - 1] - length)) if j == 0 else ((y[0] + length) - y[n - 2])) / 2
        else:
            h = (y[1] - y[0]) if j == 0 else (y[n - 1] - y[n - 2])
        out.append(1.0 / h)
    return np.array(out)


def es20_12(x):
    """one value as Fortran's ES20.12 writes it (two-digit exponents; Python's form beyond)"""
    return "%20.12E" % float(x)


def format_row(t, values):
    return ",".join(es20_12(v) for v in [t] + list(values)) + "\n"


def format_header(columns):
    return "# time" + "".join(", " + c for c in columns) + "\n"


def tgv_fields(n):
    """the Taylor-Green initial condition on n^3 vertices of [0, 2 pi)^3 and its exact gradients, arrays [nz, ny, nx]"""
    c = 2.0 * math.pi * np.arange(n) / n
    x, y, z = c[None, None, :], c[None, :, None], c[:, None, None]
    sx, cx, sy, cy, cz, sz = np.sin(x), np.cos(x), np.sin(y), np.cos(y), np.cos(z), np.sin(z)
    one = np.ones((n, n, n))
    u, v, w = sx * cy * cz * one, -cx * sy * cz * one, 0.0 * one
    grads = [cx * cy * cz * one, -sx * sy * cz * one, -sx * cy * sz * one,
             sx * sy * cz * one, -cx * cy * cz * one, cx * sy * sz * one,
             0.0 * one, 0.0 * one, 0.0 * one]
    return u, v, w, grads
