"""numpy restatement of the loads and the probes (x3d2_amd/loads.py, x3d2_amd/probes.py, csrc/ibm.hip, csrc/probe.hip), written
from their definitions, not from the product's code:

    impulse_c = sum over the points of the work list of (((1 - ep1) f_c) w_x[i]) (w_y[j] w_z[k]),   all in float64

with w_d formed here from the vertex coordinates; the nearest-vertex rule (ties to the lower index); and the
Strouhal number of a uniformly sampled series."""
import math

import numpy as np


def weights(mesh):
    """w_x, w_y, w_z of a ONE-RANK mesh, straight from its vertex coordinates: 1/2 (x[i+1] - x[i-1]); at the ends of a
    periodic direction the neighbour across the period (its coordinate shifted by the length), at the ends of any other the
    one-sided difference x[1] - x[0], x[n-1] - x[n-2].  Nothing of the product's spacing tables is used: for a uniform
    direction the product holds 1 / (1 / d) instead, which differs from this by the rounding of the coordinates, at most
    an ulp of the length per difference (weights_tolerance)."""
    assert all(int(p) == 1 for p in mesh.nproc_dir)
    out = []
    for d in range(3):
        x = [float(v) for v in mesh.vert_coords[d]]
        n, length = len(x), float(mesh.L[d])
        w = [0.5 * (x[i + 1] - x[i - 1]) for i in range(1, n - 1)]
        if bool(mesh.periodic_BC[d]):
            w = [0.5 * (x[1] - (x[n - 1] - length))] + w + [0.5 * ((x[0] + length) - x[n - 2])]
        else:
            w = [x[1] - x[0]] + w + [x[n - 1] - x[n - 2]]
        out.append(np.array(w, dtype=np.float64))
    return out


def weights_tolerance(mesh, d):
    """how far a weight of direction d formed from rounded coordinates may lie from the exact spacing: coordinates up to
    the length L carry half an ulp of L each, the difference one rounding more"""
    return 2.0 * float(np.spacing(float(mesh.L[d])))


def terms(ep1, f, w):
    """[nz, ny, nx] float64: the term of every point (zero where ep1 = 1), the products in the definition's order; ep1 and f
    hold the values the device holds (float32 values in the FP32 flavour), widened here"""
    m = np.asarray(ep1).astype(np.float64)
    wx, wy, wz = (np.asarray(a, dtype=np.float64) for a in w)
    return (((1.0 - m) * np.asarray(f).astype(np.float64)) * wx[None, None, :]) * (wy[None, :, None] * wz[:, None, None])


def impulse(ep1, u, v, w_field, w):
    """(row [3], sum |terms| [3]) of one body call: math.fsum of the terms, so the reference's own error is one rounding"""
    row, mag = np.zeros(3), np.zeros(3)
    for c, f in enumerate((u, v, w_field)):
        t = terms(ep1, f, w).ravel()
        row[c], mag[c] = math.fsum(t), math.fsum(np.abs(t))
    return row, mag


def masked_volume(ep1, w):
    """sum (1 - ep1) w_x w_y w_z, the products in the definition's order with f = 1"""
    return math.fsum(terms(ep1, np.ones(np.shape(ep1)), w).ravel())


def nearest_vertex(coords, x, periodic=False, length=None):
    """index of the vertex nearest to the scalar x by exhaustive search; a tie goes to the lower index.  periodic: the image
    of the first vertex at coords[0] + length competes as index 0."""
    c = [float(v) for v in coords]
    hi = float(length) if periodic else c[-1]
    if x < c[0] or x > hi:
        raise ValueError("outside the domain")
    cand = [(abs(x - v), i) for i, v in enumerate(c)]
    if periodic:
        cand.append((abs(x - (c[0] + float(length))), 0))
    return min(cand)[1]  # (tuples compare distance first, then index: the lower index wins a tie)


def strouhal(t, y, length_ref, u_ref):
    """the frequency of the largest periodogram value of y - mean(y), by direct evaluation of the DFT power at the bins, then
    the three-point parabola through the logarithms of the peak and its neighbours"""
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = y.size
    dt = (t[-1] - t[0]) / (n - 1)
    y = y - y.mean()
    j = np.arange(n)
    power = np.array([abs(np.sum(y * np.exp(-2j * np.pi * k * j / n))) ** 2 for k in range(n // 2 + 1)])
    k = 1 + int(np.argmax(power[1:]))
    pos = float(k)
    if k + 1 < power.size:
        a, b, c = np.log(power[k - 1:k + 2])
        pos += 0.5 * (a - c) / (a - 2.0 * b + c)
    return pos / (n * dt) * length_ref / u_ref
