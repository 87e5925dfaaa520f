"""Restatement of the subgrid scalar flux of the explicit LES (Les.add with species, csrc/les.hip's x3d_les_scalar_flux) for
the tests, in numpy.longdouble from arrays [nz, ny, nx]; takes nothing from the library.

    kappa = nu_t / Pr_t        q_j = kappa dphi/dx_j        sgs_phi = sum_j d/dx_j q_j        row = sum kappa |grad phi|^2

The pointwise bound of the GPU tests: the kernel forms kappa = nu_t * (1 / Pr_t) and q_j = kappa * g_j in double, two
roundings, and stores q_j (FP64: exactly): |q_j - ref| <= 2 2^-52 |kappa g_j|.  The host hands 1 / Pr_t over as a double; the
restatement takes THAT double, so its rounding is no part of the comparison."""
import math

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def kappa(nut, inv_prt, dtype=LD):
    return np.asarray(nut, dtype=dtype) * dtype(inv_prt)


def flux(nut, gphi, inv_prt, dtype=LD, drop=None):
    """[q_x, q_y, q_z] from the three gradient arrays of one species; drop = 0..2: that component's gradient is left out (the
    mutation check)"""
    k = kappa(nut, inv_prt, dtype)
    return [np.zeros_like(k) if j == drop else k * np.asarray(g, dtype=dtype) for j, g in enumerate(gphi)]


def flux_bound(nut, gphi, inv_prt):
    """per component, float64: 2 2^-52 |kappa g_j|"""
    return [np.asarray(2.0 * LD(EPS) * np.abs(q), dtype=np.float64) for q in flux(nut, gphi, inv_prt)]


def row_terms(nut, gphi, inv_prt, dtype=LD):
    """kappa ((g_x^2 + g_y^2) + g_z^2) per point"""
    gx, gy, gz = (np.asarray(g, dtype=dtype) for g in gphi)
    return kappa(nut, inv_prt, dtype) * ((gx * gx + gy * gy) + gz * gz)


def row(nut, gphi, inv_prt):
    """the sum of the terms, exactly rounded (math.fsum of the terms as doubles of their longdouble values is not used: the
    terms are split into a double head and tail first, so that fsum sees all their bits)"""
    t = row_terms(nut, gphi, inv_prt).ravel()
    head = np.asarray(t, dtype=np.float64)
    tail = np.asarray(t - head.astype(LD), dtype=np.float64)
    return math.fsum(list(head) + list(tail))


def dense_scalar_term(phi, nut, ops, inv_prt):
    """(sgs_phi, [g_x, g_y, g_z], kappa) in float64 from vertex fields [nz, ny, nx] with the dense der1st operators
    ops = [x, y, z] of les_ref.dense_der1st; array axis of direction d is 2 - d"""
    import util
    der = lambda f, d: util.dense_apply(ops[d], f, 2 - d)
    g = [der(np.asarray(phi, dtype=np.float64), d) for d in range(3)]
    k = np.asarray(nut, dtype=np.float64) * float(inv_prt)
    sgs = sum(der(k * g[d], d) for d in range(3))
    return sgs, g, k


def noisy_phi(dims, offset=(0, 0, 0), local_dims=None, amp=0.05, salt=4):
    """a smooth field plus amp * util.hash_noise on the box [offset, offset + local_dims) of a periodic grid of `dims`
    vertices, from GLOBAL indices (every rank of a decomposed run gets the bits of the one-rank field); arrays [k, j, i]"""
    import util
    ox, oy, oz = (int(v) for v in offset)
    nx, ny, nz = (int(v) for v in (dims if local_dims is None else local_dims))
    gi = np.arange(ox, ox + nx)[None, None, :]
    gj = np.arange(oy, oy + ny)[None, :, None]
    gk = np.arange(oz, oz + nz)[:, None, None]
    twopi = 6.283185307179586
    x, y, z = gi * (twopi / dims[0]), gj * (twopi / dims[1]), gk * (twopi / dims[2])
    return np.cos(x) * np.sin(2 * y) * np.cos(z) + 0.3 * np.sin(x + z) + amp * util.hash_noise(gi, gj, gk, salt)
