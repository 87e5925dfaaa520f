"""numpy restatement of the active-scalar rules of x3d2_amd/scalars.py (csrc/scalars.hip).  Nothing is taken from the library:
the three formulas, the face stamp, the five plane sums (math.fsum), the Nusselt definitions and one sub-step composed from the
oracle's pieces (oracle/x3d_oracle.py: Solver.transeq, transeq_species, TimeIntegrator.step with nvars = 3 + ns,
pressure_correction) with the coupling term and the stamps in numpy.

    d_i    += up_i sum_s ri_s (phi_s - ref_s)
    dphi_s += -(G_s,x u + G_s,y v + G_s,z w)
    phi_s   = value on a face, directions in the order x, y, z (a shared edge takes the later direction's value)

Arrays are [nz, ny, nx], x fastest, as the library's get_field_data returns them."""
import math

import numpy as np


# ---------------------------------------------------------------- the three formulas
def couple(d, dphi, vel, phi, up, ri, ref, grad=None):
    """-> (new d[3], new dphi[ns], mag_d[3], mag_phi[ns]) in longdouble; mag = |d| + sum |terms|, what a rounding bound
    scales with"""
    ld = np.longdouble
    ns = len(phi)
    buoy = np.zeros(np.shape(phi[0]), dtype=ld)
    mag_b = np.zeros_like(buoy)
    for s in range(ns):
        buoy += ld(ri[s]) * (np.asarray(phi[s], dtype=ld) - ld(ref[s]))
        mag_b += abs(ld(ri[s])) * (np.abs(np.asarray(phi[s], dtype=ld)) + abs(ld(ref[s])))
    out_d, mag_d = [], []
    for i in range(3):
        out_d.append(np.asarray(d[i], dtype=ld) + ld(up[i]) * buoy)
        mag_d.append(np.abs(np.asarray(d[i], dtype=ld)) + abs(ld(up[i])) * mag_b)
    out_p, mag_p = [], []
    for s in range(ns):
        g = (0.0, 0.0, 0.0) if grad is None else grad[s]
        adv = sum(ld(g[i]) * np.asarray(vel[i], dtype=ld) for i in range(3))
        out_p.append(np.asarray(dphi[s], dtype=ld) - adv)
        mag_p.append(np.abs(np.asarray(dphi[s], dtype=ld)) + sum(abs(ld(g[i])) * np.abs(np.asarray(vel[i], dtype=ld)) for i in range(3)))
    return out_d, out_p, mag_d, mag_p


def stamp(a, wall):
    """wall: [(lo, hi)] * 3 for x, y, z, each None or a value; in place on a [nz, ny, nx] array, x then y then z"""
    for d, ax in ((0, 2), (1, 1), (2, 0)):
        lo, hi = wall[d]
        sl = [slice(None)] * 3
        if lo is not None:
            sl[ax] = 0
            a[tuple(sl)] = lo
        if hi is not None:
            sl[ax] = a.shape[ax] - 1
            a[tuple(sl)] = hi
    return a


# ---------------------------------------------------------------- plane sums
def plane_sums(u, v, w, phi, dir_keep):
    """-> (sums[5][n_keep] by math.fsum, mags[5][n_keep] = sum |terms|, n_plane) for one species; moments phi, phi phi,
    u phi, v phi, w phi; dir_keep 2 (y) or 3 (z)"""
    ax = {2: 1, 3: 0}[dir_keep]
    n = phi.shape[ax]
    terms = [phi, phi * phi, u * phi, v * phi, w * phi]
    sums, mags = np.zeros((5, n)), np.zeros((5, n))
    for m, t in enumerate(terms):
        for q in range(n):
            pl = np.take(t, q, axis=ax).ravel()
            sums[m, q] = math.fsum(pl)
            mags[m, q] = math.fsum(np.abs(pl))
    return sums, mags, phi.size // n


# ---------------------------------------------------------------- Nusselt numbers
def slope_at_first(c, f):
    """derivative at c[0] of the parabola through the first three points (Lagrange form)"""
    x0, x1, x2 = (float(x) for x in c[:3])
    return (f[0] * ((x0 - x1) + (x0 - x2)) / ((x0 - x1) * (x0 - x2)) + f[1] * (x0 - x2) / ((x1 - x0) * (x1 - x2))
            + f[2] * (x0 - x1) / ((x2 - x0) * (x2 - x1)))


def nusselt(c, phi_mean, upphi_mean, kappa, dphi):
    """nu_lo, nu_hi = -kappa dphi_mean/dn at the two walls over kappa dphi / H; nu_vol = 1 + <up-component phi>_V H / (kappa dphi),
    the volume mean by the trapezoid rule on c"""
    c = np.asarray(c, dtype=np.float64)
    H = c[-1] - c[0]
    flux_ref = kappa * dphi / H
    nu_lo = -kappa * slope_at_first(c, phi_mean) / flux_ref
    nu_hi = -kappa * slope_at_first(c[::-1], np.asarray(phi_mean)[::-1]) / flux_ref
    q = np.asarray(upphi_mean, dtype=np.float64)
    vol = 0.0
    for j in range(len(c) - 1):
        vol += 0.5 * (q[j] + q[j + 1]) * (c[j + 1] - c[j])
    vol /= H
    return nu_lo, nu_hi, 1.0 + vol * H / (kappa * dphi)


# ---------------------------------------------------------------- the composed sub-step
class RayleighBenardRef:
    """Rayleigh-Benard in free-fall units on the oracle: Re = sqrt(Ra / Pr), one species with nu = 1 / (Re Pr), walls phi = 1
    (y = 0) and 0 (y = H), u = v = w = 0 on both, buoyancy ri = 1 along y.  step() is base_case's sub-step loop:
    transeq, transeq_species, + coupling, stage, wall stamps, pressure correction."""

    def __init__(self, dims, L, Ra=1e6, Pr=1.0, stretching="uniform", beta=0.259065151, dt=2e-3, time_intg="RK3",
                 noise=1e-3, seed=None, phi0=None, vel0=None):
        from oracle import x3d_oracle as orc
        self.orc = orc
        mesh = orc.Mesh(list(dims), [1, 1, 1], list(L), ["periodic"] * 2, ["dirichlet"] * 2, ["periodic"] * 2,
                        stretching=("uniform", stretching, "uniform"), beta=(1.0, beta, 1.0))
        Re = math.sqrt(Ra / Pr)
        self.o = o = orc.Solver(mesh, Re=Re, dt=dt, time_intg=time_intg, poisson="FFT")
        self.kappa = 1.0 / Re / Pr
        b = o.backend
        self.phi = b.get_block(orc.DIR_X, orc.VERT)
        self.ti = orc.TimeIntegrator(b, time_intg, nvars=4)
        self.H = float(mesh.L[1])
        self.y = np.asarray(mesh.vert_coords[1], dtype=np.float64)
        nx, ny, nz = (int(n) for n in dims)
        y = self.y[None, :, None]
        for f in (o.u, o.v, o.w):
            f.data_loc = orc.VERT
            f.data[...] = 0.0
        if vel0 is not None:
            for f, a in zip((o.u, o.v, o.w), vel0):
                b.set_field_data(f, np.ascontiguousarray(a, dtype=np.float64))
        if phi0 is None:
            phi0 = (1.0 - y / self.H) * np.ones((nz, ny, nx))
            if noise != 0.0:
                r = np.random.default_rng(seed).random((nz, ny, nx))
                phi0 = phi0 + noise * np.sin(np.pi * y / self.H) * (2.0 * r - 1.0)
        phi0 = stamp(np.array(phi0, dtype=np.float64), [(None, None), (1.0, 0.0), (None, None)])
        b.set_field_data(self.phi, phi0)

    def get(self, f):
        return self.o.backend.get_field_data(f, self.orc.VERT)

    def fields(self):
        o = self.o
        return [self.get(f) for f in (o.u, o.v, o.w, self.phi)]

    def step(self):
        o, orc = self.o, self.orc
        b = o.backend
        curr = [o.u, o.v, o.w, self.phi]
        for _ in range(self.ti.nstage):
            deriv = [b.get_block(orc.DIR_X) for _ in range(4)]
            o.transeq(deriv[:3], curr[:3])
            o.transeq_species(deriv[3:], curr, [self.kappa])
            # the coupling term: dv += 1 * (phi - 0)
            dv = self.get(deriv[1]) + self.get(self.phi)
            deriv[1].data_loc = orc.VERT
            b.set_field_data(deriv[1], dv)
            self.ti.step(curr, deriv, o.dt)
            for f in (o.u, o.v, o.w):
                a = self.get(f)
                a[:, 0, :] = 0.0
                a[:, -1, :] = 0.0
                b.set_field_data(f, a)
            b.set_field_data(self.phi, stamp(self.get(self.phi), [(None, None), (1.0, 0.0), (None, None)]))
            o.pressure_correction(o.u, o.v, o.w)
            del deriv

    def kinetic_energy(self):
        u, v, w, _ = self.fields()
        return 0.5 * float(np.mean(u * u + v * v + w * w))

    def monitor(self):
        """plane means along y of phi and v phi, min / max, and the three Nusselt numbers"""
        u, v, w, phi = self.fields()
        sums, _, n_plane = plane_sums(u, v, w, phi, 2)
        means = sums / n_plane
        nu_lo, nu_hi, nu_vol = nusselt(self.y, means[0], means[3], self.kappa, 1.0)
        return {"phi": means[0], "vphi": means[3], "phi_min": float(phi.min()), "phi_max": float(phi.max()), "nu_lo": nu_lo,
                "nu_hi": nu_hi, "nu_vol": nu_vol}
