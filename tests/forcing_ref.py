"""numpy restatement of the band forcing (x3d2_amd/forcing.py, csrc/forcing.hip) and of the initial field of the isotropic
turbulence case (x3d2_amd/case.py, hit_initial_field).  Nothing is taken from the library: the band, g, D, E_band, F and the
forcing field through numpy's rfftn / irfftn with explicit axes, the separable direct sums, the initial-field recipe, and one
sub-step composed from the oracle's pieces (oracle/x3d_oracle.py: Solver.transeq, TimeIntegrator.step, pressure_correction) plus
the forcing term in numpy.

Arrays are [nz, ny, nx], x fastest, as the library's get_field_data returns them.  U(m) = rfftn(u, axes=(0, 1, 2)) is the
unnormalised DFT; the half space is mx >= 0 with Hermitian weight 1 for mx = 0 (and the Nyquist mx, which is never in a band),
else 2; signed mode numbers m_d, k_d = 2 pi m_d / L_d."""
import math

import numpy as np

AXES = (0, 1, 2)


# ---------------------------------------------------------------- the band
def mode_box(L, k_hi):
    return tuple(int(math.floor(k_hi * float(l) / (2.0 * math.pi))) for l in L)


def wave_numbers(dims, L):
    """kx [1, 1, nx/2+1], ky [1, ny, 1], kz [nz, 1, 1] of rfftn's layout"""
    nx, ny, nz = dims
    kx = (2.0 * np.pi / L[0]) * np.arange(nx // 2 + 1, dtype=np.float64)[None, None, :]
    ky = (2.0 * np.pi / L[1]) * (np.fft.fftfreq(ny) * ny)[None, :, None]
    kz = (2.0 * np.pi / L[2]) * (np.fft.fftfreq(nz) * nz)[:, None, None]
    return kx, ky, kz


def band_mask(dims, L, k_lo, k_hi):
    """bool [nz, ny, nx/2+1]: k_lo <= |k| <= k_hi without the mean; the Nyquist planes are left out (the library refuses a
    band that could reach them)"""
    nx, ny, nz = dims
    kx, ky, kz = wave_numbers(dims, L)
    k = np.sqrt(kx ** 2 + ky ** 2 + kz ** 2)
    m = (k >= k_lo) & (k <= k_hi)
    m[0, 0, 0] = False
    for n, ax in ((nz, 0), (ny, 1)):
        if n % 2 == 0:
            sl = [slice(None)] * 3
            sl[ax] = n // 2
            assert not m[tuple(sl)].any(), "the band reaches a Nyquist plane"
    if nx % 2 == 0:
        assert not m[:, :, nx // 2].any(), "the band reaches a Nyquist plane"
    return m


def weights(dims):
    nx = dims[0]
    w = np.full(nx // 2 + 1, 2.0)
    w[0] = 1.0
    if nx % 2 == 0:
        w[nx // 2] = 1.0
    return w[None, None, :]


# ---------------------------------------------------------------- the term
def forcing(vel, L, scheme="power", power=0.1, coeff=0.0, k_lo=0.0, k_hi=2.5, solenoidal=True, d_min=1e-300):
    """-> dict: f (three [nz, ny, nx] arrays), U, g, F (three rfftn-shaped complex arrays), band, e_band, d, coeff, power"""
    vel = [np.asarray(a, dtype=np.float64) for a in vel]
    nz, ny, nx = vel[0].shape
    dims = (nx, ny, nz)
    N = float(nx * ny * nz)
    U = [np.fft.rfftn(a, axes=AXES) for a in vel]
    band = band_mask(dims, L, k_lo, k_hi)
    kx, ky, kz = wave_numbers(dims, L)
    g = [np.where(band, u, 0.0) for u in U]
    if solenoidal:
        kk = kx ** 2 + ky ** 2 + kz ** 2
        kk = np.where(kk > 0.0, kk, 1.0)
        kg = (kx * g[0] + ky * g[1] + kz * g[2]) / kk
        g = [g[0] - kx * kg, g[1] - ky * kg, g[2] - kz * kg]
        g = [np.where(band, x, 0.0) for x in g]
    w = weights(dims)
    d = float(np.sum(w * sum((x * np.conj(u)).real for x, u in zip(g, U)))) / N ** 2
    e_band = 0.5 * float(np.sum(np.where(band, w * sum(np.abs(u) ** 2 for u in U), 0.0))) / N ** 2
    if d > d_min:
        c = power / d if scheme == "power" else coeff
    else:
        c = 0.0
    F = [c * x for x in g]
    f = [np.fft.irfftn(x, s=(nz, ny, nx), axes=AXES) for x in F]
    return {"f": f, "U": U, "g": g, "F": F, "band": band, "e_band": e_band, "d": d, "coeff": c, "power": c * d}


def box_index(dims, M):
    """index arrays that pick the mode box [Mx + 1][2 My + 1][2 Mz + 1] (mx slowest, then my, then mz: the library's order) out
    of an rfftn-shaped [nz, ny, nx/2+1] array"""
    nx, ny, nz = dims
    mx = np.arange(0, M[0] + 1)[:, None, None]
    my = np.arange(-M[1], M[1] + 1)[None, :, None] % ny
    mz = np.arange(-M[2], M[2] + 1)[None, None, :] % nz
    return mz, my, mx


def box_of(c, dims, M):
    """the mode box of an rfftn-shaped array, [Mx + 1][2 My + 1][2 Mz + 1]"""
    iz, iy, ix = box_index(dims, M)
    return c[iz, iy, ix]


def direct_sums(a, M):
    """U(m) on the mode box by separable direct sums, exp(-i 2 pi m g / n) per direction: [Mx + 1][2 My + 1][2 Mz + 1]"""
    a = np.asarray(a, dtype=np.float64)
    nz, ny, nx = a.shape
    ex = np.exp(-2j * np.pi * np.outer(np.arange(0, M[0] + 1), np.arange(nx)) / nx)        # [mx][i]
    ey = np.exp(-2j * np.pi * np.outer(np.arange(-M[1], M[1] + 1), np.arange(ny)) / ny)   # [my][j]
    ez = np.exp(-2j * np.pi * np.outer(np.arange(-M[2], M[2] + 1), np.arange(nz)) / nz)   # [mz][k]
    t = np.einsum("kji,ai->kja", a, ex)
    t = np.einsum("kja,bj->kab", t, ey)
    return np.einsum("kab,ck->abc", t, ez)


def spectral_divergence(f, L):
    """max |k . F| / max |F| over rfftn's modes"""
    nz, ny, nx = f[0].shape
    kx, ky, kz = wave_numbers((nx, ny, nz), L)
    F = [np.fft.rfftn(a, axes=AXES) for a in f]
    scale = max(float(np.max(np.abs(x))) for x in F)
    return float(np.max(np.abs(kx * F[0] + ky * F[1] + kz * F[2]))) / scale


# ---------------------------------------------------------------- the initial field
def initial_field(dims, L, k0=4.0, ke0=0.5, seed=0):
    """the recipe of the isotropic-turbulence case on the global grid dims = (nx, ny, nz)"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    noise = [rng.standard_normal((nz, ny, nx)) for _ in range(3)]  # u, then v, then w
    hat = [np.fft.rfftn(a, axes=AXES) for a in noise]
    kx, ky, kz = wave_numbers(dims, L)
    kk = kx ** 2 + ky ** 2 + kz ** 2
    k = np.sqrt(kk)
    shape = k * np.exp(-(k / k0) ** 2)
    hat = [h * shape for h in hat]
    for h in hat:
        h[0, 0, 0] = 0.0
        if nz % 2 == 0:
            h[nz // 2, :, :] = 0.0
        if ny % 2 == 0:
            h[:, ny // 2, :] = 0.0
        if nx % 2 == 0:
            h[:, :, nx // 2] = 0.0
    kk1 = np.where(kk > 0.0, kk, 1.0)
    kg = (kx * hat[0] + ky * hat[1] + kz * hat[2]) / kk1
    hat = [hat[0] - kx * kg, hat[1] - ky * kg, hat[2] - kz * kg]
    f = [np.fft.irfftn(h, s=(nz, ny, nx), axes=AXES) for h in hat]
    ke = 0.5 * float(np.mean(f[0] ** 2 + f[1] ** 2 + f[2] ** 2))
    a = math.sqrt(ke0 / ke)
    return [a * x for x in f]


# ---------------------------------------------------------------- the composed sub-step
class HitRef:
    """the isotropic-turbulence case on the oracle: step() is base_case's sub-step loop -- transeq, + the forcing term of the
    sub-step's velocity, stage, pressure correction"""

    def __init__(self, dims, L, Re=1600.0, dt=1e-3, time_intg="RK3", k0=4.0, ke0=0.5, seed=0, forcing_kw=None, vel0=None):
        from oracle import x3d_oracle as orc
        self.orc = orc
        self.L = tuple(float(l) for l in L)
        mesh = orc.Mesh(list(dims), [1, 1, 1], list(self.L), ["periodic"] * 2, ["periodic"] * 2, ["periodic"] * 2)
        self.o = o = orc.Solver(mesh, Re=Re, dt=dt, time_intg=time_intg, poisson="FFT")
        self.forcing_kw = forcing_kw
        self.rows = []
        vel0 = initial_field(dims, self.L, k0, ke0, seed) if vel0 is None else vel0
        for f, a in zip((o.u, o.v, o.w), vel0):
            f.data_loc = orc.VERT
            o.backend.set_field_data(f, np.ascontiguousarray(a, dtype=np.float64))

    def get(self, f):
        return self.o.backend.get_field_data(f, self.orc.VERT)

    def fields(self):
        o = self.o
        return [self.get(f) for f in (o.u, o.v, o.w)]

    def step(self):
        o, orc = self.o, self.orc
        b = o.backend
        curr = [o.u, o.v, o.w]
        for _ in range(o.time_integrator.nstage):
            deriv = [b.get_block(orc.DIR_X) for _ in range(3)]
            o.transeq(deriv, curr)
            if self.forcing_kw is not None:
                r = forcing(self.fields(), self.L, **self.forcing_kw)
                self.rows.append({k: r[k] for k in ("e_band", "d", "coeff", "power")})
                for d, f in zip(deriv, r["f"]):
                    a = self.get(d) + f
                    d.data_loc = orc.VERT
                    b.set_field_data(d, a)
            o.time_integrator.step(curr, deriv, o.dt)
            o.pressure_correction(o.u, o.v, o.w)
            del deriv

    def kinetic_energy(self):
        u, v, w = self.fields()
        return 0.5 * float(np.mean(u * u + v * v + w * w))
