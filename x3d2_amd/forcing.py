"""Band forcing of a three-periodic box: a term that holds the large scales of isotropic turbulence, on the device without a
transform (csrc/forcing.hip).  Not in the reference (x3d2 has no forcing): this project's addition.

    case = make_hit(128, forcing=ForcingConfig(scheme="power", power=0.1, k_hi=2.5))     # or, on any three-periodic solver:
    solver.forcing = Forcing(solver, ForcingConfig(scheme="linear", coeff=0.3, k_lo=0.5, k_hi=2.5))
    case.run(n_iters=...)
    solver.forcing.row()   # {"e_band", "d", "coeff", "power"} of the last add(): the only call that waits for the host

With U(m) = sum_x u(x) exp(-i k.x) the unnormalised DFT of the velocity on the vertex grid (numpy's rfftn), signed mode numbers
m = (mx, my, mz), k_d = 2 pi m_d / L_d, the half space mx >= 0 with Hermitian weight w = 1 for mx = 0, else 2, N the number of
points:
    band     { m != 0 : k_lo <= |k| <= k_hi }, inside the mode box M_d = floor(k_hi L_d / 2 pi)
    g        U on the band, zero elsewhere; solenoidal=True (default): g <- g - k (k.g) / |k|^2
    D        sum_band w Re(g . conj U) / N^2          E_band = 1/2 sum_band w |U|^2 / N^2
    "power"  F = (P / D) g: by Parseval the volume mean of f . u on the vertex grid is P
    "linear" F = A g
    guard    D <= d_min (default 1e-300): F = 0
    f(x)     (1 / N) sum_m w Re(F(m) exp(i k.x)): numpy's irfftn of the banded spectrum, added to du, dv, dw

Forcing.add(du, dv, dw, u, v, w), called by BaseCase.substep after the case's forcings: flush_grad, launch A (the band's
coefficients as separable sums: one read of u, v, w), on several ranks the sum of the small coefficient array over the ranks
(the collective of the statistics' plane sums), launch B (one workgroup: g, D, E_band, F and the row, all on the device), launch
C (the separable synthesis: one read-modify-write of the three derivative blocks).  No call waits for the host.  The
coefficients are recomputed at every sub-step from that sub-step's velocity: the term has no state, a checkpoint needs nothing
from it and an exact resume follows.  y and z may be cut, x never (the particles' rule).

Refused, each an X3dError before anything is allocated: a direction that is not periodic or not uniform, a cut x, a mode box
with any M_d > 8 or M_d >= n_d / 2 (a Nyquist mode can then never be in the band), an empty band, an unknown scheme, values that
are not finite.

Not built: stochastic (Eswaran-Pope) forcing; full-band Lundgren forcing; coefficients frozen over a step; forcing columns in
Diagnostics; a cut x; the Fortran shim; non-periodic directions."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .common import VERT, X3dError

SCHEMES = {"power": 0, "linear": 1}  # X3D_FORCING_POWER, X3D_FORCING_LINEAR
MMAX = 8                             # X3D_FORCING_MMAX
ROW = ("e_band", "d", "coeff", "power")


def _finite(name, x):
    if isinstance(x, (str, bytes, bool)) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(float(x)):
        raise X3dError("ForcingConfig: %s is a finite number (got %r)" % (name, x))
    return float(x)


class ForcingConfig:
    """scheme "power" (the injected power `power` is held) or "linear" (F = coeff g); the band k_lo <= |k| <= k_hi; solenoidal:
    the forcing is projected onto the divergence-free part; d_min: the guard on D"""

    def __init__(self, scheme="power", power=0.1, coeff=0.0, k_lo=0.0, k_hi=2.5, solenoidal=True, d_min=1e-300):
        self.scheme = str(scheme).lower()
        if self.scheme not in SCHEMES:
            raise X3dError("ForcingConfig: unknown scheme %r (one of %s)" % (scheme, ", ".join(SCHEMES)))
        self.power, self.coeff = _finite("power", power), _finite("coeff", coeff)
        self.k_lo, self.k_hi = _finite("k_lo", k_lo), _finite("k_hi", k_hi)
        if self.k_lo < 0.0 or self.k_hi < self.k_lo:
            raise X3dError("ForcingConfig: the band needs 0 <= k_lo <= k_hi (got %r, %r)" % (self.k_lo, self.k_hi))
        self.solenoidal = bool(solenoidal)
        self.d_min = _finite("d_min", d_min)
        if self.d_min < 0.0:
            raise X3dError("ForcingConfig: d_min must not be negative")

    @property
    def value(self):
        """what launch B takes: P or A"""
        return self.power if self.scheme == "power" else self.coeff


def mode_box(L, k_hi):
    """M_d = floor(k_hi L_d / 2 pi)"""
    return tuple(int(math.floor(float(k_hi) * float(l) / (2.0 * math.pi))) for l in L)


def band_tables(n, L, k_lo, k_hi):
    """(M, band[modes] int32, kvec[modes, 3]) of the mode box, modes in the library's order (mx slowest, then my, then mz), or an
    X3dError for a box or band that is not served; n: the global vertex dims"""
    M = mode_box(L, k_hi)
    for d in range(3):
        if M[d] > MMAX:
            raise X3dError("Forcing: the mode box reaches %d in direction %d (at most %d)" % (M[d], d, MMAX))
        if 2 * M[d] >= int(n[d]):
            raise X3dError("Forcing: the mode box reaches %d in direction %d, the Nyquist mode of its %d points" % (M[d], d, int(n[d])))
    mx = np.arange(0, M[0] + 1)[:, None, None]
    my = np.arange(-M[1], M[1] + 1)[None, :, None]
    mz = np.arange(-M[2], M[2] + 1)[None, None, :]
    shape = (M[0] + 1, 2 * M[1] + 1, 2 * M[2] + 1)
    k = [np.broadcast_to(2.0 * np.pi * m / float(l), shape) for m, l in zip((mx, my, mz), L)]
    kk = np.sqrt(k[0] ** 2 + k[1] ** 2 + k[2] ** 2)
    zero = np.broadcast_to((mx == 0) & (my == 0) & (mz == 0), shape)
    band = (kk >= float(k_lo)) & (kk <= float(k_hi)) & ~zero
    if not band.any():
        raise X3dError("Forcing: no mode lies in the band %r <= |k| <= %r" % (k_lo, k_hi))
    kvec = np.ascontiguousarray(np.stack([a.ravel() for a in k], axis=1), dtype=np.float64)
    return M, np.ascontiguousarray(band.ravel(), dtype=np.int32), kvec


def twiddle_table(n, M):
    """[n][M + 1][2] = {cos, -sin}(2 pi m g / n), the angle reduced in integers first"""
    r = (np.arange(n, dtype=np.int64)[:, None] * np.arange(M + 1, dtype=np.int64)[None, :]) % n
    a = 2.0 * np.pi * r.astype(np.float64) / float(n)
    return np.ascontiguousarray(np.stack([np.cos(a), -np.sin(a)], axis=2))


def check_served(solver):
    """X3dError for a mesh Forcing does not serve"""
    m = solver.mesh
    for d in range(3):
        if not m.periodic_BC[d]:
            raise X3dError("Forcing: direction %d is not periodic" % d)
        if m.stretched[d]:
            raise X3dError("Forcing: direction %d is not uniform" % d)
    if int(m.nproc_dir[0]) > 1:
        raise X3dError("Forcing: x is never cut (nproc_dir[0] = %d)" % int(m.nproc_dir[0]))


class Forcing:
    """Forcing(solver, cfg), attached as `solver.forcing = Forcing(solver, cfg)`"""

    coupled = True  # the term reads the completed velocity and needs the derivatives stored: BaseCase.substep's explicit branch

    def __init__(self, solver, cfg=None):
        self.cfg = cfg = cfg or ForcingConfig()
        if not isinstance(cfg, ForcingConfig):
            raise X3dError("Forcing: cfg is a ForcingConfig")
        check_served(solver)
        m = solver.mesh
        n = [int(v) for v in m.get_global_dims(VERT)]
        self.M, band, kvec = band_tables(n, [float(l) for l in m.L], cfg.k_lo, cfg.k_hi)
        # ---- nothing was allocated up to here
        self.solver = solver
        b = solver.backend
        self.lib = b.lib
        dev = lambda a: torch.from_numpy(a).to(b.device)
        self.tw = [dev(twiddle_table(n[d], self.M[d])) for d in range(3)]
        self.band, self.kvec = dev(band), dev(kvec)
        self.band_host, self.kvec_host = band, kvec
        nl = [int(v) for v in m.get_dims(VERT)]
        off = [int(o) for o in m.n_offset]
        self.prm = _lib.ForcingParams((_lib.I * 3)(*n), (_lib.I * 3)(*off), (_lib.I * 3)(*nl), (_lib.I * 3)(1, 1, 1),
                                      (_lib.I * 3)(*self.M), int(band.sum()), self.tw[0].data_ptr(), self.tw[1].data_ptr(),
                                      self.tw[2].data_ptr(), self.band.data_ptr(), self.kvec.data_ptr())
        sz = (ctypes.c_long * 4)()
        _lib.check(self.lib.x3d_forcing_sizes(ctypes.byref(self.prm), sz))
        self.nmodes = int(sz[0])
        z = lambda k: torch.zeros(int(k), dtype=torch.float64, device=b.device)
        self.uhat, self.fhat, self.part, self._row = z(sz[1]), z(sz[1]), z(sz[2]), z(sz[3])

    def reads_state(self, it):
        """does anything of this object read the solver's fields outside the sub-step?  Never: add() runs inside it"""
        return False

    # ------------------------------------------------------------ the three launches
    def project(self, u, v, w, uhat=None, reduce=True):
        """launch A (and, on several ranks, the sum over the ranks; reduce=False: this rank's block alone): uhat[3][modes][2] of
        the blocks u, v, w; no host wait"""
        uhat = self.uhat if uhat is None else uhat
        b = self.solver.backend
        _lib.check(self.lib.x3d_forcing_project(b.h, ctypes.byref(self.prm), u.ptr, v.ptr, w.ptr, self.part.data_ptr(),
                                                self.part.numel(), uhat.data_ptr()))
        if reduce and b.comm.size > 1:
            b.comm.allreduce_tensor(uhat)
        return uhat

    def coefficients(self, uhat=None):
        """launch B: fhat and the row from uhat; no host wait"""
        c = self.cfg
        uhat = self.uhat if uhat is None else uhat
        _lib.check(self.lib.x3d_forcing_coeffs(self.solver.backend.h, ctypes.byref(self.prm), uhat.data_ptr(), SCHEMES[c.scheme],
                                               c.value, int(c.solenoidal), c.d_min, self.fhat.data_ptr(), self._row.data_ptr()))
        return self.fhat

    def synthesise(self, du, dv, dw):
        """launch C: du, dv, dw += the field of fhat; no host wait"""
        _lib.check(self.lib.x3d_forcing_synth(self.solver.backend.h, ctypes.byref(self.prm), du.ptr, dv.ptr, dw.ptr,
                                              self.fhat.data_ptr(), self._row.data_ptr()))

    def add(self, du, dv, dw, u, v, w):
        """du, dv, dw += f of the velocity u, v, w; no host wait"""
        for f in (du, dv, dw, u, v, w):
            if f.data_loc != VERT:
                raise X3dError("Forcing.add: every field must be at VERT")
        self.solver.flush_grad()  # a velocity correction left pending is not in u, v, w yet
        self.project(u, v, w)
        self.coefficients()
        self.synthesise(du, dv, dw)

    # ------------------------------------------------------------ results
    def row(self):
        """{e_band, d, coeff, power} of the last add(): ONE host wait"""
        return dict(zip(ROW, (float(x) for x in self._row.cpu().numpy())))

    def coefficients_host(self):
        """(uhat, fhat) of the last add() as complex arrays [3][Mx + 1][2 My + 1][2 Mz + 1]; waits for the host"""
        shape = (3, self.M[0] + 1, 2 * self.M[1] + 1, 2 * self.M[2] + 1)
        out = []
        for t in (self.uhat, self.fhat):
            a = t.cpu().numpy().reshape(3, self.nmodes, 2)
            out.append((a[..., 0] + 1j * a[..., 1]).reshape(shape))
        return tuple(out)
