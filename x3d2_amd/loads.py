"""Loads: the force the immersed boundary puts on the body, as a series, reduced on the device (csrc/ibm.hip).

This is the DIRECT-FORCING ESTIMATE: the momentum the forcing takes out of the fluid, per step.  ibm_t%body (src/module/
ibm.f90:148-170) multiplies the velocity by ep1; what it removes from component c in one sub-step is the impulse

    I_c = sum over the points of the work list of (1 - ep1) f_c w_x[i] w_y[j] w_z[k],

f_c the value about to be masked, w_d = 1 / (the inverse spacing of diagnostics.spacing_tables): 1/2 (x[i+1] - x[i-1]) of
the GLOBAL vertex coordinates, one-sided at a wall, the period's wrap in a periodic direction.  Every factor is a double
before any product and the products are taken as (((1 - m) f) w_x) (w_y w_z).  A row of step n is the sum of I_c over that
step's sub-steps; the force on the body is F_c = row_c / dt and the coefficient C_c = 2 F_c / (u_ref^2 area_ref).  The
reference's FIXME about dt * grad p inside the solid (ibm.f90:160-162) applies to it: the pressure gradient that the
correction adds inside the body after the mask is part of what the next sub-step's mask removes.

The sample rides on the body's own launch (x3d_ibm_body_loads: the same mapping and expression as x3d_ibm_body, so the
fields get the same bits) plus ONE small finishing launch per sub-step; nothing waits for the host, and because a sample
reads what the sub-steps see, not the completed state, Loads has no reads_state: it does not switch off BaseCase.run's
more=True deferral.  Ibm.body asks begin_body() where the row goes; Loads counts the body calls since its construction
against time_integrator.nstage to know the iteration and the sub-step, so every body call has to come from BaseCase.step.

Tables, ring, file: the diagnostics series' (diagnostics.Series, here for a row of 4 doubles that are all sums over the
ranks).  A row is 4 doubles: I_u, I_v, I_w and a reserved slot that holds zero.  File `<prefix>.csv`:
time, fx, fy, fz, cx, cy, cz."""
import ctypes

import numpy as np

from . import _lib
from .common import X3dError, sample_due
from .diagnostics import Series, spacing_tables

NSLOT = 4
COLUMNS = ("fx", "fy", "fz", "cx", "cy", "cz")


class LoadsConfig:
    """when to sample (as DiagnosticsConfig: from iteration initload on, every iloadfreq iterations; initload <= 0: never),
    where to write, how many rows a device table holds, and the reference velocity and area of the coefficients
    (area_ref=None: the case's own, Ibm.area_ref -- make_cylinder sets D * L_z of its default body)"""

    def __init__(self, initload=1, iloadfreq=1, prefix="loads", flush_every=256, u_ref=1.0, area_ref=None):
        self.initload, self.iloadfreq = int(initload), int(iloadfreq)
        if self.iloadfreq < 1:
            raise X3dError("LoadsConfig: iloadfreq must be at least 1")
        self.prefix = str(prefix)
        self.flush_every = int(flush_every)
        if self.flush_every < 1:
            raise X3dError("LoadsConfig: flush_every must be at least 1")
        self.u_ref = float(u_ref)
        if not self.u_ref > 0.0:
            raise X3dError("LoadsConfig: u_ref must be positive")
        self.area_ref = None if area_ref is None else float(area_ref)
        if self.area_ref is not None and not self.area_ref > 0.0:
            raise X3dError("LoadsConfig: area_ref must be positive")

    def sample_due(self, it):
        return sample_due(it, self.initload, self.iloadfreq)


def weights(mesh):
    """this rank's three tables of quadrature weights (float64, one value per local vertex): 1 / spacing_tables"""
    return [np.ascontiguousarray(1.0 / ih) for ih in spacing_tables(mesh)]


def strouhal(t, series, length_ref, u_ref):
    """the Strouhal number f length_ref / u_ref of a uniformly sampled series: the mean is removed, f is the peak of the
    periodogram refined by three-point parabolic interpolation (on the log of the power; a peak at the first or the last
    bin is taken as it is).  Fewer than 8 rows, a t that is not uniform, or a constant series: an error.  Pure host."""
    t, y = np.asarray(t, dtype=np.float64).ravel(), np.asarray(series, dtype=np.float64).ravel()
    if t.size != y.size:
        raise X3dError("strouhal: t and the series differ in length")
    n = int(t.size)
    if n < 8:
        raise X3dError("strouhal: %d rows, at least 8 are needed" % n)
    steps = np.diff(t)
    dt = float(t[-1] - t[0]) / (n - 1)
    if not dt > 0.0 or float(np.max(np.abs(steps - dt))) > 1e-6 * dt:
        raise X3dError("strouhal: t is not uniformly sampled")
    if not float(u_ref) > 0.0 or not float(length_ref) > 0.0:
        raise X3dError("strouhal: length_ref and u_ref must be positive")
    power = np.abs(np.fft.rfft(y - np.mean(y))) ** 2
    if not float(np.max(power[1:])) > 0.0:
        raise X3dError("strouhal: the series has no variance")
    k = int(np.argmax(power[1:])) + 1
    pos = float(k)
    if 1 <= k < power.size - 1 and power[k - 1] > 0.0 and power[k + 1] > 0.0:
        a, b, c = (float(np.log(power[j])) for j in (k - 1, k, k + 1))
        den = a - 2.0 * b + c
        if den < 0.0:
            pos += min(max(0.5 * (a - c) / den, -0.5), 0.5)
    return pos / (n * dt) * float(length_ref) / float(u_ref)


class Loads(Series):
    """Loads(solver, cfg, append=False), attached as `case.loads = Loads(case.solver, cfg, append=case.restarted)`; it sets
    solver.ibm.loads to itself.  BaseCase.run polls it once per step, flushes it before a checkpoint and finalises it at
    the end.  Needs the sparse immersed boundary (an Ibm with iibm = 1 made without X3D_NO_IBM_SPARSE=1)."""

    def __init__(self, solver, cfg, append=False):
        ibm = getattr(solver, "ibm", None)
        if ibm is None:
            raise X3dError("Loads: the solver has no immersed boundary (solver.ibm)")
        if ibm.iibm != 1:
            raise X3dError("Loads: the immersed boundary is off (iibm = %d)" % ibm.iibm)
        if ibm.h is None:
            raise X3dError("Loads: the work-list form of the immersed boundary is needed (X3D_NO_IBM_SPARSE=1 is set)")
        self.cfg = cfg
        self.area_ref = cfg.area_ref if cfg.area_ref is not None else getattr(ibm, "area_ref", None)
        if self.area_ref is None:
            raise X3dError("Loads: area_ref is not given and the case supplies none")
        super().__init__(solver, "Loads", cfg.prefix, cfg.flush_every, NSLOT, COLUMNS, append)
        self.w_host = weights(solver.mesh)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(solver.backend.lib.x3d_ibm_set_weights(ibm.h, *[w.ctypes.data_as(dp) for w in self.w_host]))
        self.nstage = int(solver.time_integrator.nstage)
        self._it0 = int(solver.current_iter)
        self._calls = 0     # body calls since construction: call n belongs to iteration it0 + 1 + n // nstage
        self._open = False  # a row is being written by the current body call
        self.ibm = ibm
        ibm.loads = self

    def begin_body(self):
        """Ibm.body, before its launch: (device address of the row, accumulate) if this body call's step is due, else
        None"""
        n = self._calls
        self._calls += 1
        it, sub = self._it0 + 1 + n // self.nstage, n % self.nstage
        if sub == 0 and it != int(self.solver.current_iter) + 1:  # (a body call from outside BaseCase.step shifted the count)
            self._calls = n
            raise X3dError("Loads: body call %d would belong to iteration %d, the solver is about to take iteration %d; "
                           "every Ibm.body call must come from BaseCase.step" % (n, it, int(self.solver.current_iter) + 1))
        self._open = self.cfg.sample_due(it)
        if not self._open:
            return None
        self._last = sub == self.nstage - 1
        return self.row_address(it), int(sub > 0)

    def end_body(self):
        """Ibm.body, behind its launch: the last sub-step closes the row (and a full table starts its copy)"""
        if self._open and self._last:
            self.commit()
        self._open = False

    def values(self, raw):
        """fx, fy, fz, cx, cy, cz of a raw row"""
        f = [float(raw[c]) / float(self.solver.dt) for c in range(3)]
        q = 2.0 / (self.cfg.u_ref ** 2 * self.area_ref)
        return f + [q * v for v in f]
