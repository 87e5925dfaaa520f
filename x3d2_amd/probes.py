"""Probes: u, v, w at fixed points as a series, gathered on the device (csrc/probe.hip).

Not in the reference: this project's own addition.  Every point snaps to the NEAREST GLOBAL VERTEX per direction (a tie goes
to the lower index; a stretched direction's own coordinates are used), so a probe's value is the field's own bits -- there is
no interpolation.  A point outside the domain ([0, L] of a periodic direction, [first, last vertex] of any other) is an
error.  A sample is one launch with one thread per (owned probe, field) that writes the values, widened to double, into the
row of a device table; the slots of probes another rank owns stay at the zero the table was cleared to, and a landed table is
summed over the ranks (every slot has one owner and x + 0 = x).  No call of a sample waits for the host.

A sample reads the COMPLETED velocity of its step, like a diagnostics row: reads_state(it) is true on due steps, and
iprobefreq = 1 therefore forgoes BaseCase.run's more=True deferral on every step.

Tables, ring, file: diagnostics.Series.  File `<prefix>.csv`: time, u_0, v_0, w_0, u_1, ...; behind the header one comment line per
probe with the vertex it snapped to: `# probe <n>: vertex <i> <j> <k> (1-based, global) at x y z`."""
import ctypes

import numpy as np

from . import _lib
from .common import VERT, X3dError, sample_due
from .diagnostics import Series, global_vert_coords

MAX_PROBES = 4096  # X3D_PROBE_MAX of include/x3d2_hip.h


class ProbesConfig:
    """points: [n, 3] coordinates, 1 <= n <= 4096; when to sample (from iteration initprobe on, every iprobefreq
    iterations; initprobe <= 0: never), where to write, how many rows a device table holds"""

    def __init__(self, points, initprobe=1, iprobefreq=1, prefix="probes", flush_every=256):
        pts = np.array(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != 3 or not 1 <= pts.shape[0] <= MAX_PROBES:
            raise X3dError("ProbesConfig: points is an [n, 3] array of coordinates, 1 <= n <= %d" % MAX_PROBES)
        if not np.all(np.isfinite(pts)):
            raise X3dError("ProbesConfig: a coordinate is not finite")
        self.points = pts
        self.initprobe, self.iprobefreq = int(initprobe), int(iprobefreq)
        if self.iprobefreq < 1:
            raise X3dError("ProbesConfig: iprobefreq must be at least 1")
        self.prefix = str(prefix)
        self.flush_every = int(flush_every)
        if self.flush_every < 1:
            raise X3dError("ProbesConfig: flush_every must be at least 1")

    def sample_due(self, it):
        return sample_due(it, self.initprobe, self.iprobefreq)


def nearest_vertex(coords, x, periodic=False, length=None):
    """the 0-based index of the vertex of `coords` (ascending) nearest to every value of x; a tie goes to the lower index.
    periodic: the domain is [0, length] and a point nearer to the wrapped first vertex than to the last snaps to index 0.
    A value outside the domain (by more than 1e-12 of its length) is an error."""
    c = np.asarray(coords, dtype=np.float64)
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    hi = float(length) if periodic else float(c[-1])
    tol = 1e-12 * (hi - float(c[0]))  # (a stretched direction's first vertex can lie a rounding error above 0)
    if np.any(x < c[0] - tol) or np.any(x > hi + tol):
        raise X3dError("a probe lies outside the domain [%g, %g]" % (float(c[0]), hi))
    x = np.clip(x, c[0], hi)
    right = np.clip(np.searchsorted(c, x, side="left"), 1, c.size - 1)  # c[right - 1] <= x <= c[right] (or x beyond c[-1])
    left = right - 1
    idx = np.where(x - c[left] <= c[right] - x, left, right)
    if periodic:  # (beyond the last vertex: that one or the wrapped first, index 0 being the lower)
        idx = np.where(x > c[-1], np.where((c[0] + float(length)) - x <= x - c[-1], 0, c.size - 1), idx)
    return idx.astype(np.int64)


def snap(mesh, points):
    """([n, 3] global 0-based vertex indices, [n, 3] their coordinates) of the points"""
    pts = np.asarray(points, dtype=np.float64)
    ijk, xyz = np.zeros(pts.shape, dtype=np.int64), np.zeros(pts.shape)
    for d in range(3):
        c = global_vert_coords(mesh, d)
        ijk[:, d] = nearest_vertex(c, pts[:, d], bool(mesh.periodic_BC[d]), float(mesh.L[d]))
        xyz[:, d] = c[ijk[:, d]]
    return ijk, xyz


def column_names(n):
    return tuple("%s_%d" % (c, q) for q in range(n) for c in "uvw")


def header_comments(ijk, xyz):
    return ["# probe %d: vertex %d %d %d at %.17g %.17g %.17g\n" % ((q,) + tuple(int(i) + 1 for i in ijk[q]) + tuple(xyz[q]))
            for q in range(len(ijk))]


class Probes(Series):
    """Probes(solver, cfg, append=False), attached as `case.probes = Probes(case.solver, cfg, append=case.restarted)`:
    BaseCase.run then calls update(it) and poll() once per step, flush() before a checkpoint and finalise() at the end."""

    def __init__(self, solver, cfg, append=False):
        self.cfg = cfg
        b, m = solver.backend, solver.mesh
        self.n = int(cfg.points.shape[0])
        self.ijk, self.xyz = snap(m, cfg.points)
        off = np.array([int(o) for o in m.n_offset], dtype=np.int64)
        dims = np.array([int(n) for n in m.get_dims(VERT)], dtype=np.int64)
        local = self.ijk - off[None, :]
        self.owned = np.flatnonzero(np.all((local >= 0) & (local < dims[None, :]), axis=1))
        ijk_c = np.ascontiguousarray(local[self.owned], dtype=np.int32)
        slot_c = np.ascontiguousarray(self.owned, dtype=np.int32)
        self.lib, self.h = b.lib, ctypes.c_void_p()
        # the library accepts the probes BEFORE the series touches its file: a refused construction leaves no file behind
        # and truncates none
        _lib.check(b.lib.x3d_probe_create(b.h, ijk_c.ctypes.data_as(_lib.c_int_p), int(self.owned.size),
                                          slot_c.ctypes.data_as(_lib.c_int_p), self.n, ctypes.byref(self.h)))
        super().__init__(solver, "Probes", cfg.prefix, cfg.flush_every, 3 * self.n, column_names(self.n), append,
                         header_comments(self.ijk, self.xyz))

    def __del__(self):
        try:
            if self.h is not None:
                self.lib.x3d_probe_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def record(self, it, u, v, w):
        """one row for iteration `it` from fields of the caller's; no host wait unless both tables are in flight"""
        self.solver.backend.probe_sample(self.h, u, v, w, self.row_address(it))
        self.commit()

    def reads_state(self, it):
        """does update(it) read the solver's fields?  (BaseCase.run then completes the step first)"""
        return self.cfg.sample_due(it)

    def update(self, it):
        """one sample if iteration `it` is due; returns whether one was taken.  No host wait."""
        if not self.reads_state(it):
            return False
        s = self.solver
        s.flush_grad()  # a velocity correction left pending by step(more=True) is not in u, v, w yet
        self.record(it, s.u, s.v, s.w)
        return True
