"""ibm_t mirror (/root/reference/src/module/ibm.f90): the basic immersed-boundary method, vel = vel * ep1 before the
pressure solve, with ep1 = 1 in the fluid and 0 in the solid.

The reference keeps ep1 as a full device block and calls vecmult three times per sub-step (:164-166).  Here the
library keeps a work list of the 64-point x segments in which ep1 differs from 1 and the mask values of those
segments only (csrc/ibm.hip); `body` is one launch over that list and gives the same bits, because x * 1.0 = x.
X3D_NO_IBM_SPARSE=1 (read when an Ibm is made) keeps the reference's form -- a device mask block and three vecmult
calls -- as the A/B and test baseline.

The reference reads iibm and ep1 from `ibm_XYZ.bp`, an ADIOS2 file written by an outside tool; here the same two
variables travel in an .npz file (`Ibm.save` / `Ibm.from_file`)."""
import ctypes

import numpy as np

from . import _lib
from .common import DIR_X, VERT, X3dError
from .switches import Switches

IIBM_BASIC = 1  # iibm_basic, src/module/ibm.f90:25


def cylinder_mask(mesh, centre, radius, axis=2):
    """ep1 [nz, ny, nx] on this rank's vertex coordinates (stretched directions included): 0 strictly inside the
    circular cylinder of the given radius whose axis runs along direction `axis` (0 = x, 1 = y, 2 = z) through
    `centre`, 1 elsewhere.  centre: the two coordinates across the axis in x, y, z order (or all three; the one along
    the axis is ignored).  axis=None: a sphere about the three coordinates of `centre`.  radius 0: all ones."""
    x = np.asarray(mesh.vert_coords[0], dtype=np.float64)[None, None, :]
    y = np.asarray(mesh.vert_coords[1], dtype=np.float64)[None, :, None]
    z = np.asarray(mesh.vert_coords[2], dtype=np.float64)[:, None, None]
    coords = [x, y, z]
    centre = [float(c) for c in centre]
    if axis is None:
        if len(centre) != 3:
            raise X3dError("cylinder_mask: a sphere needs three centre coordinates")
        across = [0, 1, 2]
    else:
        if axis not in (0, 1, 2):
            raise X3dError("cylinder_mask: axis must be 0, 1, 2 or None")
        across = [d for d in range(3) if d != axis]
        if len(centre) == 2:
            centre = [centre[across.index(d)] if d != axis else 0.0 for d in range(3)]
        elif len(centre) != 3:
            raise X3dError("cylinder_mask: centre needs two or three coordinates")
    d2 = sum((coords[d] - centre[d]) ** 2 for d in across)
    nx, ny, nz = (int(n) for n in mesh.vert_dims)
    inside = np.broadcast_to(d2 < float(radius) ** 2, (nz, ny, nx))
    return np.where(inside, 0.0, 1.0)


class Ibm:
    """Ibm(solver, ep1, iibm=1): ep1 = numpy [nz, ny, nx] on this rank's vertices.  Rank-local: every rank masks its own
    points, nothing is exchanged.  Attach it with `solver.ibm = Ibm(...)`; BaseCase.substep then calls `body` between
    apply_BC and the pressure correction (base_case.f90:282-285).  iibm != 1: an object that does nothing, as in the
    reference (:138-141, 155)."""

    def __init__(self, solver, ep1, iibm=IIBM_BASIC):
        self.backend = solver.backend  # (the backend only: solver.ibm -> Ibm -> solver would be a reference cycle)
        self.iibm = int(iibm)
        self.h = None          # the library's work list (sparse form)
        self.ep1_field = None  # the reference's device mask block (X3D_NO_IBM_SPARSE=1)
        self.n_segments = self.n_masked = 0
        self.loads = None      # optional loads.Loads: `body` then takes the impulse it removes along on the steps that are due
        self.area_ref = None   # the reference area of the body's force coefficients, if whoever made the mask knows one
        b = self.backend
        nx, ny, nz = b.mesh.get_dims(VERT)
        self.ep1 = np.ascontiguousarray(ep1, dtype=np.float64)
        if self.ep1.shape != (nz, ny, nx):
            raise X3dError(f"Ibm: ep1 has shape {self.ep1.shape}, this rank's vertices are {(nz, ny, nx)}")
        self.sparse = not Switches.from_env().no_ibm_sparse
        if self.iibm != IIBM_BASIC:
            return
        a = np.ascontiguousarray(self.ep1, dtype=_lib.NP_REAL)
        h = ctypes.c_void_p()
        _lib.check(b.lib.x3d_ibm_create(b.h, a.ctypes.data_as(_lib.c_double_p), _lib.ints(nx, ny, nz), ctypes.byref(h)))
        out = (ctypes.c_long * 2)()
        _lib.check(b.lib.x3d_ibm_counts(h, out))
        self.n_segments, self.n_masked = int(out[0]), int(out[1])
        if self.sparse:
            self.h = h
        else:
            # the baseline: the library's list served for the two counts only; src/module/ibm.f90:126-132: a block of
            # ones with ep1 on the vertices
            _lib.check(b.lib.x3d_ibm_destroy(h))
            f = b.allocator.get_block(DIR_X, VERT)
            f.fill(1.0)
            b.set_field_data(f, self.ep1)
            self.ep1_field = f

    def __del__(self):
        try:
            if self.h is not None:
                self.backend.lib.x3d_ibm_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def body(self, u, v, w):
        """ibm_t%body, src/module/ibm.f90:148-170 (the FIXME about dt * grad p inside the solid stands here too)"""
        if self.iibm != IIBM_BASIC:
            return
        b = self.backend
        if self.h is not None:
            for f in (u, v, w):
                if f.dir != DIR_X:
                    raise X3dError("Ibm.body: DIR_X fields are needed")
            row = self.loads.begin_body() if self.loads is not None else None
            if row is None:
                _lib.check(b.lib.x3d_ibm_body(b.h, self.h, u.ptr, v.ptr, w.ptr, b._dims(VERT)))
            else:
                b.ibm_body_loads(self.h, u, v, w, row[0], row[1])
                self.loads.end_body()
        else:
            b.vecmult(u, self.ep1_field)
            b.vecmult(v, self.ep1_field)
            b.vecmult(w, self.ep1_field)

    # ---- file form: the reference's variable names (ibm.f90:104, 123), .npz instead of ADIOS2
    def save(self, path):
        save_mask(path, self.ep1, self.iibm)

    @classmethod
    def from_file(cls, solver, path):
        iibm, ep1 = load_mask(path)  # (this rank's vertices, like the constructor's ep1)
        return cls(solver, ep1, iibm)


def save_mask(path, ep1, iibm=IIBM_BASIC):
    """the two variables of the reference's ibm_XYZ.bp, `iibm` (integer) and `ep1` ([nz, ny, nx], C order), as an .npz"""
    np.savez(path, iibm=np.int64(iibm), ep1=np.ascontiguousarray(ep1, dtype=np.float64))


def load_mask(path):
    """(iibm, ep1) of an .npz written by save_mask"""
    with np.load(path) as z:
        if "iibm" not in z.files or "ep1" not in z.files:
            raise X3dError(f"{path} does not hold the variables iibm and ep1")
        return int(z["iibm"]), np.array(z["ep1"], dtype=np.float64)
