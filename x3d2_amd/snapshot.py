"""Snapshots: mirror of snapshot_manager_t (src/io/snapshot_manager.f90, src/io/io_field_utils.f90) with the striding,
the conversion and the derived fields on the device.

The reference copies every output field to the host whole, strides it there, and fills two full blocks for vort and
qcrit (src/postprocess/postprocess.f90).  Here `write` computes the nine velocity gradients (only if vort or qcrit is
asked for) and the vertex pressure with the operators of compute_derived_fields / compute_pressure_vert on the one
Cartesian layout, then launches ONE kernel that decimates, converts and packs every variable into a dense device buffer
(HipBackend.snapshot_pack, csrc/snapshot.hip; |omega| and Q at the kept points only) and ONE asynchronous copy of that
buffer into pinned host memory on a second stream.  `write` returns without a host wait; `poll` writes the files of the
copies that have landed, `finalise` waits for the rest.  The buffers are a ring of 2 slots (copyring.CopyRing): the 3rd
acquire waits, that is, a third snapshot that arrives before the first has been written waits for it.

Which points are kept.  The reference strides each rank's block from the rank's own first point
(io_field_utils.f90:122, 175-188).  Here a point is kept where its GLOBAL index (0-based) is a multiple of the stride:
the first kept local index of a rank is (-n_offset) mod stride.  The two rules agree whenever every rank's offset is a
multiple of the stride, and only the global rule gives a uniform output grid (and output counts that add up to the
global output shape) when it is not.

Pressure.  `pressure` in output_fields sets Solver.keep_pressure (src/solver.f90:705-726).  The op-granular driver then
keeps the last sub-step's pressure as the reference does.  The fused driver has no pressure field on its z-first 000 and
row-interleaved 010 paths; BaseCase.run tells the solver before a step whose snapshot is due, and the last sub-step's
correction of that step takes the plain z pair -> solve -> z pair branch and copies p out.  A run with pressure snapshots
is therefore not bit-identical, on those steps, to one without.

Output: the reference writes ADIOS2 (.bp); ADIOS2 is not a dependency of this project, so a snapshot is
`<prefix>_<it:06d>.npz` (several ranks: `<prefix>_<it:06d>.r<rank>.npz`, assembled by load_snapshot) with the variables
under the reference's names, shaped [nz_out, ny_out, nx_out], plus time, iteration, stride, shape / start / count
(x, y, z order), origin, spacing and the `vtk.xml` ImageData string of generate_vtk_xml."""
import glob
import os

import numpy as np

from . import _lib
from .common import DIR_X, VERT, X3dError
from .copyring import CopyRing

# output_fields of checkpoint_params (src/config.f90), in the order get_snapshot_fields tests them
OUTPUT_FIELDS = ("pressure", "vorticity", "qcriterion", "ibm", "species")


class SnapshotConfig:
    """the snapshot part of checkpoint_params (src/config.f90): snapshot_freq, snapshot_prefix, output_stride,
    snapshot_sp (4-byte output), output_fields"""

    def __init__(self, snapshot_freq=0, snapshot_prefix="snapshot", output_stride=(1, 1, 1), snapshot_sp=False,
                 output_fields=()):
        self.snapshot_freq = int(snapshot_freq)
        self.snapshot_prefix = str(snapshot_prefix)
        self.output_stride = tuple(int(s) for s in output_stride)
        if len(self.output_stride) != 3 or any(s < 1 for s in self.output_stride):
            raise X3dError("SnapshotConfig: output_stride is three integers >= 1")
        self.snapshot_sp = bool(snapshot_sp)
        if isinstance(output_fields, str):
            output_fields = (output_fields,)
        self.output_fields = tuple(str(f) for f in output_fields)
        for f in self.output_fields:
            if f not in OUTPUT_FIELDS:
                raise X3dError(f"SnapshotConfig: unknown output field {f!r} (one of {', '.join(OUTPUT_FIELDS)})")

    def has(self, name):
        return name in self.output_fields

    def due(self, it):
        """src/io/snapshot_manager.f90:125-126"""
        if self.snapshot_freq <= 0:
            return False
        return it % self.snapshot_freq == 0


def snapshot_fields(cfg, nspecies):
    """get_snapshot_fields, src/io/snapshot_manager.f90:198-243"""
    names = ["u", "v", "w"]
    if cfg.has("pressure"):
        names.append("p")
    if cfg.has("vorticity"):
        names.append("vort")
    if cfg.has("qcriterion"):
        names.append("qcrit")
    if cfg.has("ibm"):
        names.append("ibm")
    if cfg.has("species"):
        names += ["phi_%d" % i for i in range(1, int(nspecies) + 1)]
    return names


def output_geometry(global_dims, offset, local_dims, stride):
    """get_output_dimensions (src/io/io_field_utils.f90:126-189) under the global rule of the module docstring.
    Returns (shape, start, count, first), each (x, y, z): the global output shape, this rank's first output index and
    number of output points, and its first kept local index."""
    shape, start, count, first = [], [], [], []
    for n_glob, off, n, s in zip(global_dims, offset, local_dims, stride):
        n_glob, off, n, s = int(n_glob), int(off), int(n), int(s)
        f = (-off) % s
        shape.append((n_glob + s - 1) // s)
        first.append(f)
        start.append((off + f) // s)
        count.append((n - f + s - 1) // s if f < n else 0)
    return tuple(shape), tuple(start), tuple(count), tuple(first)


def _g0(x):
    """a real(dp) as the G0 edit descriptor renders it: 17 significant digits, fixed notation for 0.1 <= |x| < 1e17 (and
    for zero), else a mantissa in [0.1, 1) with an exponent"""
    x = float(x)
    if x == 0.0:
        return "0.0000000000000000"
    e = int(np.floor(np.log10(abs(x)))) + 1  # digits before the point
    if 0 <= e <= 17:
        return "%.*f" % (17 - max(e, 1) if e > 0 else 17, x)
    return "%.17fE%+03d" % (x / 10.0 ** e, e)


def generate_vtk_xml(dims, fields, origin, spacing):
    """generate_vtk_xml, src/io/snapshot_manager.f90:245-285; dims = output shape in (x, y, z) order"""
    extent = "0 %d 0 %d 0 %d" % (dims[2] - 1, dims[1] - 1, dims[0] - 1)  # (:257-258: the extents are written z, y, x)
    xml = ('<?xml version="1.0"?>\n<VTKFile type="ImageData" version="0.1">\n'
           '  <ImageData WholeExtent=" %s" Origin="%s" Spacing="%s">\n    <Piece Extent="%s">\n      <PointData>\n'
           % (extent, " ".join(_g0(v) for v in origin), " ".join(_g0(v) for v in spacing), extent))
    for f in fields:
        xml += '      <DataArray Name="%s">%s</DataArray>\n' % (f, f)
    xml += '        <DataArray Name="TIME">time</DataArray>\n'
    xml += "      </PointData>\n    </Piece>\n  </ImageData>\n</VTKFile>"
    return xml


class Snapshots:
    """Snapshots(solver, cfg), attached as `case.snapshots = Snapshots(case.solver, cfg)`: BaseCase.run then calls
    write(it) and poll() once per step and finalise() before it returns."""

    def __init__(self, solver, cfg):
        self.solver, self.cfg = solver, cfg
        m = solver.mesh
        nspecies = len(getattr(solver, "species", ()))
        if cfg.has("species") and nspecies <= 0:
            # (the reference stops here too, snapshot_manager.f90:130-138)
            raise X3dError("species snapshot output requested, but no transported species are configured")
        if cfg.has("ibm") and getattr(solver, "ibm", None) is None:
            # (the reference would write an unassociated field)
            raise X3dError("ibm snapshot output requested, but the solver has no immersed boundary (solver.ibm)")
        self.names = snapshot_fields(cfg, nspecies)
        if len(self.names) > 16:
            raise X3dError("Snapshots: at most 16 variables per snapshot")
        self.shape, self.start, self.count, self.first = output_geometry(
            m.get_global_dims(VERT), m.n_offset, m.get_dims(VERT), cfg.output_stride)
        if min(self.count) < 1:
            raise X3dError("Snapshots: this rank keeps no point with output_stride %s" % (cfg.output_stride,))
        self.dtype = np.dtype("float32") if cfg.snapshot_sp else np.dtype(_lib.NP_REAL)
        self.nbytes = len(self.names) * int(np.prod(self.count)) * self.dtype.itemsize
        # origin: the first global vertex (exact on uniform directions and on the first rank of a stretched one)
        self.origin = tuple(float(m.vert_coords[d][0]) - int(m.n_offset[d]) * float(m.d[d]) for d in range(3))
        self.spacing = tuple(float(m.d[d]) * cfg.output_stride[d] for d in range(3))
        self.vtk_xml = generate_vtk_xml(self.shape, self.names, self.origin, self.spacing)
        # (an attached but idle Snapshots takes nothing; the geometry above needs no backend at all)
        self.ring = CopyRing(getattr(solver, "backend", None), 2, self._write_file)
        self._ep1 = None    # device copy of the immersed boundary's mask, made when "ibm" is first written
        self.files = []     # names of the files written so far
        if cfg.has("pressure"):
            solver.keep_pressure = True  # base_case.f90:119-121

    # ------------------------------------------------------------ taking a snapshot
    def reads_state(self, it):
        """does write(it) read the solver's fields?  (BaseCase.run then completes the step first)"""
        return self.cfg.due(it)

    def write(self, it):
        """if iteration `it` is due: gradients / vertex pressure, one pack launch, one asynchronous copy; returns
        whether a snapshot was taken.  No host wait unless both buffers still hold unwritten snapshots."""
        if not self.reads_state(it):
            return False
        s = self.solver
        b, al = s.backend, s.backend.allocator
        s.flush_grad()  # a velocity correction left pending by step(more=True) is not in u, v, w yet
        slot = self.ring.acquire(self.nbytes)  # (the third snapshot before the first was written waits here)
        grads = None
        if self.cfg.has("vorticity") or self.cfg.has("qcriterion"):
            grads = s.velocity_gradients()
        taken = list(grads or ())
        variables = []
        for name in self.names:
            if name in ("u", "v", "w"):
                variables.append(("copy", getattr(s, name), 1.0))
            elif name == "p":
                taken += [al.get_block(DIR_X, VERT), al.get_block(DIR_X, VERT)]
                variables.append(("copy", self._pressure_vert(*taken[-2:]), 1.0 / s.dt))
            elif name in ("vort", "qcrit"):
                variables.append((name, grads))
            elif name == "ibm":
                variables.append(("copy", self._ep1_block(), 1.0))
            else:
                variables.append(("copy", s.species[int(name[4:]) - 1], 1.0))
        n = b.snapshot_pack(variables, self.first, self.cfg.output_stride, self.count, slot.dev, self.dtype)
        self.ring.submit(slot, n, int(it))
        for f in taken:  # (stream-ordered: whoever takes them next writes behind the pack)
            al.release_block(f)
        return True

    def _pressure_vert(self, t1, t2):
        """compute_pressure_vert without the scale, which the pack applies (Solver.pressure_vert)"""
        return self.solver.pressure_vert(t1, t2)

    def _ep1_block(self):
        if self._ep1 is None:
            ibm, b = self.solver.ibm, self.solver.backend
            if ibm.ep1_field is not None:  # (the baseline form of Ibm keeps the mask on the device already)
                self._ep1 = ibm.ep1_field
            else:
                f = b.allocator.get_block(DIR_X, VERT)
                f.fill(1.0)
                b.set_field_data(f, ibm.ep1)
                self._ep1 = f
        return self._ep1

    # ------------------------------------------------------------ writing
    def _file_name(self, it):
        m = self.solver.mesh
        return "%s_%06d%s.npz" % (self.cfg.snapshot_prefix, it, "" if m.nproc == 1 else ".r%d" % m.nrank)

    def _write_file(self, it, raw):
        """the ring's landing: the file of iteration `it` from the packed bytes"""
        cx, cy, cz = self.count
        a = raw.view(self.dtype).reshape(len(self.names), cz, cy, cx)
        out = {name: a[k] for k, name in enumerate(self.names)}
        out.update({"time": np.float64(it * self.solver.dt), "iteration": np.int64(it),
                    "stride": np.array(self.cfg.output_stride, dtype=np.int64),
                    "shape": np.array(self.shape, dtype=np.int64), "start": np.array(self.start, dtype=np.int64),
                    "count": np.array(self.count, dtype=np.int64), "origin": np.array(self.origin),
                    "spacing": np.array(self.spacing), "vtk.xml": np.array(self.vtk_xml)})
        name = self._file_name(it)
        np.savez(name, **out)
        self.files.append(name)
        return name

    def poll(self):
        """write every snapshot whose copy has landed (oldest first); never blocks.  Returns the files written."""
        return self.ring.poll()

    def finalise(self):
        """wait for and write what is left"""
        return self.ring.drain()


def load_snapshot(prefix, it):
    """one dict for iteration `it`: the single file of a one-rank run as it is, or the pieces `<prefix>_<it:06d>.r*.npz`
    of a decomposed run assembled into arrays of the global output shape (start and count then describe the whole)"""
    base = "%s_%06d" % (prefix, it)
    if os.path.exists(base + ".npz"):
        with np.load(base + ".npz") as z:
            return {k: z[k] for k in z.files}
    parts = sorted(glob.glob(glob.escape(base) + ".r*.npz"))
    if not parts:
        raise X3dError(f"load_snapshot: neither {base}.npz nor {base}.r<rank>.npz exists")
    meta = ("time", "iteration", "stride", "shape", "start", "count", "origin", "spacing", "vtk.xml")
    out, filled = {}, None
    for p in parts:
        with np.load(p) as z:
            sx, sy, sz = (int(v) for v in z["start"])
            cx, cy, cz = (int(v) for v in z["count"])
            if not out:
                nx, ny, nz = (int(v) for v in z["shape"])
                for k in z.files:
                    out[k] = z[k] if k in meta else np.empty((nz, ny, nx), dtype=z[k].dtype)
                filled = np.zeros((nz, ny, nx), dtype=np.int64)
            for k in z.files:
                if k not in meta:
                    out[k][sz:sz + cz, sy:sy + cy, sx:sx + cx] = z[k]
            filled[sz:sz + cz, sy:sy + cy, sx:sx + cx] += 1
    if not np.all(filled == 1):
        raise X3dError(f"load_snapshot: the pieces of {base} do not tile the output exactly once")
    out["start"] = np.zeros(3, dtype=np.int64)
    out["count"] = np.array(out["shape"], dtype=np.int64)
    return out
