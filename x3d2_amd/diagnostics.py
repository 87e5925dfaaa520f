"""Diagnostics series: kinetic energy, enstrophy, dissipation, maxima, CFL, max / mean |div u| and the wall shear stress
of every sampled step, reduced on the device (csrc/diagnostics.hip) and written as a scalar series.

The reference's monitoring (src/postprocess/monitoring.f90; case.Monitoring here) takes a curl with its reorders, three
scalar products and a max / mean per row, each ending in a host wait.  A sample here is: the nine velocity gradients on the
x-fastest blocks (HipBackend.tds_apply, as Snapshots.write takes them), ONE reduction over u, v, w and the gradients that
leaves the row's sixteen doubles in a device table (HipBackend.diag_reduce), and, with divergence=True, divergence_v2p and
the max / sum of its block (HipBackend.diag_max_sum).  No call of a sample waits for the host.  A sample holds nine
transient pool blocks (about 9.3 GiB at 512^3 in FP64); their release is stream-ordered.

Tables.  Row r of the current batch goes to table[r] of a device table of flush_every x 16 doubles.  A full table -- and
flush() / finalise() -- starts one asynchronous copy into its pinned twin; poll(), once per step, turns the tables that
have landed into rows and lines of the file.  The tables are a ring of 2 slots (copyring.CopyRing): the 3rd acquire waits,
that is, a table that is needed again before it has been landed waits for its copy and counts sync_count.  Several ranks: every rank's table holds its local sums and maxima; a landed
table is combined in two collectives (sum over slots 0-7, max over slots 8-13).  So that the collectives match, every rank
flushes at the same sample counts and a table is landed by the second poll() after its flush (waiting for the copy if it
has to), not whenever its own copy happens to be done.

Columns, with N the global vertex count, nu = 1 / Re and S the raw slots (include/x3d2_hip.h):
    ke = 1/2 (S0 + S1 + S2) / N     enstrophy = 1/2 S3 / N (the reference's definition)     dissipation = 2 nu S4 / N
    u_max, v_max, w_max = S8, S9, S10     vort_max = sqrt(S11)     cfl = dt S12
    div_u_max = S13, div_u_mean = S7 / N_cell                (divergence=True)
    tau_w_lo = nu S5 / (nx nz), tau_w_hi = -nu S6 / (nx nz)   (y not periodic)

Spacing tables of the CFL number: 1 / mesh.d of a uniform direction; for a stretched one the centred difference
1/2 (y[j+1] - y[j-1]) of the GLOBAL vertex coordinates, one-sided at the first and last vertex of a non-periodic
direction; built once, on the host; every rank takes its slice.

File: `<prefix>.csv`, root rank only, in scalar_series_t's format (src/postprocess/scalar_series.f90): the header
`# time, <col>, <col>, ...`, then one line per row, every value as ES20.12 (Python's '%20.12E'), comma-separated, flushed
per batch.  A three-digit exponent is written Python's way (1.0E-100), not Fortran's (1.0-100).  append=True keeps an
existing file and drops its rows later than solver.current_iter * dt (a restarted run)."""
import math
import os

import numpy as np
import torch

from .common import DIR_Z, CELL, VERT, BC_NAMES, X3dError, sample_due
from .copyring import CopyRing

NSLOT = 16
SUM_SLOTS, MAX_SLOTS = slice(0, 8), slice(8, 14)
MAX_FLUSH_EVERY = 4096  # rows per device table: 512 KiB


class DiagnosticsConfig:
    """when to sample (as StatsConfig: from iteration initdiag on, every idiagfreq iterations; initdiag <= 0: never),
    where to write, how many rows a device table holds, and whether max / mean |div u| are part of a row"""

    def __init__(self, initdiag=1, idiagfreq=1, prefix="diagnostics", flush_every=256, divergence=True):
        self.initdiag, self.idiagfreq = int(initdiag), int(idiagfreq)
        if self.idiagfreq < 1:
            raise X3dError("DiagnosticsConfig: idiagfreq must be at least 1")
        self.prefix = str(prefix)
        self.flush_every = int(flush_every)
        if self.flush_every < 1:
            raise X3dError("DiagnosticsConfig: flush_every must be at least 1")
        self.divergence = bool(divergence)

    @property
    def active(self):
        return self.initdiag > 0

    def sample_due(self, it):
        return sample_due(it, self.initdiag, self.idiagfreq)


# ---------------------------------------------------------------- host side: columns, spacings, file
def column_names(divergence=True, y_walls=False):
    names = ["ke", "enstrophy", "dissipation", "u_max", "v_max", "w_max", "vort_max", "cfl"]
    if divergence:
        names += ["div_u_max", "div_u_mean"]
    if y_walls:
        names += ["tau_w_lo", "tau_w_hi"]
    return tuple(names)


def derive(raw, n_vert, n_cell, n_plane, nu, dt, divergence=True, y_walls=False):
    """the columns of one row from its sixteen raw slots (summed / maximised over the ranks), in column_names' order"""
    S = [float(v) for v in raw]
    out = [0.5 * (S[0] + S[1] + S[2]) / n_vert, 0.5 * S[3] / n_vert, 2.0 * nu * S[4] / n_vert, S[8], S[9], S[10],
           math.sqrt(S[11]), dt * S[12]]
    if divergence:
        out += [S[13], S[7] / n_cell]
    if y_walls:
        out += [nu * S[5] / n_plane, -nu * S[6] / n_plane]
    return out


def inverse_spacing(coords, periodic, length):
    """1 / h of every vertex of one direction from its GLOBAL coordinates: h[j] = 1/2 (y[j+1] - y[j-1]), wrapped around a
    periodic direction of the given length, one-sided at the two ends of any other"""
    y = np.asarray(coords, dtype=np.float64)
    h = np.empty_like(y)
    h[1:-1] = 0.5 * (y[2:] - y[:-2])
    if periodic:
        h[0] = 0.5 * (y[1] - (y[-1] - float(length)))
        h[-1] = 0.5 * ((y[0] + float(length)) - y[-2])
    else:
        h[0], h[-1] = y[1] - y[0], y[-1] - y[-2]
    return 1.0 / h


def global_vert_coords(mesh, d):
    """the vertex coordinates of direction d over ALL ranks"""
    if int(mesh.nproc_dir[d]) == 1:
        return np.asarray(mesh.vert_coords[d], dtype=np.float64)
    from .mesh import Mesh
    names = {v: k for k, v in BC_NAMES.items()}
    bcs = [tuple(names[int(c)] for c in mesh.BCs_global[k]) for k in range(3)]
    whole = Mesh(tuple(int(n) for n in mesh.global_vert_dims), (1, 1, 1), tuple(mesh.L), bcs[0], bcs[1], bcs[2],
                 tuple(mesh.stretching), tuple(mesh.beta))
    return np.asarray(whole.vert_coords[d], dtype=np.float64)


def spacing_tables(mesh):
    """this rank's three tables of inverse spacings (float64, one value per local vertex)"""
    out = []
    for d in range(3):
        n, off = int(mesh.vert_dims[d]), int(mesh.n_offset[d])
        if not mesh.stretched[d]:
            out.append(np.full(n, 1.0 / float(mesh.d[d])))
        else:
            ih = inverse_spacing(global_vert_coords(mesh, d), bool(mesh.periodic_BC[d]), float(mesh.L[d]))
            out.append(np.ascontiguousarray(ih[off:off + n]))
    return out


def format_header(columns):
    return "# time" + "".join(", " + c for c in columns) + "\n"


def format_row(t, values):
    """scalar_series_t%write_step: ES20.12 per value, comma-separated (a three-digit exponent Python's way)"""
    return ",".join("%20.12E" % float(v) for v in [t] + list(values)) + "\n"


def parse_csv(path):
    """(columns, array [nrows, 1 + ncolumns]) of a series file; comment lines other than the header are skipped"""
    columns, rows = None, []
    with open(path) as fh:
        for line in fh:
            if line.startswith("#"):
                if line.startswith("# time"):
                    columns = tuple(c.strip() for c in line[1:].split(",")[1:])
                continue
            if line.strip():
                rows.append([float(v) for v in line.split(",")])
    if columns is None:
        raise X3dError("%s has no `# time, ...` header" % path)
    return columns, np.array(rows, dtype=np.float64).reshape(len(rows), 1 + len(columns))


def trim_csv(path, t_last, columns):
    """keep the header and the rows with time <= t_last (an existing series a restarted run appends to); the header must
    name `columns`.  Returns the number of rows kept."""
    with open(path) as fh:
        lines = fh.readlines()
    if format_header(columns) not in lines:
        raise X3dError("%s: the series was written with other columns than %s" % (path, ", ".join(columns)))
    keep, n = [], 0
    for line in lines:
        if line.startswith("#") or not line.strip():
            keep.append(line)
        elif float(line.split(",")[0]) <= t_last * (1.0 + 1e-12):
            keep.append(line)
            n += 1
    with open(path, "w") as fh:
        fh.writelines(keep)
    return n


# ---------------------------------------------------------------- a series: tables, ring, file
class Series:
    """the table -> pinned copy -> file path of a series (module docstring, "Tables" and "File") for rows of `width` doubles
    that kernels of the owner's write into the device table: row_address(it) is where the next row goes, commit() closes
    it.  combine(raw) joins a landed table over the ranks (here: ONE sum over all slots); values(raw) -> the columns of a
    row; comments: lines behind the header.  Diagnostics below, loads.Loads and probes.Probes are such series."""

    def __init__(self, solver, who, prefix, flush_every, width, columns, append, comments=()):
        self.solver, self.width, self.columns = solver, int(width), tuple(columns)
        b, m = solver.backend, solver.mesh
        if flush_every > MAX_FLUSH_EVERY:
            raise X3dError("%s: flush_every = %d, a device table holds at most %d rows" % (who, flush_every, MAX_FLUSH_EVERY))
        self.flush_every = int(flush_every)
        self.sample_count = 0
        self.ring = CopyRing(b, 2, self._land)  # (an attached but idle series takes nothing)
        self._slot = None     # the ring slot of the current table, acquired by the first row of a batch
        self._meta = np.zeros((self.flush_every, 2), dtype=np.float64)  # (iteration, time) of the current table's rows
        self._count = 0
        self._rows = []  # (iteration, time, the combined raw row)
        self.file = prefix + ".csv" if m.is_root() else None
        if self.file is not None:
            if append and os.path.exists(self.file):
                trim_csv(self.file, int(solver.current_iter) * float(solver.dt), self.columns)
            else:
                with open(self.file, "w") as fh:
                    fh.write(format_header(self.columns))
                    fh.writelines(comments)

    @property
    def sync_count(self):
        """how often a row had to wait for a table whose copy had not been landed"""
        return self.ring.waits

    def row_address(self, it):
        """the device address of the row of iteration `it` in the current table (a third table before the first has
        landed waits here)"""
        if self._slot is None:  # (asked once per kernel that writes the row: the first call of a table acquires it)
            self._slot = self.ring.acquire(self.flush_every * self.width * 8)
        self._meta[self._count] = (int(it), int(it) * float(self.solver.dt))
        return self._slot.dev.data_ptr() + self._count * self.width * 8

    def commit(self):
        self._count += 1
        self.sample_count += 1
        if self._count == self.flush_every:
            self.flush()

    def flush(self):
        """start the copy of the current table's rows (if it has any) and go on with the other table; no host wait"""
        if self._count == 0:
            return False
        n = self._count
        self.ring.submit(self._slot, n * self.width * 8, [n, self._meta[:n].copy(), 0])  # (rows, meta, polls seen)
        self._slot, self._count = None, 0
        return True

    def _land(self, payload, raw):
        b = self.solver.backend
        n, meta, _ = payload
        raw = raw.view(np.float64).reshape(n, self.width).copy()
        if b.comm.size > 1:
            self.combine(raw)
        lines = []
        for r in range(n):
            self._rows.append((int(meta[r, 0]), float(meta[r, 1]), raw[r]))
            lines.append(format_row(meta[r, 1], self.values(raw[r])))
        if self.file is not None:
            with open(self.file, "a") as fh:
                fh.writelines(lines)
        return n

    def combine(self, raw):
        """a landed table [rows, width] of this rank -> that of all ranks, in place; every rank calls it for the same table"""
        sums = torch.from_numpy(raw)  # (shares raw's memory)
        self.solver.backend.comm.allreduce_tensor(sums, "sum")

    def poll(self):
        """turn the tables whose copies have landed into rows, oldest first; returns the rows added.  One rank: never
        blocks.  Several ranks: a table is landed by the second poll after its flush, so that the collectives match."""
        if self.solver.backend.comm.size == 1:
            return sum(self.ring.poll())
        n = 0
        for slot, p in self.ring.pending():
            p[2] += 1
            if p[2] < 2:
                break
            n += self.ring.land(slot)
        return n

    def finalise(self):
        """flush, then wait for and write what is left"""
        self.flush()
        return sum(self.ring.drain())

    def values(self, raw):
        return list(raw)

    def raw_rows(self):
        """[nrows, width]: the raw slots of the rows landed so far (summed over the ranks)"""
        return np.array([r[2] for r in self._rows], dtype=np.float64).reshape(len(self._rows), self.width)

    def rows(self):
        """the rows landed so far as a structured array: iteration, time and the columns"""
        dt = [("iteration", np.int64), ("time", np.float64)] + [(c, np.float64) for c in self.columns]
        out = np.zeros(len(self._rows), dtype=dt)
        for i, (it, t, raw) in enumerate(self._rows):
            out[i] = (it, t) + tuple(self.values(raw))
        return out


# ---------------------------------------------------------------- the device object
class Diagnostics(Series):
    """Diagnostics(solver, cfg, append=False), attached as `case.diagnostics = Diagnostics(case.solver, cfg)`:
    BaseCase.run then calls update(it) and poll() once per step, flush() before a checkpoint and finalise() at the end.
    A restarted run constructs it with append=case.restarted."""

    def __init__(self, solver, cfg, append=False):
        self.cfg = cfg
        b, m = solver.backend, solver.mesh
        self.y_walls = not bool(m.periodic_BC[1])
        super().__init__(solver, "Diagnostics", cfg.prefix, cfg.flush_every, NSLOT, column_names(cfg.divergence, self.y_walls),
                         append)
        gv, gc = m.get_global_dims(VERT), m.get_global_dims(CELL)
        self.n_vert, self.n_cell = float(np.prod(gv)), float(np.prod(gc))
        self.n_plane = float(int(gv[0]) * int(gv[2]))
        self.first_y = self.y_walls and int(m.nrank_dir[1]) == 0
        self.last_y = self.y_walls and int(m.nrank_dir[1]) == int(m.nproc_dir[1]) - 1
        self.ih_host = spacing_tables(m)
        self.ih = [torch.from_numpy(a).to(b.device) for a in self.ih_host]
        self._scratch = None

    # ------------------------------------------------------------ taking a sample
    def reduce(self, u, v, w, grads, out=None):
        """the raw row of u, v, w and nine gradient fields of the caller's (compute_vorticity's order) -> `out`, a device
        float64 tensor of 16 values (default: a scratch row of this object), which is returned; slots 7 and 13 keep what
        they hold.  No host wait."""
        b = self.solver.backend
        if out is None:
            if self._scratch is None:
                self._scratch = torch.zeros(NSLOT, dtype=torch.float64, device=b.device)
            out = self._scratch
        if out.dtype != torch.float64 or not out.is_cuda or out.numel() < NSLOT:
            raise X3dError("Diagnostics.reduce: out is a device float64 tensor of 16 values")
        b.diag_reduce(u, v, w, grads, self.ih, self.first_y, self.last_y, out.data_ptr())
        return out

    def record(self, it, u, v, w, grads, div_u=None):
        """one row for iteration `it` into the current device table from fields of the caller's: the reduction over u, v,
        w and the nine gradients and, if div_u is given, the max / sum of that block; no host wait unless both tables
        are in flight"""
        self.row_address(it)  # (a third table before the first has landed waits here)
        row = self._slot.dev.view(torch.float64)[self._count * NSLOT:(self._count + 1) * NSLOT]
        self.reduce(u, v, w, grads, out=row)
        if div_u is not None:
            self.solver.backend.diag_max_sum(div_u, row.data_ptr())
        self.commit()

    def sample(self, it):
        """one row for iteration `it` from the solver's velocity: nine gradients, the reduction, the divergence"""
        s = self.solver
        al = s.backend.allocator
        s.flush_grad()  # a velocity correction left pending by step(more=True) is not in u, v, w yet
        taken = s.velocity_gradients()
        div_u = None
        if self.cfg.divergence:
            div_u = al.get_block(DIR_Z)
            s.divergence_v2p(div_u, s.u, s.v, s.w)
        self.record(it, s.u, s.v, s.w, taken[:9], div_u)
        if div_u is not None:
            taken.append(div_u)
        for g in taken:  # (stream-ordered: whoever takes them next writes behind the reductions)
            al.release_block(g)

    def reads_state(self, it):
        """does update(it) read the solver's fields?  (BaseCase.run then completes the step first)"""
        return self.cfg.sample_due(it)

    def update(self, it):
        """one sample if iteration `it` is due; returns whether one was taken.  No host wait."""
        if not self.reads_state(it):
            return False
        self.sample(it)
        return True

    # ------------------------------------------------------------ several ranks, columns
    def combine(self, raw):
        """two collectives: the sum over slots 0-7, the maximum over slots 8-13"""
        comm = self.solver.backend.comm
        sums, maxs = torch.from_numpy(raw[:, SUM_SLOTS].copy()), torch.from_numpy(raw[:, MAX_SLOTS].copy())
        comm.allreduce_tensor(sums, "sum")
        comm.allreduce_tensor(maxs, "max")
        raw[:, SUM_SLOTS], raw[:, MAX_SLOTS] = sums.numpy(), maxs.numpy()

    def values(self, raw):
        s = self.solver
        return derive(raw, self.n_vert, self.n_cell, self.n_plane, float(s.nu), float(s.dt), self.cfg.divergence, self.y_walls)
