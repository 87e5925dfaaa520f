"""Particles: Lagrangian tracers and inertial points, interpolated and advanced on the device (csrc/particles.hip).

Not in the reference: this project's own addition.  A particle follows dx/dt = v with v = u(x) (tau_p = 0: a tracer) or
dv/dt = (u(x) - v) / tau_p + g (an inertial point).  u(x) is a piecewise Lagrange interpolation of the vertex fields, per
direction on the ACTUAL vertex coordinates (a stretched y needs nothing special):

  wrap     periodic direction: x <- x - L floor(x / L); a result equal to L becomes 0
  cell     i = the largest index with c[i] <= x; the last cell of a periodic direction runs to L, elsewhere i <= n - 2
  nodes    order 2: i, i + 1.  order 4: s .. s + 3 with s = i - 1, clamped to [0, n - 4] in a non-periodic direction (one-sided
           next to a wall), taken mod n in a periodic one, node m sitting at c[m mod n] + L floor(m / n)
  weights  w_a = prod_{b != a} (x - xi_b) / (xi_a - xi_b)
  value    sum_k w_k sum_j w_j sum_i w_i f[k][j][i]

Time: second-order Adams-Bashforth on values stored with the particle (no old field is kept).  Construction primes the state
from the fields as they are (a = u(x), v, F); update(it), called by BaseCase.run after step `it`, is ONE launch:

  x += dt (c1 v + c0 v_prev)   [inertial: v += dt (c1 F + c0 F_prev)]     (c1, c0) = (1, 0) on the first advance, (1.5, -0.5) later
  periodic directions wrap; a non-periodic one mirrors once about the wall it crossed ("reflect": an inertial v_d changes sign;
  a particle still outside is clamped) or clamps and freezes the particle for good ("absorb": alive = 0)
  a = u^it(x), tracers v = a, inertial F = (a - v) / tau_p + g; the history rotates

so that x, v and a all belong to t_it afterwards.  A position that stops being finite freezes its particle (status 2) before
any index is formed.  Particle state is FP64 in both flavours of the library.

reads_state(it) is true at EVERY step from initpart - 1 on: a run with particles forgoes BaseCase.run's more=True deferral, as
iprobefreq = 1 does.  Before initpart the particles rest; the state is primed again after step initpart - 1, which is why that
step is completed like the ones that follow.

sort_every = m > 0: after the updates with it % m == 0 the state is ordered by cell (a stable radix sort of the linear cell
index and one gather of every array into a second set), so that neighbouring lanes gather from neighbouring cells.  Particles
do not interact: a run's state by id has the same bits with any sort_every.

Output: every ipartout steps one pack launch and one asynchronous copy through copyring.CopyRing (2 slots); poll() writes
`<prefix>_<it:06d>.npz` (id, x[n, 3], v, a, alive, status, iteration, time, in id order) once the copy has landed; write never
waits for the host.  state() is the same content now, with one host wait.

Several ranks (y and / or z cut; x never is).  A rank holds the particles it OWNS: rank r of a cut direction owns
c[r nl] <= x < c[(r + 1) nl] on the global vertex table, the last rank up to L (periodic) or up to and including the last
vertex (owner_index below; csrc/particles.hip holds the same comparisons on the same doubles); absorbed particles are owned by
position like any other, a particle whose position stopped being finite stays where it died.  cfg.x0 / v0 are the same global
arrays on every rank, each keeps its rows, id is the global row.  An advance is then

  move      one launch: the position (velocity) update, finiteness test, wrap, wall rule, v_prev <- v [v <- v_new, F_prev <- F]
  migrate   per cut direction, y then z: classification and a deterministic compaction on the device (stayers to the front in
            their order, leavers as whole rows into two messages of mig_capacity slots with their count in a header word),
            Comm.sendrecv with pprev / pnext, one launch that appends the arrivals: from pprev, then from pnext
  ghosts    per cut direction, y then z (z on rows that include the y ghosts): the face planes of u, v, w the stencil reaches
            (order 4: one below, two above; order 2: one above, and one below that keeps every message non-empty), never
            the interior
  sample    one launch: a = u(x) through rows of the block or of a ghost frame; v or F from it

with no host wait of its own (a host-staged transport waits in sendrecv).  The state has `capacity` slots
(default ceil(1.5 n / nproc) + 1024) and a message `mig_capacity` (default max(1024, capacity // 8)): this project's choice.
More leavers than mig_capacity, more residents than capacity, or a particle owned neither here nor by a ring neighbour set a
sticky device flag and keep the particle where it is; state(), raw_state(), state_dict(), check() and the file writer raise an
X3dError that names the cause and the rank.  state() is collective and returns the global state on every rank; files are
`<prefix>_<it:06d>.r<rank>.npz`, which load_particles assembles; interpolate is refused.

Two-way coupling (ParticlesConfig(tau_p > 0, two_way=True, mass=m), one rank): the fluid receives the drag reaction
-D_p = -mass (a_p - v_p) / tau_p of every alive particle (no gravity; mass = particle mass / fluid density) through the TRILINEAR
weights of the particle's cell, whatever `order` interpolates, each vertex share divided by the vertex's dual volume
dx_i dy_j dz_k (dual_widths), so that sum f V = -sum D_p.  Particles then sets solver.particle_feedback = Feedback (below):
build() at the end of every update (and at priming and after a restore) forms one record of 24 doubles per occupied cell, each
summed in ascending id; BaseCase.substep adds them to the derivatives of every sub-step of the next step, after the band forcing
and before the subgrid term, in eight passes by cell colour.  No atomics, one order of every sum: the same particles in any slot
order give the same bits.  Refused before anything is allocated: tau_p = 0, a mass that is missing, not positive or not finite,
a periodic direction with an odd vertex count, several ranks."""
import ctypes
import glob
import math
import os

import numpy as np

from . import _lib
from .common import DIR_X, VERT, X3dError
from .copyring import CopyRing
from .diagnostics import global_vert_coords

MAX_PARTICLES = 1 << 24  # X3D_PARTICLES_MAX of include/x3d2_hip.h
WALLS = {"reflect": 0, "absorb": 1}
DP = ctypes.POINTER(ctypes.c_double)
ROWS = ("x", "v", "a", "v_prev", "F", "F_prev")  # three rows each; tracers hold the first four
FLAGS = ((1, "more leavers than mig_capacity in one step (they stayed on this rank)"),
         (2, "more residents than capacity (arrivals that did not fit were not taken)"),
         (4, "a particle is owned neither by this rank nor by a neighbour of the direction it left in"))


class ParticlesConfig:
    """x0: [n, 3] start positions, 1 <= n <= 2^24; order 2 or 4; tau_p = 0: tracers; v0: [n, 3] start velocities of
    inertial particles (None: the fluid's); wall: "reflect" or "absorb"; advance from iteration initpart on (<= 0: never);
    a file every ipartout iterations (0: none); sort by cell every sort_every iterations (0: never; 8 is the measured
    minimum of advance plus amortised sort, README); several ranks: capacity slots of state per rank (None:
    ceil(1.5 n / nproc) + 1024) and mig_capacity slots per migration message (None: max(1024, capacity // 8)); two_way: the
    drag reaction acts on the fluid (inertial particles on one rank), with mass = one positive finite number, a particle's
    mass divided by the fluid density (mass_for_loading gives it from a mass loading)"""

    def __init__(self, x0, order=4, tau_p=0.0, gravity=(0.0, 0.0, 0.0), v0=None, wall="reflect", initpart=1, ipartout=0,
                 prefix="particles", sort_every=8, capacity=None, mig_capacity=None, two_way=False, mass=None):
        self.two_way = bool(two_way)
        self.mass = None
        if self.two_way:  # (refused before anything else is looked at: nothing of a refused config exists)
            if not float(tau_p) > 0.0:
                raise X3dError("ParticlesConfig: two_way needs inertial particles (tau_p > 0): a tracer exerts no drag")
            if mass is None or isinstance(mass, (str, bytes, bool)) or not isinstance(mass, (int, float, np.integer, np.floating)) \
                    or not math.isfinite(float(mass)) or not float(mass) > 0.0:
                raise X3dError("ParticlesConfig: two_way needs mass, one positive finite number: a particle's mass divided by "
                               "the fluid density (got %r)" % (mass,))
            self.mass = float(mass)
        x = np.array(x0, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != 3 or not 1 <= x.shape[0] <= MAX_PARTICLES:
            raise X3dError("ParticlesConfig: x0 is an [n, 3] array of positions, 1 <= n <= %d" % MAX_PARTICLES)
        if not np.all(np.isfinite(x)):
            raise X3dError("ParticlesConfig: a position is not finite")
        self.x0 = x
        self.order = int(order)
        if self.order not in (2, 4):
            raise X3dError("ParticlesConfig: order is 2 or 4")
        self.tau_p = float(tau_p)
        if not np.isfinite(self.tau_p) or self.tau_p < 0.0:
            raise X3dError("ParticlesConfig: tau_p must be finite and not negative")
        g = np.array(gravity, dtype=np.float64)
        if g.shape != (3,) or not np.all(np.isfinite(g)):
            raise X3dError("ParticlesConfig: gravity is three finite values")
        self.gravity = tuple(float(v) for v in g)
        self.v0 = None
        if v0 is not None:
            if self.tau_p == 0.0:
                raise X3dError("ParticlesConfig: v0 is for inertial particles (tau_p > 0); a tracer's velocity is the fluid's")
            v = np.array(v0, dtype=np.float64)
            if v.shape != x.shape or not np.all(np.isfinite(v)):
                raise X3dError("ParticlesConfig: v0 is an [n, 3] array of finite velocities")
            self.v0 = v
        if wall not in WALLS:
            raise X3dError("ParticlesConfig: wall is \"reflect\" or \"absorb\"")
        self.wall = wall
        self.initpart, self.ipartout, self.sort_every = int(initpart), int(ipartout), int(sort_every)
        if self.ipartout < 0 or self.sort_every < 0:
            raise X3dError("ParticlesConfig: ipartout and sort_every must not be negative")
        self.prefix = str(prefix)
        self.capacity = None if capacity is None else int(capacity)
        self.mig_capacity = None if mig_capacity is None else int(mig_capacity)
        if (self.capacity is not None and not 1 <= self.capacity <= MAX_PARTICLES) or \
                (self.mig_capacity is not None and self.mig_capacity < 1):
            raise X3dError("ParticlesConfig: capacity is 1 to %d, mig_capacity at least 1" % MAX_PARTICLES)

    def capacities(self, nproc):
        """(capacity, mig_capacity) on `nproc` ranks"""
        cap = self.capacity if self.capacity is not None else min(MAX_PARTICLES, int(math.ceil(1.5 * self.n / nproc)) + 1024)
        mig = self.mig_capacity if self.mig_capacity is not None else max(1024, cap // 8)
        return cap, mig  # (a message has one length on every rank, whatever the rank's own capacity)

    @property
    def n(self):
        return int(self.x0.shape[0])

    @property
    def inertial(self):
        return self.tau_p > 0.0

    def output_due(self, it):
        return self.ipartout > 0 and it % self.ipartout == 0

    def sort_due(self, it):
        return self.sort_every > 0 and it % self.sort_every == 0


def ab2_coefficients(first):
    """(c1, c0) of x += dt (c1 v + c0 v_prev): explicit Euler on the first advance after priming, AB2 afterwards"""
    return (1.0, 0.0) if first else (1.5, -0.5)


def mass_for_loading(mesh, n, phi):
    """the `mass` of ParticlesConfig at which n particles carry the mass loading phi (particle mass over fluid mass in the
    box): phi Lx Ly Lz / n"""
    n, phi = int(n), float(phi)
    if n < 1 or not math.isfinite(phi) or not phi > 0.0:
        raise X3dError("mass_for_loading: n >= 1 particles and a positive finite loading")
    return phi * float(mesh.L[0]) * float(mesh.L[1]) * float(mesh.L[2]) / n


def dual_widths(c, periodic, L):
    """d_i of the vertices c of one direction, the factors of a vertex's dual volume: L / n in a periodic (uniform) direction;
    otherwise half the first and the last spacing at the ends and (c[i + 1] - c[i - 1]) / 2 between them"""
    c = np.asarray(c, dtype=np.float64)
    n = c.size
    if periodic:
        return np.full(n, float(L) / n)
    d = np.empty(n)
    d[0], d[-1] = 0.5 * (c[1] - c[0]), 0.5 * (c[-1] - c[-2])
    d[1:-1] = 0.5 * (c[2:] - c[:-2])
    return d


def check_two_way(mesh, comm_size):
    """X3dError for a mesh or a communicator the two-way coupling does not serve"""
    if int(mesh.nproc) != 1 or int(comm_size) != 1:
        raise X3dError("Particles: two_way is not built on several ranks (the mesh has %d, the communicator %d)"
                       % (int(mesh.nproc), int(comm_size)))
    for d in range(3):
        n = int(mesh.global_vert_dims[d])
        if mesh.periodic_BC[d] and n % 2:
            raise X3dError("Particles: two_way needs an even vertex count in a periodic direction (the cell colouring), "
                           "direction %d has %d" % (d + 1, n))


def seed_uniform(mesh, n, seed=0):
    """[n, 3] positions drawn uniformly over the domain: [0, L) of a periodic direction, [first, last vertex] of any other"""
    rng = np.random.default_rng(seed)
    out = np.empty((int(n), 3))
    for d in range(3):
        c = global_vert_coords(mesh, d)
        lo, hi = (0.0, float(mesh.L[d])) if mesh.periodic_BC[d] else (float(c[0]), float(c[-1]))
        out[:, d] = lo + (hi - lo) * rng.random(int(n))
        if mesh.periodic_BC[d]:
            out[:, d] = np.where(out[:, d] >= hi, 0.0, out[:, d])
    return out


def wrap(x, L):
    """part_wrap of csrc/particles.hip, as the host applies it before it asks who owns a start position"""
    x = np.asarray(x, dtype=np.float64)
    y = x - L * np.floor(x / L)
    y = np.where(y >= L, 0.0, y)
    return np.where(y < 0.0, 0.0, y)


def owner_index(c, nproc, periodic, L, x):
    """the position along one direction of the rank that owns each (wrapped, in-domain) coordinate of x: rank r owns
    c[r nl] <= x < c[(r + 1) nl], the last rank up to L (periodic) or up to and including the last vertex; -1: nobody"""
    c, x = np.asarray(c, dtype=np.float64), np.asarray(x, dtype=np.float64)
    nl = c.size // int(nproc)
    out = np.full(x.shape, -1, dtype=np.int64)
    for r in range(int(nproc)):
        own = x >= c[r * nl]
        own &= ((x < L) if periodic else (x <= c[-1])) if r == nproc - 1 else (x < c[(r + 1) * nl])
        out[own] = r
    return out


def file_name(prefix, it, rank=None):
    return "%s_%06d.npz" % (prefix, int(it)) if rank is None else "%s_%06d.r%d.npz" % (prefix, int(it), int(rank))


def by_id(id_, *arrays):
    """the arrays (particles along the LAST axis) brought from device order into id order"""
    order = np.argsort(np.asarray(id_), kind="stable")
    return [np.ascontiguousarray(np.asarray(a)[..., order]) for a in arrays]


def unpack(raw, n, sorted_ids=False):
    """the bytes x3d_particles_pack wrote -> dict of id, x, v, a [n, 3], alive, status in id order (sorted_ids: the ids are
    a rank's own, not 0..n-1)"""
    raw = np.asarray(raw)
    rows = raw[:72 * n].view(np.float64).reshape(9, n)
    ints = raw[72 * n:80 * n].view(np.int32).reshape(2, n)
    rows, status = by_id(ints[0], rows, ints[1])
    return {"id": np.sort(ints[0]).astype(np.int64) if sorted_ids else np.arange(n, dtype=np.int64), "x": rows[0:3].T.copy(), "v": rows[3:6].T.copy(), "a": rows[6:9].T.copy(),
            "alive": (status == 1).astype(np.int32), "status": status.astype(np.int32)}


def load_particles(prefix, it):
    """the file write(it) left, as a dict (id order): id, x, v, a, alive, status, iteration, time"""
    name = file_name(prefix, it)
    parts = [] if os.path.exists(name) else sorted(glob.glob(glob.escape(name[:-4]) + ".r*.npz"))
    try:
        if parts:  # the pieces of a decomposed run, assembled in id order
            pieces = []
            for q in parts:
                with np.load(q, allow_pickle=False) as z:
                    pieces.append({k: z[k] for k in z.files})
            ids = np.concatenate([q["id"] for q in pieces])
            order = np.argsort(ids, kind="stable")
            if not np.array_equal(ids[order], np.arange(ids.size)):
                raise ValueError("the ids of the pieces are not 0..n-1, each once")
            out = {k: (np.concatenate([q[k] for q in pieces])[order] if np.ndim(v) else v) for k, v in pieces[0].items()}
            name = name[:-4] + ".r<rank>.npz"
        else:
            with np.load(name, allow_pickle=False) as z:
                out = {k: z[k] for k in z.files}
    except Exception as e:
        raise X3dError("load_particles: cannot read %s: %s: %s" % (name, type(e).__name__, e))
    for k in ("id", "x", "v", "a", "alive", "iteration", "time"):
        if k not in out:
            raise X3dError("load_particles: %s is not a particle file: no `%s`" % (name, k))
    return out


def check_state_dict(z, n, order, tau_p):
    """does the checkpoint `z` hold the particles of this run?  Raises an X3dError that names what differs."""
    if "particles_n" not in z:
        raise X3dError("restore: this run has particles, the checkpoint holds none")
    for key, here in (("n", int(n)), ("order", int(order))):
        if int(z["particles_" + key]) != here:
            raise X3dError("restore: particles_%s differs: the checkpoint has %d, this run %d" % (key, int(z["particles_" + key]), here))
    if float(z["particles_tau_p"]) != float(tau_p):
        raise X3dError("restore: particles_tau_p differs: the checkpoint has %r, this run %r" % (float(z["particles_tau_p"]), float(tau_p)))
    nrow = 18 if tau_p > 0.0 else 12
    rows, status = np.asarray(z["particles_rows"]), np.asarray(z["particles_status"])
    if "particles_id" in z:  # a rank's own particles of a decomposed run
        n = int(np.asarray(z["particles_id"]).size)
    if rows.shape != (nrow, n) or rows.dtype != np.float64 or status.shape != (n,):
        raise X3dError("restore: particles_rows is %s %s, this run needs float64 %s" % (rows.dtype.name, rows.shape, (nrow, n)))


class Particles:
    """Particles(solver, cfg), attached as `case.particles = Particles(case.solver, cfg)`: BaseCase.run then calls update(it),
    write(it) and poll() once per step and finalise() at the end; checkpoint.Checkpoints carries state_dict()."""

    def __init__(self, solver, cfg):
        self.h, self.feedback = None, None  # (a refusal below leaves both)
        self.solver, self.cfg = solver, cfg
        b, m = solver.backend, solver.mesh
        if cfg.two_way:
            check_two_way(m, int(getattr(b.comm, "size", 1)))
        self.mp = int(m.nproc) != 1
        self.rank, self.comm = int(m.nrank), b.comm
        self.n, self.nrow = cfg.n, 18 if cfg.inertial else 12
        dims = [int(v) for v in m.get_dims(VERT)]
        if self.mp:
            if int(m.nproc_dir[0]) > 1:
                raise X3dError("Particles: x is never cut (nproc_dir[0] = %d)" % int(m.nproc_dir[0]))
            for d in (1, 2):
                if int(m.nproc_dir[d]) > 1 and dims[d] < 4:
                    raise X3dError("Particles: a rank needs at least 4 vertices in a cut direction, direction %d has %d" % (d + 1, dims[d]))
            if int(getattr(b.comm, "size", 1)) != int(m.nproc):
                raise X3dError("Particles: the mesh is cut into %d ranks, the backend's communicator has %d: multi-rank particles "
                               "are not built without one process per rank" % (int(m.nproc), int(getattr(b.comm, "size", 1))))
        if cfg.order == 4 and min(int(v) for v in m.global_vert_dims) < 4:
            raise X3dError("Particles: order 4 needs at least 4 vertices per direction")
        if cfg.inertial and cfg.tau_p < 2.0 * float(solver.dt):
            raise X3dError("Particles: 0 < tau_p < 2 dt is refused (AB2 on the drag term needs dt / tau_p <= 0.5)")
        self.coords = [np.ascontiguousarray(global_vert_coords(m, d), dtype=np.float64) for d in range(3)]
        prm = _lib.ParticlesParams()
        prm.n, prm.order, prm.wall, prm.tau = self.n, cfg.order, WALLS[cfg.wall], cfg.tau_p
        for d in range(3):
            prm.g[d] = cfg.gravity[d]
            prm.periodic[d] = int(bool(m.periodic_BC[d]))
            prm.uniform[d] = int(not m.stretched[d])
            prm.L[d] = float(m.L[d])
            prm.coords[d] = self.coords[d].ctypes.data_as(DP)
        self.lib, self.h = b.lib, ctypes.c_void_p()
        if self.mp:
            self._create_mp(prm, dims)
        else:
            x0 = np.ascontiguousarray(cfg.x0.T)
            v0 = np.ascontiguousarray(cfg.v0.T) if cfg.v0 is not None else None
            _lib.check(b.lib.x3d_particles_create(b.h, ctypes.byref(prm), x0.ctypes.data_as(DP),
                                                  v0.ctypes.data_as(DP) if v0 is not None else None, ctypes.byref(self.h)))
        self.ring = CopyRing(b, 2, self._write_file)  # (nothing is allocated until the first write)
        self.files = []
        self.iteration = int(solver.current_iter)  # the iteration the state belongs to
        if cfg.two_way:
            self.feedback = Feedback(self)
        self.prime()
        if cfg.two_way:
            self._records()
            solver.particle_feedback = self.feedback

    def _records(self):
        """two-way coupling: the records of the state as it is, from iteration initpart - 1 on; before that the particles
        rest and nothing is added"""
        if self.reads_state(self.iteration):
            self.feedback.build()
        else:
            self.feedback.built = False

    def owned(self, x):
        """which of the (wrapped) positions x [m, 3] this rank owns"""
        m = self.solver.mesh
        mask = np.ones(x.shape[0], dtype=bool)
        for d in (1, 2):
            if int(m.nproc_dir[d]) > 1:
                mask &= owner_index(self.coords[d], int(m.nproc_dir[d]), bool(m.periodic_BC[d]), float(m.L[d]), x[:, d]) == \
                    int(m.nrank_dir[d])
        return mask

    def _create_mp(self, prm, dims):
        import torch
        b, m, cfg = self.solver.backend, self.solver.mesh, self.cfg
        x = cfg.x0.copy()
        for d in range(3):
            if m.periodic_BC[d]:
                x[:, d] = wrap(x[:, d], float(m.L[d]))
        ids = np.ascontiguousarray(np.nonzero(self.owned(x))[0], dtype=np.int32)
        self.capacity, self.mig_capacity = cfg.capacities(int(m.nproc))
        if ids.size > self.capacity:
            raise X3dError("Particles: rank %d owns %d particles at the start, capacity is %d" % (self.rank, ids.size, self.capacity))
        dc = _lib.ParticlesDecomp()
        for d in range(3):
            dc.nglobal[d], dc.offset[d], dc.nlocal[d] = int(m.global_vert_dims[d]), int(m.n_offset[d]), dims[d]
            dc.nproc[d], dc.rank[d] = int(m.nproc_dir[d]), int(m.nrank_dir[d])
        dc.capacity, dc.mig_capacity = self.capacity, self.mig_capacity
        x0 = np.ascontiguousarray(x[ids].T)
        v0 = np.ascontiguousarray(cfg.v0[ids].T) if cfg.v0 is not None else None
        _lib.check(b.lib.x3d_particles_mp_create(b.h, ctypes.byref(prm), ctypes.byref(dc), x0.ctypes.data_as(DP),
                                                 v0.ctypes.data_as(DP) if v0 is not None else None,
                                                 ids.ctypes.data_as(_lib.c_int_p), int(ids.size), ctypes.byref(self.h)))
        # the messages: per cut direction (to pprev, to pnext, from pprev, from pnext)
        real = torch.float64 if np.dtype(_lib.NP_REAL) == np.dtype(np.float64) else torch.float32
        gh, nx, ny, nz = (2 if cfg.order == 4 else 1), dims[0], dims[1], dims[2]
        self.dirs = [d for d in (1, 2) if int(m.nproc_dir[d]) > 1]
        self.ghost_buf, self.mig_buf = {}, {}
        for d in self.dirs:
            nr = nz if d == 1 else ny + 1 + gh
            lo, hi = 3 * gh * nr * nx, 3 * nr * nx  # (what goes down serves the neighbour's gh planes above)
            self.ghost_buf[d] = tuple(torch.zeros(k, dtype=real, device=b.device) for k in (lo, hi, hi, lo))
            self.mig_buf[d] = tuple(torch.zeros(1 + (self.nrow + 1) * self.mig_capacity, dtype=torch.float64, device=b.device)
                                    for _ in range(4))

    def __del__(self):
        try:
            if self.h is not None:
                self.lib.x3d_particles_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ------------------------------------------------------------ the launches
    def _fields(self, u, v, w):
        b = self.solver.backend
        for f in (u, v, w):
            if f.dir != DIR_X:
                raise X3dError("Particles: DIR_X fields are needed")
        b._need_vert("Particles", u, v, w)
        return u.ptr, v.ptr, w.ptr, b._dims(VERT)

    def _ghosts(self, ptrs):
        """the face planes the stencil reaches, y then z: pack, exchange, unpack"""
        b, m = self.solver.backend, self.solver.mesh
        for d in self.dirs:
            ss, se, rs, re = self.ghost_buf[d]
            _lib.check(self.lib.x3d_particles_mp_ghost_pack(b.h, self.h, d + 1, *ptrs, ss.data_ptr(), se.data_ptr()))
            self.comm.sendrecv([(ss, se, rs, re)], int(m.pprev[d]), int(m.pnext[d]))
            _lib.check(self.lib.x3d_particles_mp_ghost_unpack(b.h, self.h, d + 1, rs.data_ptr(), re.data_ptr()))

    def _migrate(self):
        b, m = self.solver.backend, self.solver.mesh
        for d in self.dirs:
            ss, se, rs, re = self.mig_buf[d]
            _lib.check(self.lib.x3d_particles_mp_emigrate(b.h, self.h, d + 1, ss.data_ptr(), se.data_ptr()))
            self.comm.sendrecv([(ss, se, rs, re)], int(m.pprev[d]), int(m.pnext[d]))
            _lib.check(self.lib.x3d_particles_mp_immigrate(b.h, self.h, d + 1, rs.data_ptr(), re.data_ptr()))

    def prime(self):
        """a = u(x) from the solver's fields as they are; v and F from it.  The next advance is a first one."""
        s = self.solver
        s.flush_grad()  # a velocity correction left pending by step(more=True) is not in u, v, w yet
        ptrs = self._fields(s.u, s.v, s.w)
        if self.mp:
            self._ghosts(ptrs)
            _lib.check(self.lib.x3d_particles_mp_prime(s.backend.h, self.h, *ptrs))
        else:
            _lib.check(self.lib.x3d_particles_prime(s.backend.h, self.h, *ptrs))

    def advance(self, u, v, w, dt):
        """one launch on fields of the caller's; several ranks: move, migrate, ghosts, sample (collective)"""
        b = self.solver.backend
        ptrs = self._fields(u, v, w)
        if not self.mp:
            _lib.check(self.lib.x3d_particles_advance(b.h, self.h, *ptrs, float(dt)))
            return
        _lib.check(self.lib.x3d_particles_mp_move(b.h, self.h, float(dt)))
        self._migrate()
        self._ghosts(ptrs)
        _lib.check(self.lib.x3d_particles_mp_sample(b.h, self.h, *ptrs))

    def sort(self):
        f = self.lib.x3d_particles_mp_sort if self.mp else self.lib.x3d_particles_sort
        _lib.check(f(self.solver.backend.h, self.h))

    def interpolate(self, points, u, v, w):
        """[m, 3] values of (u, v, w) at the [m, 3] points: one launch, one host wait.  A point outside a non-periodic
        direction's [first, last vertex] or one that is not finite is an error."""
        import torch
        if self.mp:
            raise X3dError("Particles.interpolate: not built on several ranks")
        b = self.solver.backend
        pts = np.array(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != 3 or not 1 <= pts.shape[0] <= MAX_PARTICLES:
            raise X3dError("Particles.interpolate: points is an [m, 3] array, 1 <= m <= %d" % MAX_PARTICLES)
        if not np.all(np.isfinite(pts)):
            raise X3dError("Particles.interpolate: a point is not finite")
        for d in range(3):
            c = self.coords[d]
            if not self.solver.mesh.periodic_BC[d] and (np.any(pts[:, d] < c[0]) or np.any(pts[:, d] > c[-1])):
                raise X3dError("Particles.interpolate: a point lies outside [%g, %g] of direction %d" % (c[0], c[-1], d + 1))
        m = int(pts.shape[0])
        ptrs = self._fields(u, v, w)
        dev = torch.from_numpy(np.ascontiguousarray(pts.T)).to(b.device)
        out = torch.empty((3, m), dtype=torch.float64, device=b.device)
        _lib.check(self.lib.x3d_particles_interpolate(b.h, self.h, *ptrs, dev.data_ptr(), m, out.data_ptr()))
        return out.cpu().numpy().T.copy()

    # ------------------------------------------------------------ BaseCase.run's protocol
    def reads_state(self, it):
        """does update(it) read the solver's fields?  At every step from initpart on, and at initpart - 1, where the
        resting particles are primed."""
        return self.cfg.initpart > 0 and it >= self.cfg.initpart - 1

    def update(self, it):
        """advance to iteration `it` (the fields hold u^it, the state is at it - 1); returns whether the particles moved.
        No host wait.  An iteration other than the next one is an error, never a silently skipped step."""
        if it != self.iteration + 1:
            raise X3dError("Particles.update: iteration %d after %d (every step is needed, in order)" % (it, self.iteration))
        cfg, s = self.cfg, self.solver
        moved = cfg.initpart > 0 and it >= cfg.initpart
        if moved:
            s.flush_grad()
            self.advance(s.u, s.v, s.w, s.dt)
            if cfg.sort_due(it):
                self.sort()
        elif self.reads_state(it):
            self.prime()  # it == initpart - 1, resting until now: the history starts here
        self.iteration = it  # (only once the launches were accepted: a refused advance leaves the count with the state)
        if self.feedback is not None:
            self._records()  # applied unchanged in every sub-step of step it + 1
        return moved

    def write(self, it):
        """if iteration `it` is due: one pack launch, one asynchronous copy; no host wait unless both slots are in flight"""
        if not self.cfg.output_due(it):
            return False
        if it != self.iteration:
            raise X3dError("Particles.write: iteration %d, the state is at %d" % (it, self.iteration))
        b = self.solver.backend
        nbytes = 80 * self.capacity + 8 if self.mp else 80 * self.n
        slot = self.ring.acquire(nbytes)
        pack = self.lib.x3d_particles_mp_pack if self.mp else self.lib.x3d_particles_pack
        _lib.check(pack(b.h, self.h, slot.dev.data_ptr(), nbytes))
        self.ring.submit(slot, nbytes, (int(it), float(it * self.solver.dt)))
        return True

    def _write_file(self, payload, raw):
        it, t = payload
        if self.mp:  # `capacity` slots, then the local count and the flags: trimmed here
            raw, cap = np.asarray(raw), self.capacity
            n, flags = (int(v) for v in raw[80 * cap:80 * cap + 8].view(np.int32))
            self._raise_flags(flags)
            rows = raw[:72 * cap].view(np.float64).reshape(9, cap)[:, :n]
            ints = raw[72 * cap:80 * cap].view(np.int32).reshape(2, cap)[:, :n]
            out = unpack(np.concatenate([np.ascontiguousarray(rows).view(np.uint8).ravel(),
                                         np.ascontiguousarray(ints).view(np.uint8).ravel()]), n, sorted_ids=True)
        else:
            out = unpack(raw, self.n)
        out["iteration"], out["time"] = np.int64(it), np.float64(t)
        name = file_name(self.cfg.prefix, it, self.rank if self.mp else None)
        with open(name, "wb") as fh:
            np.savez(fh, **out)
        self.files.append(name)
        return name

    def poll(self):
        """write the files whose copies have landed; never blocks"""
        return self.ring.poll()

    def finalise(self):
        """wait for and write what is left"""
        return self.ring.drain()

    @property
    def sync_count(self):
        return self.ring.waits

    # ------------------------------------------------------------ the state on the host
    def _raise_flags(self, flags):
        if flags:
            raise X3dError("Particles: rank %d: %s" % (self.rank, "; ".join(text for bit, text in FLAGS if flags & bit)))

    def check(self):
        """one host wait: raises if this rank's migration ever overflowed or lost track of a particle; returns the local count"""
        if not self.mp:
            return self.n
        q = _lib.ints(0, 0)
        _lib.check(self.lib.x3d_particles_mp_query(self.solver.backend.h, self.h, q))
        self._raise_flags(int(q[1]))
        return int(q[0])

    def raw_state(self):
        """(rows [12 or 18, n], id, status, has_history) in DEVICE order; one host wait.  Several ranks: this rank's own."""
        n = self.capacity if self.mp else self.n
        rows = np.empty((self.nrow, n), dtype=np.float64)
        id_, status = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        hist = ctypes.c_int(0)
        args = (self.solver.backend.h, self.h, rows.ctypes.data_as(DP), id_.ctypes.data_as(_lib.c_int_p),
                status.ctypes.data_as(_lib.c_int_p))
        if not self.mp:
            _lib.check(self.lib.x3d_particles_download(*args, ctypes.byref(hist)))
            return rows, id_, status, bool(hist.value)
        nl, flags = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(self.lib.x3d_particles_mp_download(*args, ctypes.byref(nl), ctypes.byref(flags), ctypes.byref(hist)))
        self._raise_flags(flags.value)
        nl = nl.value
        return rows.ravel()[:self.nrow * nl].reshape(self.nrow, nl).copy(), id_[:nl].copy(), status[:nl].copy(), bool(hist.value)

    def _gathered(self):
        """(rows, id, status, has_history) of ALL ranks, rank after rank (collective; pickled bytes, so every bit survives)"""
        rows, id_, status, hist = self.raw_state()
        if not self.mp:
            return rows, id_, status, hist
        import torch.distributed as dist
        parts = [None] * self.comm.size
        dist.all_gather_object(parts, (rows, id_, status), group=self.comm.group)
        rows, id_, status = (np.concatenate([q[k] for q in parts], axis=-1) for k in range(3))
        if not np.array_equal(np.sort(id_), np.arange(self.n)):
            raise X3dError("Particles.state: the ids over the ranks are not 0..n-1, each once")
        return rows, id_, status, hist

    def state(self):
        """id, x, v, a [n, 3], alive, status, iteration, time in id order: the only host wait.  Several ranks: collective,
        the global state on every rank."""
        rows, id_, status, _ = self._gathered()
        rows, status = by_id(id_, rows, status)
        return {"id": np.arange(self.n, dtype=np.int64), "x": rows[0:3].T.copy(), "v": rows[3:6].T.copy(),
                "a": rows[6:9].T.copy(), "alive": (status == 1).astype(np.int32), "status": status.astype(np.int32),
                "iteration": np.int64(self.iteration), "time": np.float64(self.iteration * self.solver.dt)}

    def state_dict(self):
        """everything a resumed run needs, through the host in id order, under `particles_*` keys: 12 (tracers) or 18
        (inertial) doubles and one int per particle.  Several ranks: the rank's own particles and their `particles_id`."""
        rows, id_, status, hist = self.raw_state()
        rows, status = by_id(id_, rows, status)
        out = {"particles_n": np.int64(self.n), "particles_order": np.int64(self.cfg.order),
               "particles_tau_p": np.float64(self.cfg.tau_p), "particles_iteration": np.int64(self.iteration),
               "particles_has_history": np.bool_(hist), "particles_rows": rows, "particles_status": status.astype(np.int32)}
        if self.mp:
            out["particles_id"] = np.sort(id_).astype(np.int32)
        return out

    def load_state_dict(self, z):
        check_state_dict(z, self.n, self.cfg.order, self.cfg.tau_p)
        if self.mp != ("particles_id" in z):
            raise X3dError("restore: the particles of the checkpoint belong to another decomposition")
        rows = np.ascontiguousarray(z["particles_rows"], dtype=np.float64)
        status = np.ascontiguousarray(z["particles_status"], dtype=np.int32)
        b = self.solver.backend
        if self.mp:  # (a particle this rank does not own is refused by the library: another rank's file)
            id_ = np.ascontiguousarray(z["particles_id"], dtype=np.int32)
            _lib.check(self.lib.x3d_particles_mp_upload(b.h, self.h, rows.ctypes.data_as(DP), id_.ctypes.data_as(_lib.c_int_p),
                                                        status.ctypes.data_as(_lib.c_int_p), int(id_.size),
                                                        int(bool(z["particles_has_history"]))))
        else:
            id_ = np.arange(self.n, dtype=np.int32)
            _lib.check(self.lib.x3d_particles_upload(b.h, self.h, rows.ctypes.data_as(DP), id_.ctypes.data_as(_lib.c_int_p),
                                                     status.ctypes.data_as(_lib.c_int_p), int(bool(z["particles_has_history"]))))
        self.iteration = int(z["particles_iteration"])
        if self.feedback is not None:
            self._records()  # from the restored x, v, a: the records are no state of their own


class Feedback:
    """The drag reaction of two-way coupled particles on the fluid, Particles.feedback and solver.particle_feedback
    (csrc/particles.hip, x3d_particles_feedback_*).  build() forms the records of the occupied cells from the particle state as
    it is (Particles does it at the end of every update, at priming and after a restore); add(du, dv, dw) applies them to three
    derivative blocks in eight passes by cell colour (BaseCase.substep, after the band forcing and before the subgrid term);
    before the first build nothing is added.  No call waits for the host except field() readers and records()."""

    coupled = True  # the derivatives must be stored: BaseCase.substep's explicit branch

    def __init__(self, particles):
        p = self.particles = particles
        m, b = p.solver.mesh, p.solver.backend
        self.lib, self.mass, self.built = b.lib, float(p.cfg.mass), False
        self.inv_d = [np.ascontiguousarray(1.0 / dual_widths(p.coords[d], bool(m.periodic_BC[d]), float(m.L[d]))) for d in range(3)]
        _lib.check(self.lib.x3d_particles_feedback_enable(b.h, p.h, self.mass, *(t.ctypes.data_as(DP) for t in self.inv_d)))

    def build(self):
        """keys, sort, records of the state as it is; no host wait"""
        p = self.particles
        _lib.check(self.lib.x3d_particles_feedback_build(p.solver.backend.h, p.h))
        self.built = True

    def add(self, du, dv, dw):
        """du, dv, dw += f of the records; no host wait"""
        if not self.built:
            return
        p = self.particles
        b = p.solver.backend
        for f in (du, dv, dw):
            if f.dir != DIR_X or f.data_loc != VERT:
                raise X3dError("Feedback.add: DIR_X blocks at VERT are needed")
        _lib.check(self.lib.x3d_particles_feedback_add(b.h, p.h, du.ptr, dv.ptr, dw.ptr, b._dims(VERT)))

    def field(self):
        """f itself, for tests and snapshots: the same passes into three zeroed blocks of the allocator's, which the caller
        releases"""
        al = self.particles.solver.backend.allocator
        out = [al.get_block(DIR_X, VERT) for _ in range(3)]
        for f in out:
            f.fill(0.0)
        self.add(*out)
        return out

    def records(self):
        """(counts[9]: the first record of each colour and the number of occupied cells, cells[q], records[q, 8, 3]) in the
        order of the colour lists; one host wait"""
        p = self.particles
        counts = _lib.ints(*([0] * 9))
        cells, rec = np.zeros(p.n, dtype=np.uint32), np.zeros((p.n, 8, 3))
        _lib.check(self.lib.x3d_particles_feedback_download(p.solver.backend.h, p.h, counts, cells.ctypes.data, rec.ctypes.data))
        q = int(counts[8])
        return np.array(list(counts), dtype=np.int64), cells[:q].copy(), rec[:q].copy()
