"""Active scalars: what turns the transported species of SolverConfig(n_species, pr_species) into a heated channel, a
Rayleigh-Benard cell or a stratified box -- initial values, Dirichlet wall values, Boussinesq buoyancy, an imposed mean
gradient, and the scalar-flux profiles such runs are judged by.  On the device (csrc/scalars.hip).  Not in the reference (x3d2
transports species but never sets, bounds or couples one): this project's addition.

    case = make_channel((128, 65, 64), fused=True, n_species=1, pr_species=[0.71])
    s = case.solver
    s.scalars = Scalars(s, ScalarsConfig(ri=[0.1], wall=[{"y": (1.0, 0.0)}], init=[lambda x, y, z: 1.0 - y / 2.0],
                                         profile_dir=2, initstat=1000))
    case.run(n_iters=...)
    m = s.scalars.monitor()   # plane means now, phi_min, phi_max, nu_lo, nu_hi, nu_vol: one host wait, only when asked

Physics, with ns species phi_s (s counts from 0 here; phi_1 .. phi_ns in the file names of statistics and checkpoints):
    du_i   +=  up_i sum_s ri_s (phi_s - ref_s)       i = x, y, z        Boussinesq buoyancy
    dphi_s +=  -(G_s,x u + G_s,y v + G_s,z w)                           imposed mean scalar gradient
    phi_s   =  value on a face of a non-periodic direction, after every sub-step's stage   Dirichlet wall value
up: the direction AGAINST gravity, three finite numbers, not normalised -- its length is part of the coefficient.  ri[s]: a
Richardson-type coefficient (0: passive).  ref[s]: reference value.  grad[s] = G_s: three numbers, default 0.  wall[s]: None,
or per non-periodic direction ("x", "y", "z" or 0, 1, 2) a pair (lo, hi), each None or a finite value.  A point on two stamped
faces takes the value of the later direction in the order x, y, z.

The driver (BaseCase.substep): transeq -> forcings -> Scalars.add -> stage -> apply_BC -> Scalars.apply_bc -> pressure
correction.  A coupled Scalars (some ri_s |up| != 0 or some G != 0) needs the derivatives stored before the stage, so the
fused driver gives up the branch that folds transeq's last accumulation into the stage; an uncoupled one (initial values,
walls, profiles only) keeps it.  Species are never part of a deferred update, so the stamp right after the stage is final.

Profiles (profile_dir = 2 or 3; 1 is not built): one pass over u, v, w and the species leaves, per species and plane, the
sums of phi, phi phi, u phi, v phi, w phi (and min / max of phi over the rank); on several ranks the plane sums are added over
all ranks before they enter the running mean, which is Stats' recurrence (x3d_stats_profile_accumulate).

Nusselt numbers (monitor(), profile_dir along a direction with both wall values of species s set and whole on every rank).
With kappa = solver.nu_species[s], c the vertex coordinates along profile_dir, H = c[-1] - c[0], dphi = wall lo - wall hi,
pbar the plane means of phi_s and q the plane means of (up . u) phi_s / |up|:
    nu_lo, nu_hi = -kappa dpbar/dn at the first / last vertex, by the three-point one-sided difference on the ACTUAL
                   coordinates, over kappa dphi / H
    nu_vol       = 1 + <q>_V H / (kappa dphi),  <q>_V = the trapezoid rule on c, over H
All three are 1 for pure conduction.

Refused, each an X3dError before anything is allocated or launched: no species; a list whose length is not nspecies; a value
that is not finite; a wall value in a periodic direction; profile_dir not in (None, 2, 3); solver.les set to a model that
does not serve species (les.Les with LesConfig(prt=...) does: its serves_species is true); fields not at VERT.

With such an LES model attached the species' right-hand side also gets the subgrid flux of the eddy diffusivity nu_t / Pr_t
(Les.add).  The profiles and nu_vol below do NOT include that flux: they hold the resolved part only.  nu_lo / nu_hi are
unaffected where nu_t vanishes at the wall, as WALE's does (Smagorinsky's does not, and has no wall damping here).

Not built: Neumann (adiabatic) and Robin scalar walls; variable density beyond Boussinesq; a settling velocity; the
subgrid flux in the flux profiles and nu_vol; the Fortran shim's use; profile_dir = 1; scalar terms in Budgets; buoyancy fused into
transeq's z launch (a coupled run would then keep the deferred branch)."""
import math

import numpy as np
import torch

from . import _lib
from .common import DIR_Y, DIR_Z, VERT, X3dError, sample_due

PROFILE_NAMES = ("phi", "phiphi", "uphi", "vphi", "wphi")
NMOM = len(PROFILE_NAMES)
_AXES = {"x": 0, "y": 1, "z": 2, 0: 0, 1: 1, 2: 2}


def _finite(x, what):
    try:
        x = float(x)
    except (TypeError, ValueError):
        raise X3dError("ScalarsConfig: %s is not a number" % what)
    if not math.isfinite(x):
        raise X3dError("ScalarsConfig: %s is not finite" % what)
    return x


class ScalarsConfig:
    """see the module docstring; initstat, istatfreq, istatout as StatsConfig's, for the scalar profiles"""

    def __init__(self, ri=None, ref=None, up=(0, 1, 0), grad=None, wall=None, init=None, profile_dir=None, initstat=0,
                 istatfreq=1, istatout=0, prefix="scalars"):
        self.ri = None if ri is None else [_finite(x, "ri") for x in ri]
        self.ref = None if ref is None else [_finite(x, "ref") for x in ref]
        up = tuple(up)
        if len(up) != 3:
            raise X3dError("ScalarsConfig: up has three components")
        self.up = tuple(_finite(x, "up") for x in up)
        self.grad = None
        if grad is not None:
            self.grad = []
            for g in grad:
                g = (0.0, 0.0, 0.0) if g is None else tuple(g)
                if len(g) != 3:
                    raise X3dError("ScalarsConfig: grad has three components per species")
                self.grad.append(tuple(_finite(x, "grad") for x in g))
        self.wall = None
        if wall is not None:
            self.wall = [self._wall_of(w) for w in wall]
        self.init = None if init is None else list(init)
        if profile_dir not in (None, 2, 3):
            raise X3dError("ScalarsConfig: profile_dir must be None, 2 or 3 (1 is not built)")
        self.profile_dir = profile_dir
        self.initstat, self.istatfreq, self.istatout = int(initstat), int(istatfreq), int(istatout)
        if self.istatfreq < 1:
            raise X3dError("ScalarsConfig: istatfreq must be at least 1")
        self.prefix = str(prefix)

    @staticmethod
    def _wall_of(w):
        """-> [(lo, hi)] * 3, each None or a float"""
        out = [(None, None)] * 3
        if w is None:
            return out
        items = w.items() if isinstance(w, dict) else enumerate(w)
        for key, pair in items:
            if key not in _AXES:
                raise X3dError("ScalarsConfig: a wall direction is one of x, y, z or 0, 1, 2 (got %r)" % (key,))
            if pair is None:
                continue
            pair = tuple(pair)
            if len(pair) != 2:
                raise X3dError("ScalarsConfig: a wall entry is a pair (lo, hi)")
            out[_AXES[key]] = tuple(None if v is None else _finite(v, "a wall value") for v in pair)
        return out

    @property
    def active(self):
        """are running profiles kept?"""
        return self.profile_dir is not None and self.initstat > 0

    def sample_due(self, it):
        return self.profile_dir is not None and sample_due(it, self.initstat, self.istatfreq)

    def output_due(self, it):
        return self.active and self.istatout > 0 and it % self.istatout == 0


def one_sided_slope(c, f):
    """df/dc at c[0] from the first three points, exact for a parabola on any spacing"""
    h1, h2 = c[1] - c[0], c[2] - c[0]
    return -(h1 + h2) / (h1 * h2) * f[0] + h2 / (h1 * (h2 - h1)) * f[1] - h1 / (h2 * (h2 - h1)) * f[2]


def nusselt(c, phi_mean, upphi_mean, kappa, dphi):
    """(nu_lo, nu_hi, nu_vol) of the module docstring from the plane means along the wall-normal coordinates c"""
    c, p, q = (np.asarray(a, dtype=np.float64) for a in (c, phi_mean, upphi_mean))
    H = c[-1] - c[0]
    scale = H / dphi
    nu_lo = -one_sided_slope(c, p) * scale
    nu_hi = -one_sided_slope(c[::-1], p[::-1]) * scale
    vol = float(np.sum(0.5 * (q[1:] + q[:-1]) * np.diff(c))) / H
    return float(nu_lo), float(nu_hi), float(1.0 + vol * H / (kappa * dphi))


class Scalars:
    """Scalars(solver, cfg), attached as `solver.scalars = Scalars(solver, cfg)`"""

    def __init__(self, solver, cfg=None):
        self.cfg = cfg = cfg or ScalarsConfig()
        self.solver = solver
        ns = self.ns = int(getattr(solver, "nspecies", 0))
        m = solver.mesh
        # ---- refusals: nothing is allocated or launched before the last of them
        if ns == 0:
            raise X3dError("Scalars: the solver transports no species (SolverConfig(n_species=...))")
        les = getattr(solver, "les", None)
        if les is not None and not getattr(les, "serves_species", False):
            raise X3dError("Scalars: an LES model is attached that does not serve the species (Les with LesConfig(prt=...) "
                           "adds their eddy diffusivity)")
        for name in ("ri", "ref", "grad", "wall", "init"):
            v = getattr(cfg, name)
            if v is not None and len(v) != ns:
                raise X3dError("Scalars: %s has %d entries, the solver %d species" % (name, len(v), ns))
        for f in [solver.u, solver.v, solver.w] + list(solver.species):
            if f.data_loc != VERT and not (f in solver.species and cfg.init is not None):
                raise X3dError("Scalars: every field must be at VERT")
        self.ri = list(cfg.ri) if cfg.ri is not None else [0.0] * ns
        self.ref = list(cfg.ref) if cfg.ref is not None else [0.0] * ns
        self.up = tuple(cfg.up)
        self.grad = [tuple(g) for g in cfg.grad] if cfg.grad is not None else [(0.0, 0.0, 0.0)] * ns
        self.has_grad = any(x != 0.0 for g in self.grad for x in g)
        walls = cfg.wall if cfg.wall is not None else [[(None, None)] * 3] * ns
        self.mask, self.value = [], []
        for w in walls:
            mk, val = 0, [0.0] * 6
            for d in range(3):
                for side in range(2):
                    if w[d][side] is None:
                        continue
                    if m.periodic_BC[d]:
                        raise X3dError("Scalars: a wall value in the periodic direction %s" % "xyz"[d])
                    mk |= 1 << (2 * d + side)
                    val[2 * d + side] = float(w[d][side])
            self.mask.append(mk)
            self.value.append(val)
        self.walls = walls
        # the faces of the global box that lie in this rank's block
        self.own_mask = 0
        for d in range(3):
            if int(m.nrank_dir[d]) == 0:
                self.own_mask |= 1 << (2 * d)
            if int(m.nrank_dir[d]) + 1 == int(m.nproc_dir[d]):
                self.own_mask |= 1 << (2 * d + 1)
        host_init = self._host_init(cfg.init) if cfg.init is not None else None
        # ---- from here on the solver is written
        b = solver.backend
        self.sample_count = 0
        self.prof = self.sums = self.minmax = self._global = None
        if cfg.profile_dir is not None:
            d = cfg.profile_dir - 1
            self.n_keep = int(m.get_dims(VERT)[d])
            self.n_keep_global = int(m.get_global_dims(VERT)[d])
            self.keep_offset = int(m.n_offset[d])
            self.plane_points = int(np.prod([n for i, n in enumerate(m.get_global_dims(VERT)) if i != d]))
            z = lambda n: torch.zeros(n, dtype=_lib.torch_real(), device=b.device)
            self.sums, self.minmax = z(ns * NMOM * self.n_keep), z(2 * ns)
            self.prof = z(ns * NMOM * self.n_keep) if cfg.active else None
            self._global = z(ns * NMOM * self.n_keep_global) if b.comm.size > 1 else None
        if host_init is not None:
            for f, a in zip(solver.species, host_init):
                f.set_data_loc(VERT)
                if a is None:
                    f.fill(0.0)
                else:
                    b.set_field_data(f, a)
            self.apply_bc()

    def _host_init(self, init):
        m = self.solver.mesh
        nx, ny, nz = m.get_dims(VERT)
        x = np.asarray(m.vert_coords[0])[None, None, :]
        y = np.asarray(m.vert_coords[1])[None, :, None]
        z = np.asarray(m.vert_coords[2])[:, None, None]
        out = []
        for s, v in enumerate(init):
            if v is None:
                out.append(None)
                continue
            a = v(x, y, z) if callable(v) else v
            a = np.asarray(a, dtype=np.float64)
            if a.ndim == 0:
                a = np.full((nz, ny, nx), float(a))
            elif callable(v):
                a = np.broadcast_to(a, (nz, ny, nx))
            if a.shape != (nz, ny, nx):
                raise X3dError("Scalars: init[%d] has shape %s, this rank's block %s" % (s, a.shape, (nz, ny, nx)))
            if not np.all(np.isfinite(a)):
                raise X3dError("Scalars: init[%d] is not finite" % s)
            out.append(np.ascontiguousarray(a))
        return out

    # ------------------------------------------------------------ the sub-step's two calls
    @property
    def coupled(self):
        """does add() touch a derivative?  (BaseCase.substep then needs the derivatives stored before the stage)"""
        buoyant = any(x != 0.0 for x in self.up) and any(r != 0.0 for r in self.ri)
        return buoyant or self.has_grad

    def add(self, deriv, curr):
        """deriv[0:3] += buoyancy, deriv[3:] += the imposed-gradient term, from curr = [u, v, w, phi_1, ...]: one launch per
        group of 8 species; no host wait"""
        if not self.coupled:
            return
        s = self.solver
        if self.has_grad:
            s.flush_grad()  # a velocity correction left pending is not in u, v, w yet
        s.backend.scalars_couple(deriv[0:3], deriv[3:], curr[0:3], curr[3:], self.up, self.ri, self.ref,
                                 self.grad if self.has_grad else None)

    def apply_bc(self):
        """the requested wall values on the faces this rank owns: one launch per group of 8 species; no host wait"""
        if not any(mk & self.own_mask for mk in self.mask):
            return
        s = self.solver
        s.backend.scalars_apply_bc(list(s.species), self.mask, self.value, self.own_mask)

    # ------------------------------------------------------------ profiles
    @property
    def profiling(self):
        return self.cfg.active

    def reads_state(self, it):
        """does update(it) read the solver's fields?  (BaseCase.run then completes the step first)"""
        return self.cfg.active and self.cfg.sample_due(it)

    def _sample(self):
        """self.sums <- the plane sums of the fields as they are, over all ranks; self.minmax: this rank's"""
        s = self.solver
        b = s.backend
        s.flush_grad()
        b.scalars_profile_sums(s.u, s.v, s.w, list(s.species), self.cfg.profile_dir, self.sums, self.minmax)
        if self._global is not None:
            rows = self.ns * NMOM
            g = self._global.view(rows, self.n_keep_global)
            g.zero_()
            lo = self.keep_offset
            g[:, lo:lo + self.n_keep] = self.sums.view(rows, self.n_keep)
            b.comm.allreduce_tensor(self._global)
            self.sums.view(rows, self.n_keep).copy_(g[:, lo:lo + self.n_keep])

    def update(self, it):
        """one sample if iteration `it` is due; returns whether one was taken.  No host wait."""
        if not self.reads_state(it):
            return False
        self._sample()
        self.sample_count += 1
        self.solver.backend.stats_profile_accumulate(self.prof, self.sums, 1.0 / self.plane_points, 1.0 / self.sample_count)
        return True

    def _need_active(self):
        if not self.cfg.active:
            raise X3dError("scalar profiles are inactive (profile_dir is None or initstat <= 0)")

    def profiles(self):
        """the running means phi, phiphi, uphi, vphi, wphi as [ns, n_keep] host arrays, plus count"""
        self._need_active()
        h = self.prof.view(self.ns, NMOM, self.n_keep).cpu().numpy()
        out = {n: h[:, k].copy() for k, n in enumerate(PROFILE_NAMES)}
        out["count"] = self.sample_count
        return out

    def monitor(self):
        """the plane means of the fields as they are (phi, phiphi, uphi, vphi, wphi: [ns, n_keep]), phi_min and phi_max ([ns],
        over all ranks) and -- where profile_dir runs between two walls whose values are set and is whole on this rank --
        nu_lo, nu_hi, nu_vol ([ns], NaN for a species without both wall values; see the module docstring).  ONE host wait
        (and on several ranks two collectives: every rank calls it)."""
        if self.cfg.profile_dir is None:
            raise X3dError("Scalars.monitor needs ScalarsConfig(profile_dir=2 or 3)")
        s, m = self.solver, self.solver.mesh
        self._sample()
        means = self.sums.view(self.ns, NMOM, self.n_keep).cpu().numpy().astype(np.float64) / self.plane_points
        mm = self.minmax.view(self.ns, 2).cpu().numpy().astype(np.float64)
        comm = s.backend.comm
        if comm.size > 1:
            t = torch.from_numpy(np.stack([-mm[:, 0], mm[:, 1]]).copy())
            comm.allreduce_tensor(t, "max")
            mm = np.stack([-t.numpy()[0], t.numpy()[1]], axis=1)
        out = {n: means[:, k].copy() for k, n in enumerate(PROFILE_NAMES)}
        out["phi_min"], out["phi_max"] = mm[:, 0].copy(), mm[:, 1].copy()
        d = self.cfg.profile_dir - 1
        if not m.periodic_BC[d] and int(m.nproc_dir[d]) == 1:
            c = np.asarray(m.vert_coords[d], dtype=np.float64)
            norm = math.sqrt(sum(x * x for x in self.up))
            nus = np.full((3, self.ns), np.nan)
            for i in range(self.ns):
                lo, hi = self.walls[i][d]
                if lo is None or hi is None or lo == hi or norm == 0.0:
                    continue
                q = sum(self.up[k] * means[i, 2 + k] for k in range(3)) / norm
                nus[:, i] = nusselt(c, means[i, 0], q, s.nu_species[i], lo - hi)
            out["nu_lo"], out["nu_hi"], out["nu_vol"] = nus[0], nus[1], nus[2]
        return out

    # ------------------------------------------------------------ output, restart
    def write(self, it):
        """`<prefix>_<it:06d>.npz` (one file per rank on a decomposed mesh: `..._r<rank>.npz`) when istatout divides `it`;
        returns the file name or None"""
        if not self.cfg.output_due(it):
            return None
        mesh = self.solver.mesh
        name = "%s_%06d%s.npz" % (self.cfg.prefix, it, "" if mesh.nproc == 1 else "_r%d" % mesh.nrank)
        out = self.profiles()
        out["sample_count"] = np.array(out.pop("count"))
        np.savez(name, **out)
        return name

    def state_dict(self):
        """what a restarted run needs to continue its means exactly (through the host, like the profile-mode statistics)"""
        self._need_active()
        return {"scalars_sample_count": np.array(self.sample_count), "scalars_profile_dir": np.array(self.cfg.profile_dir),
                "scalars_prof": self.prof.view(self.ns, NMOM, self.n_keep).cpu().numpy()}

    def check_state_dict(self, state):
        if "scalars_sample_count" not in state or "scalars_prof" not in state:
            raise X3dError("restore: this run samples scalar profiles, the checkpoint holds none")
        if int(state["scalars_profile_dir"]) != int(self.cfg.profile_dir):
            raise X3dError("restore: scalars_profile_dir differs: the checkpoint has %d, this run %d"
                           % (int(state["scalars_profile_dir"]), int(self.cfg.profile_dir)))
        shape = tuple(np.asarray(state["scalars_prof"]).shape)
        if shape != (self.ns, NMOM, self.n_keep):
            raise X3dError("restore: scalars_prof differs: the checkpoint has %s, this run %s"
                           % (shape, (self.ns, NMOM, self.n_keep)))

    def load_state_dict(self, state):
        self._need_active()
        self.check_state_dict(state)
        a = np.ascontiguousarray(np.asarray(state["scalars_prof"]), dtype=_lib.NP_REAL)
        self.prof.copy_(torch.from_numpy(a.reshape(-1)))
        self.sample_count = int(state["scalars_sample_count"])
