"""Reynolds-stress budget profiles with the reduction on the device (csrc/budget.hip).  Not in the reference: this
project's own addition, like StatsConfig.profile_dir and the spectra.

A sample is: the nine velocity gradients on the x-fastest blocks (Solver.velocity_gradients), with pressure=True the vertex
pressure (Solver.pressure_vert, scaled by 1 / dt as the snapshots scale it), ONE reduction over the thirteen blocks that
leaves the plane sums of 41 raw moments along profile_dir (HipBackend.budget_profile_sums) and the running-mean recurrence
on 41 x n doubles (HipBackend.budget_profile_accumulate).  No call of a sample waits for the host.  A sample holds eleven
transient pool blocks (nine without pressure; about 11.3 GiB at 512^3 in FP64); their release is stream-ordered.  Sums
and running means are float64 in both flavours of the library: the central moments below are differences of raw ones.

Several ranks: every rank writes its rows into a [41, n_global] buffer, one all-reduce, and -- unlike Stats -- EVERY rank
keeps the global running profile: the write-time derivatives need the whole line.  The root rank writes the file.

Raw moments (MOMENT_NAMES; d = profile_dir - 1, n = the kept direction, pairs in the order uu, vv, ww, uv, uw, vw):
    umean vmean wmean | pmean | uumean .. vwmean | ppmean | pumean pvmean pwmean | uunmean .. vwnmean  (<u_i u_j u_d>)
    dudxmean dudymean dudzmean dvdxmean .. dwdzmean  (<g_ij>, g_ij = d u_i / d x_j)
    gguumean .. ggvwmean  (<sum_k g_ik g_jk>) | psuumean .. psvwmean  (<p (g_ij + g_ji)>)

Write-time algebra (derive; upper case = mean, D = ddn, the derivative along the kept direction):
    R_ij = <u_i u_j> - U_i U_j          T_ij = <u_i u_j u_d> - U_i <u_j u_d> - U_j <u_i u_d> - U_d <u_i u_j> + 2 U_i U_j U_d
    q_i = <p u_i> - P U_i               p_rms = sqrt(max(0, <pp> - P^2))
    production_ij = -(R_id G_jd + R_jd G_id)                    dissipation_ij = 2 nu (<sum_k g_ik g_jk> - sum_k G_ik G_jk)
    pressure_strain_ij = <p (g_ij + g_ji)> - P (G_ij + G_ji)    convection_ij = -U_d D R_ij
    turbulent_transport_ij = -D T_ij                            pressure_diffusion_ij = -D (q_i delta_jd + q_j delta_id)
    viscous_diffusion_ij = nu D D R_ij
    residual_ij = production + convection + turbulent_transport + pressure_diffusion + pressure_strain + viscous_diffusion
                  - dissipation
and the same eight for k = 1/2 R_ii as half-traces (`..._k`).  A budget that closes (residual -> 0) needs a long
stationary run.

Output: `<prefix>_<it:06d>.npz` (load_budgets reads it back), root rank only."""
import numpy as np
import torch

from .common import DIR_X, VERT, X3dError, sample_due
from .diagnostics import global_vert_coords

NMOM = 41
COMP = ("u", "v", "w")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
PAIR_NAMES = tuple(COMP[i] + COMP[j] for i, j in PAIRS)
GRAD_NAMES = tuple("d%sd%s" % (c, x) for c in COMP for x in "xyz")
MOMENT_NAMES = (("umean", "vmean", "wmean", "pmean") + tuple(n + "mean" for n in PAIR_NAMES) + ("ppmean",)
                + tuple("p%smean" % c for c in COMP) + tuple(n + "nmean" for n in PAIR_NAMES)
                + tuple(n + "mean" for n in GRAD_NAMES) + tuple("gg%smean" % n for n in PAIR_NAMES)
                + tuple("ps%smean" % n for n in PAIR_NAMES))
PRESSURE_MOMENTS = (3,) + tuple(range(10, 14)) + tuple(range(35, 41))
TERMS = ("production", "convection", "turbulent_transport", "pressure_diffusion", "pressure_strain", "viscous_diffusion",
         "dissipation", "residual")
PRESSURE_TERMS = ("pressure_diffusion", "pressure_strain")


class BudgetsConfig:
    """when to sample (as StatsConfig: from iteration initbud on, every ibudfreq iterations; initbud <= 0: never), when to
    write (every ibudout iterations; 0: never), along which direction (2 or 3) and whether the pressure terms are formed"""

    def __init__(self, initbud=0, ibudfreq=1, ibudout=0, prefix="budgets", profile_dir=2, pressure=True):
        self.initbud, self.ibudfreq, self.ibudout = int(initbud), int(ibudfreq), int(ibudout)
        if self.ibudfreq < 1:
            raise X3dError("BudgetsConfig: ibudfreq must be at least 1")
        if self.ibudout < 0:
            raise X3dError("BudgetsConfig: ibudout must not be negative")
        self.prefix = str(prefix)
        if profile_dir == 1:
            raise X3dError("BudgetsConfig: profile_dir = 1 is not built (2 or 3)")
        if profile_dir not in (2, 3):
            raise X3dError("BudgetsConfig: profile_dir must be 2 or 3")
        self.profile_dir = int(profile_dir)
        self.pressure = bool(pressure)

    @property
    def active(self):
        return self.initbud > 0

    def sample_due(self, it):
        return sample_due(it, self.initbud, self.ibudfreq)

    def output_due(self, it):
        return self.active and self.ibudout > 0 and it % self.ibudout == 0


# ---------------------------------------------------------------- host side: the write-time algebra, file, state
def ddn(f, coords, periodic=False, length=None):
    """the derivative of a profile along its own direction.  Non-periodic: np.gradient(f, coords, edge_order=2) on the
    GLOBAL vertex coordinates (second order on a stretched line, one-sided at the two ends).  Periodic: centred
    differences (f[j+1] - f[j-1]) / (x[j+1] - x[j-1]) wrapped around `length`.  The transport terms of derive are such
    second-order differences of profiles; everything else carries the solver's own compact operators."""
    f, x = np.asarray(f, dtype=np.float64), np.asarray(coords, dtype=np.float64)
    if f.shape != x.shape or f.ndim != 1 or f.size < 3:
        raise X3dError("ddn: a profile and its coordinates are 1-D arrays of one length, at least 3")
    if not periodic:
        return np.gradient(f, x, edge_order=2)
    if length is None:
        raise X3dError("ddn: a periodic direction needs its length")
    xm = np.concatenate([[x[-1] - float(length)], x[:-1]])
    xp = np.concatenate([x[1:], [x[0] + float(length)]])
    return (np.roll(f, -1) - np.roll(f, 1)) / (xp - xm)


def _pair(i, j):
    return PAIRS.index((min(i, j), max(i, j)))


def derive(m, coords, nu, periodic, length, d, pressure=True):
    """the budget terms (module docstring) from the raw running means `m` (MOMENT_NAMES -> profiles) along direction d
    (0-based: 1 = y, 2 = z): a pure host function in float64.  The mean gradient G_ij comes from the compact operator
    through the accumulated moment, not from differencing U; convection, the three transport terms and the viscous
    diffusion are second-order differences of profiles (ddn).  pressure=False: pressure_diffusion, pressure_strain, q_*
    and p_rms are absent, from the dict and from the residual."""
    if d not in (1, 2):
        raise X3dError("derive: d must be 1 (y) or 2 (z)")
    a = [np.asarray(m[n], dtype=np.float64) for n in MOMENT_NAMES]
    U, P = a[0:3], a[3]
    uu = lambda i, j: a[4 + _pair(i, j)]
    uud = lambda i, j: a[14 + _pair(i, j)]
    G = lambda i, j: a[20 + 3 * i + j]
    D = lambda f: ddn(f, coords, periodic, length)
    nu = float(nu)
    out = {}
    R = {}
    for k, (i, j) in enumerate(PAIRS):
        R[k] = uu(i, j) - U[i] * U[j]
    q = [a[11 + i] - P * U[i] for i in range(3)]
    for k, (i, j) in enumerate(PAIRS):
        name = PAIR_NAMES[k]
        T = uud(i, j) - U[i] * uu(j, d) - U[j] * uu(i, d) - U[d] * uu(i, j) + 2.0 * U[i] * U[j] * U[d]
        out["R_" + name], out["T_" + name] = R[k], T
        t = {}
        t["production"] = -(R[_pair(i, d)] * G(j, d) + R[_pair(j, d)] * G(i, d))
        t["dissipation"] = 2.0 * nu * (a[29 + k] - (G(i, 0) * G(j, 0) + G(i, 1) * G(j, 1) + G(i, 2) * G(j, 2)))
        t["convection"] = -U[d] * D(R[k])
        t["turbulent_transport"] = -D(T)
        t["viscous_diffusion"] = nu * D(D(R[k]))
        if pressure:
            t["pressure_strain"] = a[35 + k] - P * (G(i, j) + G(j, i))
            t["pressure_diffusion"] = -D(q[i] * (1.0 if j == d else 0.0) + q[j] * (1.0 if i == d else 0.0))
        t["residual"] = _residual(t, pressure)
        for term, v in t.items():
            out["%s_%s" % (term, name)] = v
    out["R_k"] = 0.5 * (R[0] + R[1] + R[2])
    for term in TERMS:
        if term in PRESSURE_TERMS and not pressure:
            continue
        out[term + "_k"] = 0.5 * (out[term + "_uu"] + out[term + "_vv"] + out[term + "_ww"])
    if pressure:
        for i, c in enumerate(COMP):
            out["q_" + c] = q[i]
        out["p_rms"] = np.sqrt(np.maximum(0.0, a[10] - P * P))
    return out


def _residual(t, pressure):
    r = t["production"] + t["convection"] + t["turbulent_transport"]
    if pressure:
        r = r + t["pressure_diffusion"] + t["pressure_strain"]
    return r + t["viscous_diffusion"] - t["dissipation"]


def file_name(prefix, it):
    return "%s_%06d.npz" % (prefix, int(it))


def save_budgets(prefix, it, profile_dir, pressure, coord, sample_count, moments, terms):
    """`<prefix>_<it:06d>.npz`: coord, sample_count, iteration, profile_dir, pressure, the 41 raw moments and the derived
    terms under their names; returns the file name"""
    payload = {"coord": np.asarray(coord, dtype=np.float64), "sample_count": np.array(int(sample_count)),
               "iteration": np.array(int(it)), "profile_dir": np.array(int(profile_dir)), "pressure": np.array(bool(pressure))}
    payload.update(moments)
    payload.update(terms)
    name = file_name(prefix, it)
    np.savez(name, **payload)
    return name


def load_budgets(prefix, it):
    """what write(it) wrote: {"coord", "sample_count", "iteration", "profile_dir", "pressure", "moments": {...},
    "budgets": {...}} with the two dicts as moments() and budgets() return them"""
    with np.load(file_name(prefix, it), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    out = {"coord": d.pop("coord"), "sample_count": int(d.pop("sample_count")), "iteration": int(d.pop("iteration")),
           "profile_dir": int(d.pop("profile_dir")), "pressure": bool(d.pop("pressure"))}
    out["moments"] = {n: d.pop(n) for n in MOMENT_NAMES}
    out["budgets"] = d
    return out


def state_from_moments(profile_dir, pressure, sample_count, moments):
    """the checkpoint variables: budgets_sample_count, budgets_profile_dir, budgets_pressure and the 41 running means under
    `budgets_<name>`"""
    out = {"budgets_sample_count": np.array(int(sample_count)), "budgets_profile_dir": np.array(int(profile_dir)),
           "budgets_pressure": np.array(bool(pressure))}
    for n in MOMENT_NAMES:
        out["budgets_" + n] = np.asarray(moments[n], dtype=np.float64)
    return out


def moments_from_state(state, profile_dir, pressure, n_keep=None):
    """the inverse: (sample_count, [41, n] float64); the state must have been taken along the same direction with the same
    pressure setting"""
    if "budgets_sample_count" not in state:
        raise X3dError("budgets: this run samples budgets, the state holds none")
    if int(state["budgets_profile_dir"]) != int(profile_dir):
        raise X3dError("budgets: the state was taken along profile_dir = %d, this run samples %d"
                       % (int(state["budgets_profile_dir"]), int(profile_dir)))
    if bool(state["budgets_pressure"]) != bool(pressure):
        raise X3dError("budgets: the state was taken with pressure = %s, this run samples with pressure = %s"
                       % (bool(state["budgets_pressure"]), bool(pressure)))
    raw = np.ascontiguousarray(np.stack([np.asarray(state["budgets_" + n], dtype=np.float64).reshape(-1)
                                         for n in MOMENT_NAMES]))
    if n_keep is not None and raw.shape != (NMOM, int(n_keep)):
        raise X3dError("budgets: the state holds profiles of %d values, this run %d" % (raw.shape[1], int(n_keep)))
    return int(state["budgets_sample_count"]), raw


# ---------------------------------------------------------------- the device object
class Budgets:
    """owns the running profile and sample_count; BaseCase.run calls update(it) and write(it) when the case has one
    (case.budgets = Budgets(case.solver, cfg))"""

    def __init__(self, solver, cfg):
        self.solver, self.cfg = solver, cfg
        self.sample_count = 0
        self.files = []
        self.prof = self.sums = self._global = None
        b, m = solver.backend, solver.mesh
        d = self.d = cfg.profile_dir - 1
        self.n_keep = int(m.get_dims(VERT)[d])
        self.n_keep_global = int(m.get_global_dims(VERT)[d])
        self.keep_offset = int(m.n_offset[d])
        self.plane_points = int(np.prod([n for i, n in enumerate(m.get_global_dims(VERT)) if i != d]))
        self.periodic, self.length = bool(m.periodic_BC[d]), float(m.L[d])
        self.coords = global_vert_coords(m, d)[:self.n_keep_global].copy()
        if not cfg.active:
            return  # (like Stats: an inactive object owns nothing and asks nothing of the solver)
        if cfg.pressure:
            solver.keep_pressure = True
        z = lambda n: torch.zeros(n, dtype=torch.float64, device=b.device)
        self.prof, self.sums = z(NMOM * self.n_keep_global), z(NMOM * self.n_keep)
        if b.comm.size > 1:
            self._global = z(NMOM * self.n_keep_global)

    def _need_active(self):
        if not self.cfg.active:
            raise X3dError("budgets are inactive (initbud <= 0)")

    # ------------------------------------------------------------ sampling
    def reads_state(self, it):
        """does update(it) read the solver's fields?  (BaseCase.run then completes the step first)"""
        return self.cfg.sample_due(it)

    def pressure_due(self, it):
        """does update(it) read the pressure of iteration `it`?  (BaseCase.run then keeps it)"""
        return self.cfg.pressure and self.reads_state(it)

    def sample(self, u, v, w, p, grads, p_scale=1.0):
        """one sample from fields of the caller's: the sums launch, on several ranks the all-reduce, the recurrence"""
        self._need_active()
        b = self.solver.backend
        b.budget_profile_sums(u, v, w, p, grads, self.cfg.profile_dir, p_scale, self.sums)
        sums = self.sums
        if self._global is not None:
            g = self._global.view(NMOM, self.n_keep_global)
            g.zero_()
            lo = self.keep_offset
            g[:, lo:lo + self.n_keep] = self.sums.view(NMOM, self.n_keep)
            b.comm.allreduce_tensor(self._global)
            sums = self._global
        self.sample_count += 1
        b.budget_profile_accumulate(self.prof, sums, 1.0 / self.plane_points, 1.0 / self.sample_count)

    def update(self, it):
        """one sample if iteration `it` is due; returns whether one was taken.  No host wait."""
        if not self.reads_state(it):
            return False
        s = self.solver
        al = s.backend.allocator
        s.flush_grad()  # a velocity correction left pending by step(more=True) is not in u, v, w yet
        taken = s.velocity_gradients()
        p = None
        if self.cfg.pressure:
            taken += [al.get_block(DIR_X, VERT), al.get_block(DIR_X, VERT)]
            p = s.pressure_vert(*taken[-2:])
        self.sample(s.u, s.v, s.w, p, taken[:9], 1.0 / s.dt)
        for f in taken:  # (stream-ordered: whoever takes them next writes behind the reduction)
            al.release_block(f)
        return True

    # ------------------------------------------------------------ results (host arrays, float64)
    def moments(self):
        """the 41 raw running means under MOMENT_NAMES: profiles of the global length along profile_dir"""
        self._need_active()
        return dict(zip(MOMENT_NAMES, self.prof.view(NMOM, self.n_keep_global).cpu().numpy()))

    def budgets(self):
        """derive(...) of the current means"""
        return derive(self.moments(), self.coords, float(self.solver.nu), self.periodic, self.length, self.d,
                      self.cfg.pressure)

    # ------------------------------------------------------------ output, restart
    def write(self, it):
        """`<prefix>_<it:06d>.npz` when ibudout divides `it` (root rank only); returns the file name or None"""
        if not self.cfg.output_due(it) or not self.solver.mesh.is_root():
            return None
        name = save_budgets(self.cfg.prefix, it, self.cfg.profile_dir, self.cfg.pressure, self.coords, self.sample_count,
                            self.moments(), self.budgets())
        self.files.append(name)
        return name

    def state_dict(self):
        """what a restarted run needs: the sample count and the running means (41 x n doubles, through the host)"""
        return state_from_moments(self.cfg.profile_dir, self.cfg.pressure, self.sample_count, self.moments())

    def load_state_dict(self, state):
        self._need_active()
        count, raw = moments_from_state(state, self.cfg.profile_dir, self.cfg.pressure, self.n_keep_global)
        self.prof.copy_(torch.from_numpy(raw.reshape(-1)))
        self.sample_count = count
