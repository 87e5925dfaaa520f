"""Flow statistics: mirror of stats_manager_t (src/io/stats.f90) with the accumulators on the device.

The reference copies u, v, w to the host at every sample (:139-141) and updates nine host arrays (:151-159).  Here a
sample is one kernel over u, v, w and nine accumulator blocks (HipBackend.stats_update_uvw, csrc/stats.hip), plus one
per species; nothing leaves the device until means() / fluctuations() / write() ask for it.

profile_dir (not in the reference): keep only profiles along one direction -- means over the two others, what a
channel run plots along y.  A sample then reads u, v, w once and updates 9 * n values; no 3-D accumulator exists.  On a
decomposed mesh the plane sums are added over all ranks before they enter the running mean; a rank holds the rows of
the kept direction that it owns.

Output: the reference writes ADIOS2 (.bp) files; ADIOS2 is not a dependency of this project, so write() produces
`<prefix>_<it:06d>.npz` with the same variable names (one file per rank on a decomposed mesh: `..._r<rank>.npz`)."""
import numpy as np
import torch

from . import _lib
from .common import DIR_X, VERT, X3dError, sample_due

# accumulator names in moment order (src/io/stats.f90:34-43, 151-159)
MEAN_NAMES = ("umean", "vmean", "wmean", "uumean", "vvmean", "wwmean", "uvmean", "uwmean", "vwmean")
# what write_stats derives at output time (:232-237, 252-263): the last three names then mean <u'v'>, <u'w'>, <v'w'>
FLUCT_NAMES = ("uprime", "vprime", "wprime", "uvmean", "uwmean", "vwmean")


class StatsConfig:
    """stats_params of the reference (initstat, istatfreq, istatout, stats_prefix) plus profile_dir: None = 3-D
    accumulators as in the reference; 1, 2 or 3 = profiles along that direction only"""

    def __init__(self, initstat=0, istatfreq=1, istatout=0, stats_prefix="statistics", profile_dir=None):
        self.initstat, self.istatfreq, self.istatout = int(initstat), int(istatfreq), int(istatout)
        self.stats_prefix = str(stats_prefix)
        if profile_dir not in (None, 1, 2, 3):
            raise X3dError("StatsConfig: profile_dir must be None, 1, 2 or 3")
        if self.istatfreq < 1:
            raise X3dError("StatsConfig: istatfreq must be at least 1")
        self.profile_dir = profile_dir

    @property
    def active(self):
        return self.initstat > 0  # src/io/stats.f90:83

    def sample_due(self, it):
        """src/io/stats.f90:129-131"""
        return sample_due(it, self.initstat, self.istatfreq)

    def output_due(self, it):
        """src/io/stats.f90:211-213"""
        return self.active and self.istatout > 0 and it % self.istatout == 0


def derive_host(m):
    """the write-time formulas (src/io/stats.f90:232-237) on host arrays: used for the profiles, which are a few KB"""
    out = {}
    for k, c in enumerate("uvw"):
        out[c + "prime"] = np.sqrt(np.maximum(0.0, m[MEAN_NAMES[3 + k]] - m[MEAN_NAMES[k]] ** 2))
    out["uvmean"] = m["uvmean"] - m["umean"] * m["vmean"]
    out["uwmean"] = m["uwmean"] - m["umean"] * m["wmean"]
    out["vwmean"] = m["vwmean"] - m["vmean"] * m["wmean"]
    return out


class Stats:
    """owns the accumulators and sample_count; BaseCase.run calls update(it) and write(it) when the case has one
    (case.stats = Stats(case.solver, cfg))"""

    def __init__(self, solver, cfg):
        self.solver, self.cfg = solver, cfg
        self.sample_count = 0
        self.nspecies = len(solver.species)
        b = solver.backend
        self.means3d, self.phi3d = [], []
        self.prof = self.sums = self.phi_prof = None
        if not cfg.active:
            return
        if cfg.profile_dir is None:
            self.means3d = [self._zero_block() for _ in MEAN_NAMES]
            self.phi3d = [(self._zero_block(), self._zero_block()) for _ in range(self.nspecies)]
        else:
            m = solver.mesh
            d = cfg.profile_dir - 1
            self.n_keep = int(m.get_dims(VERT)[d])
            self.n_keep_global = int(m.get_global_dims(VERT)[d])
            self.keep_offset = int(m.n_offset[d])
            self.plane_points = int(np.prod([n for i, n in enumerate(m.get_global_dims(VERT)) if i != d]))
            z = lambda n: torch.zeros(n, dtype=_lib.torch_real(), device=b.device)
            self.prof, self.sums = z(9 * self.n_keep), z(9 * self.n_keep)
            self.phi_prof = [z(9 * self.n_keep) for _ in range(self.nspecies)]
            self._global = z(9 * self.n_keep_global) if b.comm.size > 1 else None

    def _zero_block(self):
        f = self.solver.backend.allocator.get_block(DIR_X, VERT)
        f.fill(0.0)
        return f

    # ------------------------------------------------------------ sampling
    def reads_state(self, it):
        """does update(it) read the solver's fields?  (BaseCase.run then completes the step first)"""
        return self.cfg.sample_due(it)

    def update(self, it):
        """one sample if iteration `it` is due (src/io/stats.f90:118-187); returns whether one was taken"""
        if not self.reads_state(it):
            return False
        s = self.solver
        b = s.backend
        s.flush_grad()  # a velocity correction left pending by step(more=True) is not in u, v, w yet
        self.sample_count += 1
        inc = 1.0 / self.sample_count
        if self.cfg.profile_dir is None:
            b.stats_update_uvw(s.u, s.v, s.w, self.means3d, inc)
            for phi, (m1, m2) in zip(s.species, self.phi3d):
                b.stats_update_scalar(phi, m1, m2, inc)
        else:
            self._profile_sample(s.u, s.v, s.w, self.prof, inc)
            for phi, p in zip(s.species, self.phi_prof):
                # (phi three times: moment 0 is the sum of phi, moment 3 that of phi^2)
                self._profile_sample(phi, phi, phi, p, inc)
        return True

    def _profile_sample(self, u, v, w, prof, inc):
        b = self.solver.backend
        b.stats_profile_sums(u, v, w, self.cfg.profile_dir, self.sums)
        if self._global is not None:
            # every rank adds its plane sums into the rows it owns of a profile of the global length; the sum over all
            # ranks is then, row by row, the sum over the ranks of the two reduced directions
            g = self._global.view(9, self.n_keep_global)
            g.zero_()
            lo = self.keep_offset
            g[:, lo:lo + self.n_keep] = self.sums.view(9, self.n_keep)
            b.comm.allreduce_tensor(self._global)
            self.sums.view(9, self.n_keep).copy_(g[:, lo:lo + self.n_keep])
        b.stats_profile_accumulate(prof, self.sums, 1.0 / self.plane_points, inc)

    # ------------------------------------------------------------ results (host arrays)
    def _need_active(self):
        if not self.cfg.active:
            raise X3dError("statistics are inactive (initstat <= 0)")

    def means(self):
        """running means under the accumulators' names (umean ... vwmean: plain means of u ... v w; phimean_<i>,
        phiphimean_<i>): [nz, ny, nx] arrays, or profiles along profile_dir"""
        self._need_active()
        b = self.solver.backend
        if self.cfg.profile_dir is not None:
            out = dict(zip(MEAN_NAMES, self._host(self.prof)))
            for i, p in enumerate(self.phi_prof, 1):
                h = self._host(p)
                out["phimean_%d" % i], out["phiphimean_%d" % i] = h[0], h[3]
            return out
        out = {n: b.get_field_data(f) for n, f in zip(MEAN_NAMES, self.means3d)}
        for i, (m1, m2) in enumerate(self.phi3d, 1):
            out["phimean_%d" % i], out["phiphimean_%d" % i] = b.get_field_data(m1), b.get_field_data(m2)
        return out

    def _host(self, t):
        return t.view(9, self.n_keep).cpu().numpy()

    def fluctuations(self):
        """what write_stats derives (src/io/stats.f90:232-237, 281-282): uprime, vprime, wprime, the Reynolds stresses
        under the reference's output names uvmean, uwmean, vwmean, and phiprime_<i>"""
        self._need_active()
        if self.cfg.profile_dir is not None:
            m = self.means()
            out = derive_host(m)
            for i in range(1, self.nspecies + 1):
                out["phiprime_%d" % i] = np.sqrt(np.maximum(0.0, m["phiphimean_%d" % i] - m["phimean_%d" % i] ** 2))
            return out
        b, al = self.solver.backend, self.solver.backend.allocator
        outs = [al.get_block(DIR_X, VERT) for _ in FLUCT_NAMES]
        b.stats_derive(outs, self.means3d)
        out = {n: b.get_field_data(f) for n, f in zip(FLUCT_NAMES, outs)}
        for i, (m1, m2) in enumerate(self.phi3d, 1):
            # (the same kernel: its first output is sqrt(max(0, mean[3] - mean[0]^2)))
            b.stats_derive(outs, [m1] * 3 + [m2] * 6)
            out["phiprime_%d" % i] = b.get_field_data(outs[0])
        for f in outs:
            al.release_block(f)
        return out

    def profiles(self):
        """profile mode: means() and fluctuations() in one dict, the plain second moments under uumean ... vwmean and
        the Reynolds stresses under uv, uw, vw"""
        self._need_active()
        if self.cfg.profile_dir is None:
            raise X3dError("profiles() needs StatsConfig(profile_dir=1, 2 or 3)")
        out = self.means()
        fl = self.fluctuations()
        for n in ("uv", "uw", "vw"):
            out[n] = fl.pop(n + "mean")
        out.update(fl)
        return out

    # ------------------------------------------------------------ output, restart
    def output_arrays(self):
        """the variables of write_stats (src/io/stats.f90:245-288)"""
        m, fl = self.means(), self.fluctuations()
        out = {"sample_count": np.array(self.sample_count)}
        for n in ("umean", "vmean", "wmean"):
            out[n] = m[n]
        for n in FLUCT_NAMES:
            out[n] = fl[n]
        for i in range(1, self.nspecies + 1):
            out["phimean_%d" % i], out["phiprime_%d" % i] = m["phimean_%d" % i], fl["phiprime_%d" % i]
        return out

    def write(self, it):
        """`<prefix>_<it:06d>.npz` when istatout divides `it` (src/io/stats.f90:211-218; .npz instead of ADIOS2's
        .bp, see the module docstring); returns the file name or None"""
        if not self.cfg.output_due(it):
            return None
        mesh = self.solver.mesh
        name = "%s_%06d%s.npz" % (self.cfg.stats_prefix, it, "" if mesh.nproc == 1 else "_r%d" % mesh.nrank)
        np.savez(name, **self.output_arrays())
        return name

    def state_dict(self):
        """the checkpoint variables of write_checkpoint (src/io/stats.f90:315-357): a restarted run continues its means
        exactly"""
        self._need_active()
        out = {"stats_sample_count": np.array(self.sample_count)}
        for n, a in self.means().items():
            out["stats_" + n] = a
        return out

    def load_state_dict(self, state):
        """read_checkpoint (src/io/stats.f90:379-431)"""
        self._need_active()
        b = self.solver.backend
        names = list(MEAN_NAMES)
        for i in range(1, self.nspecies + 1):
            names += ["phimean_%d" % i, "phiphimean_%d" % i]
        arrays = {n: np.asarray(state["stats_" + n]) for n in names}
        if self.cfg.profile_dir is None:
            blocks = list(self.means3d) + [f for pair in self.phi3d for f in pair]
            for n, f in zip(names, blocks):
                b.set_field_data(f, arrays[n], VERT)
        else:
            real = _lib.NP_REAL
            self.prof.copy_(torch.from_numpy(np.stack([arrays[n] for n in MEAN_NAMES]).astype(real).reshape(-1)))
            for i, p in enumerate(self.phi_prof, 1):
                h = np.zeros((9, self.n_keep), dtype=real)
                h[0], h[3] = arrays["phimean_%d" % i], arrays["phiphimean_%d" % i]
                p.copy_(torch.from_numpy(h.reshape(-1)))
        self.sample_count = int(state["stats_sample_count"])
