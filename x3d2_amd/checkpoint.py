"""Checkpoint and restart: mirror of checkpoint_manager_t (src/io/checkpoint_manager.f90, src/io/io_manager.f90,
src/io/checkpoint_state.f90; the checkpoint part of checkpoint_params, src/config.f90:72-85) with the pack, the checksums
and the unpack on the device.

The reference pulls u, v, w (and, through the integrator and the statistics, their own arrays) to the host with one
blocking copy each.  Here `write` completes a pending velocity correction, launches ONE kernel that packs every block of
the state into a dense device buffer and forms three integers per block on the way (HipBackend.checkpoint_pack,
csrc/checkpoint.hip), and starts ONE asynchronous copy of buffer and table into pinned host memory on the copy stream of
the snapshots.  `write` returns without a host wait; `poll` writes the file once the copy has landed, `finalise` waits
for it.  The buffers are a ring of 1 slot (copyring.CopyRing): the 2nd acquire waits, that is, a checkpoint that arrives
before the previous one has been written waits for it.

The state, in this order: u, v, w; phi_<n> per species; for Adams-Bashforth of order > 1 `<name>_rhs_old<j>` for every
variable in the integrator's list order (after its rotations); with active 3-D statistics their accumulators under
Stats.state_dict's names (the profile mode's few KB go through state_dict on the host, and so do the running means of
case.spectra under Spectra.state_dict's `spectra_*` names and the budget profiles of case.budgets under
Budgets.state_dict's `budgets_*` names, and the particles of case.particles under Particles.state_dict's `particles_*` names,
in id order: 12 or 18 doubles and one int per particle).

Scalars.  The reference's: timestep, time, dt, data_loc, ti_is_ab, ti_order, ti_istep, ti_nstep, stats_sample_count.
Added here, because a resumed run must give the bits of the uninterrupted one:
  ti_gdt        CylinderCase.define_BC reads the PREVIOUS sub-step's gdt before the integrator sets the next
  precision     bytes per real: a checkpoint is bits of the working precision, not values to convert
  dims, global_dims, n_offset, nproc_dir     a rank's file only fits the same decomposition
  n_species, ti_sname                        what the block list was built from
  case_<key>    BaseCase.checkpoint_state() (the reference's checkpoint_state_t): the noise generators of the channel
                and the cylinder number their draws (noise_seed, noise_draws)

Checksums, per block, with i the dense index and bits() the element's bit pattern (zero-extended on 4-byte reals):
s1 = sum bits(e_i), s2 = sum bits(e_i) (2 i + 1), both modulo 2^64, and the number of NaN / Inf.  s1 alone does not see
two elements changing places; s2 does.  `restore` forms them again on the device from what it uploaded and compares all
three columns before it writes a single field.  A state with a NaN or Inf is still written -- as
`<prefix>_<it:06d>.nonfinite.npz` -- but never replaces a good checkpoint.

Output: the reference writes ADIOS2 (.bp); here a checkpoint is `<prefix>_<it:06d>.npz` (several ranks:
`<prefix>_<it:06d>.r<rank>.npz`), written as `<prefix>_temp[.r<rank>].npz` and moved into place with os.replace (the
reference's safe-write), holding the variables as [nz, ny, nx] arrays, `names` (their order), `checksums`
(uint64 [len(names), 3]) and the scalars."""
import os

import numpy as np

from . import _lib
from .common import VERT, X3dError
from .copyring import CopyRing

REAL_BYTES = np.dtype(_lib.NP_REAL).itemsize


class CheckpointConfig:
    """the checkpoint part of checkpoint_params (src/config.f90:72-85), the reference's names and defaults"""

    def __init__(self, checkpoint_freq=0, checkpoint_prefix="checkpoint", keep_checkpoint=True,
                 restart_from_checkpoint=False, restart_file=""):
        self.checkpoint_freq = int(checkpoint_freq)
        self.checkpoint_prefix = str(checkpoint_prefix)
        self.keep_checkpoint = bool(keep_checkpoint)
        self.restart_from_checkpoint = bool(restart_from_checkpoint)
        self.restart_file = str(restart_file)

    def due(self, it):
        """src/io/checkpoint_manager.f90 (handle_checkpoint_step): checkpoint_freq > 0 and it a multiple of it"""
        if self.checkpoint_freq <= 0:
            return False
        return it % self.checkpoint_freq == 0


def file_name(prefix, it, nproc=1, nrank=0, tag=""):
    """`<prefix>_<it:06d>[.nonfinite][.r<rank>].npz`; it = "temp": the name a file is written under before it is moved"""
    mid = "temp" if it == "temp" else "%06d" % int(it)
    return "%s_%s%s%s.npz" % (prefix, mid, tag, "" if int(nproc) == 1 else ".r%d" % int(nrank))


def checksum_rows(a):
    """(s1, s2, nonfinite) of one array in dense order, on the host: what x3d_checkpoint_pack forms on the device"""
    a = np.ascontiguousarray(a).reshape(-1)
    bits = a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)
    i = np.arange(bits.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        s1 = np.add.reduce(bits, dtype=np.uint64)
        s2 = np.add.reduce(bits * (np.uint64(2) * i + np.uint64(1)), dtype=np.uint64)
    return np.array([s1, s2, np.count_nonzero(~np.isfinite(a))], dtype=np.uint64)


def state_fields(solver, stats=None):
    """[(name, field)] of everything a checkpoint holds as blocks, in the order of the module docstring"""
    ti = solver.time_integrator
    names = ["u", "v", "w"] + ["phi_%d" % i for i in range(1, len(solver.species) + 1)]
    out = list(zip(names, [solver.u, solver.v, solver.w] + list(solver.species)))
    if ti.sname[:2] == "AB" and ti.order > 1:
        for name, row in zip(names, ti.olds):
            out += [("%s_rhs_old%d" % (name, j), f) for j, f in enumerate(row, 1)]
    if stats is not None and stats.cfg.active and stats.cfg.profile_dir is None:
        from .stats import MEAN_NAMES
        out += [("stats_" + n, f) for n, f in zip(MEAN_NAMES, stats.means3d)]
        for i, (m1, m2) in enumerate(stats.phi3d, 1):
            out += [("stats_phimean_%d" % i, m1), ("stats_phiphimean_%d" % i, m2)]
    return out


class Checkpoints:
    """Checkpoints(solver, cfg, case=None), attached as `case.checkpoints = Checkpoints(case.solver, cfg, case)`:
    BaseCase.run then calls write(it) and poll() once per step and finalise() before it returns."""

    def __init__(self, solver, cfg, case=None):
        self.solver, self.cfg, self.case = solver, cfg, case
        self.ring = CopyRing(solver.backend, 1, self._write_file)  # (an attached but idle Checkpoints takes nothing)
        self.files = []        # names of the files written so far, .nonfinite ones included
        self.last_good = None  # the newest finite checkpoint on disk

    @property
    def stats(self):
        return getattr(self.case, "stats", None) if self.case is not None else None

    @property
    def spectra(self):
        return getattr(self.case, "spectra", None) if self.case is not None else None

    @property
    def budgets(self):
        return getattr(self.case, "budgets", None) if self.case is not None else None

    @property
    def particles(self):
        return getattr(self.case, "particles", None) if self.case is not None else None

    def _file_name(self, it, tag=""):
        m = self.solver.mesh
        return file_name(self.cfg.checkpoint_prefix, it, m.nproc, m.nrank, tag)

    # ------------------------------------------------------------ taking a checkpoint
    def scalars(self, it):
        """everything of a checkpoint that is not a block, as numpy values (see the module docstring)"""
        s, m = self.solver, self.solver.mesh
        ti = s.time_integrator
        out = {"timestep": np.int64(it), "time": np.float64(it * s.dt), "dt": np.float64(s.dt),
               "data_loc": np.int64(s.u.data_loc), "ti_is_ab": np.bool_(ti.sname[:2] == "AB"),
               "ti_order": np.int64(ti.order), "ti_istep": np.int64(ti.istep), "ti_nstep": np.int64(ti.nstep),
               "ti_istage": np.int64(ti.istage), "ti_gdt": np.float64(ti.gdt), "ti_sname": np.array(str(ti.sname)),
               "precision": np.int64(REAL_BYTES), "n_species": np.int64(len(s.species)),
               "dims": np.array(m.get_dims(VERT), dtype=np.int64),
               "global_dims": np.array(m.get_global_dims(VERT), dtype=np.int64),
               "n_offset": np.array(m.n_offset, dtype=np.int64), "nproc_dir": np.array(m.nproc_dir, dtype=np.int64),
               "stats_sample_count": np.int64(0)}
        st = self.stats
        if st is not None and st.cfg.active:
            out["stats_sample_count"] = np.int64(st.sample_count)
            if st.cfg.profile_dir is not None:  # the profiles: a few KB, through the host
                out.update(st.state_dict())
            out["stats_profile_dir"] = np.int64(st.cfg.profile_dir or 0)
        sp = self.spectra
        if sp is not None and sp.cfg.active:  # the running means of the spectra: a few KB to a few MB, through the host
            out.update(sp.state_dict())
        bud = self.budgets
        if bud is not None and bud.cfg.active:  # the running budget profiles: 41 x n doubles, through the host
            out.update(bud.state_dict())
        parts = self.particles
        if parts is not None:  # the particle state: through the host in id order (one host wait)
            out.update(parts.state_dict())
        sca = getattr(s, "scalars", None)
        if sca is not None and sca.profiling:  # the running scalar profiles: 5 x n values per species, through the host
            out.update(sca.state_dict())
        if self.case is not None:
            for k, v in self.case.checkpoint_state().items():
                out["case_" + k] = np.asarray(v)
        return out

    def reads_state(self, it):
        """does write(it) read the solver's fields?  (BaseCase.run then completes the step first)"""
        return self.cfg.due(it)

    def write(self, it):
        """if iteration `it` is due: flush_grad, one pack launch, one asynchronous copy; returns whether a checkpoint
        was taken.  No host wait unless the previous checkpoint is still unwritten."""
        if not self.reads_state(it):
            return False
        s = self.solver
        b = s.backend
        s.flush_grad()  # a velocity correction left pending by step(more=True) is not in u, v, w yet
        fields = state_fields(s, self.stats)
        if len(fields) > b.CKPT_MAXBLOCK:
            raise X3dError("Checkpoints: the state has %d blocks, a checkpoint holds at most %d"
                           % (len(fields), b.CKPT_MAXBLOCK))
        dims = tuple(int(n) for n in s.mesh.get_dims(VERT))
        _, _, total = b.checkpoint_layout(len(fields), int(np.prod(dims)))
        slot = self.ring.acquire(total)  # (the second checkpoint before the first was written waits here)
        scalars = self.scalars(it)  # (now: the file is written later, the run goes on in between)
        n = b.checkpoint_pack([f for _, f in fields], dims, slot.dev)
        self.ring.submit(slot, n, (int(it), [k for k, _ in fields], scalars, dims))
        return True

    # ------------------------------------------------------------ writing
    def _write_file(self, payload, raw):
        """the ring's landing: the file of what write() packed, from the landed bytes"""
        it, names, scalars, dims = payload
        b = self.solver.backend
        n = int(np.prod(dims))
        data, off, total = b.checkpoint_layout(len(names), n)
        arrays = raw[:data].view(_lib.NP_REAL).reshape(len(names), dims[2], dims[1], dims[0])
        table = raw[off:total].view(np.uint64).reshape(len(names), 3)
        payload = {name: arrays[k] for k, name in enumerate(names)}
        payload.update(scalars)
        payload["names"] = np.array(names)
        payload["checksums"] = table.copy()
        return self.save(it, payload, bool(np.any(table[:, 2] > 0)))

    def save(self, it, payload, nonfinite):
        """the safe write: `<prefix>_temp...npz`, then os.replace.  A finite checkpoint becomes last_good and, with
        keep_checkpoint = False, removes its predecessor once it is in place; one with a NaN / Inf is named
        `.nonfinite` and removes nothing."""
        temp = self._file_name("temp")
        with open(temp, "wb") as fh:  # (a file object: np.savez would append .npz to a name of its own choosing)
            np.savez(fh, **payload)
        name = self._file_name(it, ".nonfinite" if nonfinite else "")
        os.replace(temp, name)
        self.files.append(name)
        if not nonfinite:
            prev, self.last_good = self.last_good, name
            if not self.cfg.keep_checkpoint and prev is not None and prev != name and os.path.exists(prev):
                os.remove(prev)
        return name

    def poll(self):
        """write the checkpoint whose copy has landed; never blocks.  Returns the files written."""
        return self.ring.poll()

    def finalise(self):
        """wait for and write what is left"""
        return self.ring.drain()


# ---------------------------------------------------------------- restart
def _differs(what, stored, here):
    return X3dError("restore: %s differs: the checkpoint has %s, this run %s" % (what, stored, here))


def read_checkpoint(path):
    """the file as a dict of arrays; an unreadable (truncated, damaged) file is an X3dError that names it"""
    try:
        with np.load(path, allow_pickle=False) as z:
            out = {k: z[k] for k in z.files}
    except X3dError:
        raise
    except Exception as e:  # (zipfile.BadZipFile, EOFError, ValueError, OSError: whatever the damage makes of it)
        raise X3dError("restore: cannot read the checkpoint %s: %s: %s" % (path, type(e).__name__, e))
    for k in ("names", "checksums", "timestep", "precision", "dims"):
        if k not in out:
            raise X3dError("restore: %s is not a checkpoint: no `%s`" % (path, k))
    return out


def restore(case, path):
    """continue `case` (made as for a new run, statistics and all attached) from the checkpoint file `path`: read,
    check that it fits this run, upload, form the checksums on the device and compare them with the file's, unpack.
    Every check raises an X3dError that names what differs BEFORE any field of the solver is written.
    BaseCase.run then continues from current_iter + 1."""
    s = case.solver
    b, m, ti = s.backend, s.mesh, s.time_integrator
    z = read_checkpoint(path)
    stats = getattr(case, "stats", None)
    spectra = getattr(case, "spectra", None)
    if spectra is not None and not spectra.cfg.active:
        spectra = None
    budgets = getattr(case, "budgets", None)
    if budgets is not None and not budgets.cfg.active:
        budgets = None
    particles = getattr(case, "particles", None)
    scalars = getattr(s, "scalars", None)
    if scalars is not None and not scalars.profiling:
        scalars = None
    # 2. does it fit?
    if int(z["precision"]) != REAL_BYTES:
        raise _differs("precision (bytes per real)", int(z["precision"]), REAL_BYTES)
    for key, here in (("dims", m.get_dims(VERT)), ("global_dims", m.get_global_dims(VERT)),
                      ("nproc_dir", m.nproc_dir), ("n_offset", m.n_offset)):
        stored = tuple(int(v) for v in z[key])
        here = tuple(int(v) for v in here)
        if stored != here:
            raise _differs(key, stored, here)
    is_ab = ti.sname[:2] == "AB"
    if bool(z["ti_is_ab"]) != is_ab:
        raise _differs("ti_is_ab (the integrator family)", bool(z["ti_is_ab"]), is_ab)
    if int(z["ti_order"]) != ti.order:
        raise _differs("ti_order", int(z["ti_order"]), ti.order)
    if int(z["n_species"]) != len(s.species):
        raise _differs("n_species", int(z["n_species"]), len(s.species))
    fields = state_fields(s, stats)
    names = [str(n) for n in z["names"]]
    if names != [k for k, _ in fields]:
        raise _differs("names (the variables of the state)", names, [k for k, _ in fields])
    dims = tuple(int(v) for v in m.get_dims(VERT))
    shape = (dims[2], dims[1], dims[0])
    real = np.dtype(_lib.NP_REAL)
    for k in names:
        if k not in z:
            raise X3dError("restore: the checkpoint lists `%s` but does not hold it" % k)
        if z[k].dtype != real or z[k].shape != shape:
            raise _differs("`%s` (type, shape)" % k, (z[k].dtype.name, z[k].shape), (real.name, shape))
    stored = np.asarray(z["checksums"])
    if stored.dtype != np.uint64 or stored.shape != (len(names), 3):
        raise _differs("checksums (type, shape)", (stored.dtype.name, stored.shape), ("uint64", (len(names), 3)))
    profile = stats is not None and stats.cfg.active and stats.cfg.profile_dir is not None
    if stats is not None and stats.cfg.active:
        if int(z.get("stats_profile_dir", -1)) != int(stats.cfg.profile_dir or 0):
            raise _differs("stats_profile_dir", int(z.get("stats_profile_dir", -1)), int(stats.cfg.profile_dir or 0))
    if spectra is not None:
        from .spectra import mean_from_state
        if "spectra_sample_count" not in z:
            raise X3dError("restore: this run samples spectra, the checkpoint holds none")
        mean_from_state(z, spectra.cfg.mode, spectra.cfg.fields)  # (raises on another mode or other fields)
    if budgets is not None:
        from .budgets import moments_from_state
        if "budgets_sample_count" not in z:
            raise X3dError("restore: this run samples budgets, the checkpoint holds none")
        # (raises on another profile_dir, another pressure setting or another length)
        moments_from_state(z, budgets.cfg.profile_dir, budgets.cfg.pressure, budgets.n_keep_global)
    if particles is not None:
        from .particles import check_state_dict
        check_state_dict(z, particles.n, particles.cfg.order, particles.cfg.tau_p)  # (raises on none, another n, order, tau_p)
    if scalars is not None:
        scalars.check_state_dict(z)  # (raises on none, another profile_dir, another length or species count)
    # 3. upload, 4. the checksums of what arrived, one host wait
    n = int(np.prod(dims))
    data, off, total = b.checkpoint_layout(len(names), n)
    dev, host = b.checkpoint_buffers(total)
    staged = host.numpy()[:data].view(real).reshape((len(names),) + shape)
    for k, name in enumerate(names):
        staged[k] = z[name]
    b.checkpoint_upload(dev, host, data)
    b.checkpoint_sums(dev, len(names), n)
    got = b.checkpoint_table(dev, len(names), n)
    for k, name in enumerate(names):
        for col, what in enumerate(("s1", "s2", "nonfinite")):
            if int(got[k, col]) != int(stored[k, col]):
                raise X3dError("restore: checksum %s of `%s` differs: the checkpoint says %d, its data give %d"
                               % (what, name, int(stored[k, col]), int(got[k, col])))
    # 5. from here on the solver is written
    s.flush_grad()  # (nothing may be pending on fields that are about to be replaced)
    b.checkpoint_unpack([f for _, f in fields], dims, dev)
    loc = int(z["data_loc"])
    for f in (s.u, s.v, s.w):
        f.set_data_loc(loc)
    for f in s.species:
        f.set_data_loc(loc)
    s.dt = float(z["dt"])
    s.current_iter = int(z["timestep"])
    ti.istep, ti.nstep, ti.gdt = int(z["ti_istep"]), int(z["ti_nstep"]), float(z["ti_gdt"])
    ti.istage = int(z["ti_istage"])
    if stats is not None and stats.cfg.active:
        if profile:
            stats.load_state_dict(z)
        stats.sample_count = int(z["stats_sample_count"])
    if spectra is not None:
        spectra.load_state_dict(z)
    if budgets is not None:
        budgets.load_state_dict(z)
    if particles is not None:
        particles.load_state_dict(z)
    if scalars is not None:
        scalars.load_state_dict(z)
    case.load_checkpoint_state({k[5:]: v for k, v in z.items() if k.startswith("case_")})
    case.restarted = True
    return s.current_iter


def restart_from_checkpoint(case, cfg):
    """what the reference does when restart_from_checkpoint is set (io_manager.f90, handle_restart): one line after
    make_*; returns the iteration the run continues from, or None if no restart was asked for"""
    if not cfg.restart_from_checkpoint:
        return None
    if not cfg.restart_file:
        raise X3dError("restart_from_checkpoint is set, but restart_file is empty")
    return restore(case, cfg.restart_file)
