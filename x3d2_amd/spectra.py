"""Energy spectra with the reduction on the device (csrc/spectrum.hip).  Not in the reference: this project's own
addition, like StatsConfig.profile_dir.

mode "shell": E(k), the energy of every field binned by |k| -- all three directions periodic, what a Taylor-Green run is
read through next to its enstrophy.  A sample is, per field, the forward transform the Poisson solver already owns
(x3d_poisson_fft_forward) and ONE launch that reads the spectrum once.  With C the plain DFT, N = nx ny nz and w(kx) the
Hermitian weight of the half spectrum (1 for kx = 0 and the Nyquist mode of an even nx, 2 otherwise)

    E[b] = sum over the modes with b = floor(sqrt((kx^2 + ky^2) + kz^2) / dk + 0.5) of 1/2 w(kx) |C|^2 / N^2,

k = 2 pi m / L with the signed mode number m, dk = max_i(2 pi / L_i) unless given, so that sum_b E[b] = 1/2 <f^2>.

mode "plane": per y row the one-sided 1-D spectra along x and z -- x and z periodic, y anything (the channel's stretched
rows), what a channel run is judged by at a few wall distances.  A 2-D transform over (z, x) of every y row into a
workspace of the object ([nz][ny][nx/2+1 rounded up to 8] complex: about 0.56 GB at 1024 x 257 x 512 in FP64) and one launch:

    Ex_<f>[y, kx] = sum over all kz of w(kx) 1/2 |C|^2 / (nx nz)^2,   Ez_<f>[y, kz] = the same summed over kx, kz and nz - kz folded.

Bins, partial sums and running means are float64 in both flavours of the library; the reductions use no atomics and give
the same bits for the same field.  Nothing leaves the device until spectrum() / mean() / write() / state_dict() ask for it.
One rank only.

Output: `<prefix>_<it:06d>.npz` (load_spectra reads it back)."""
import ctypes
import math

import numpy as np

from . import _lib
from .common import VERT, X3dError, sample_due

MODES = ("shell", "plane")
MAXBINS = 4096


class SpectraConfig:
    """when to sample (as StatsConfig: from iteration initspec on, every ispecfreq iterations; initspec <= 0: never),
    when to write (every ispecout iterations; 0: never), what (fields: u, v, w, phi_<n>) and how (mode, dk)"""

    def __init__(self, mode="shell", initspec=0, ispecfreq=1, ispecout=0, spectra_prefix="spectra", dk=None,
                 fields=("u", "v", "w")):
        if mode not in MODES:
            raise X3dError('SpectraConfig: mode must be "shell" or "plane"')
        self.mode = mode
        self.initspec, self.ispecfreq, self.ispecout = int(initspec), int(ispecfreq), int(ispecout)
        if self.ispecfreq < 1:
            raise X3dError("SpectraConfig: ispecfreq must be at least 1")
        self.spectra_prefix = str(spectra_prefix)
        if dk is not None and not float(dk) > 0.0:
            raise X3dError("SpectraConfig: dk must be positive")
        self.dk = None if dk is None else float(dk)
        self.fields = tuple(str(f) for f in fields)
        if not self.fields or len(set(self.fields)) != len(self.fields):
            raise X3dError("SpectraConfig: fields must be distinct names, at least one")
        for f in self.fields:
            if f not in ("u", "v", "w") and not (f.startswith("phi_") and f[4:].isdigit() and int(f[4:]) >= 1):
                raise X3dError("SpectraConfig: unknown field `%s` (u, v, w, phi_<n>)" % f)

    @property
    def active(self):
        return self.initspec > 0

    def sample_due(self, it):
        return sample_due(it, self.initspec, self.ispecfreq)

    due = sample_due

    def output_due(self, it):
        return self.active and self.ispecout > 0 and it % self.ispecout == 0


# ---------------------------------------------------------------- host side: layout, file, state
def default_dk(L):
    return max(2.0 * math.pi / float(l) for l in L)


def shell_nbins(dims, L, dk):
    """floor(sqrt(sum (pi n_i / L_i)^2) / dk + 0.5) + 1: the corner of the spectrum falls into the last bin"""
    s2 = 0.0
    for n, l in zip(dims, L):
        s2 += (math.pi * int(n) / float(l)) * (math.pi * int(n) / float(l))
    return int(math.floor(math.sqrt(s2) / dk + 0.5)) + 1


class Layout:
    """what a slot of the library's arrays means: shell -> nbins values; plane -> Ex[ny, nx/2+1] then Ez[ny, nz/2+1]"""

    def __init__(self, mode, dims, L, dk=None, y=None):
        self.mode = mode
        self.dims = tuple(int(n) for n in dims)
        self.L = tuple(float(l) for l in L)
        nx, ny, nz = self.dims
        self.nxm, self.nzh = nx // 2 + 1, nz // 2 + 1
        if mode == "shell":
            self.dk = default_dk(self.L) if dk is None else float(dk)
            self.nbins = shell_nbins(self.dims, self.L, self.dk)
            self.len = self.nbins
            self.k = np.arange(self.nbins) * self.dk  # the bin centres
        else:
            self.dk, self.nbins = 0.0, 0
            self.len = ny * (self.nxm + self.nzh)
            self.kx = 2.0 * math.pi * np.arange(self.nxm) / self.L[0]
            self.kz = 2.0 * math.pi * np.arange(self.nzh) / self.L[2]
            self.y = np.arange(ny, dtype=np.float64) if y is None else np.asarray(y, dtype=np.float64)[:ny].copy()

    def arrays(self, raw, fields):
        """the library's [nslots, len] array as the dict spectrum() / mean() return"""
        raw = np.asarray(raw, dtype=np.float64).reshape(len(fields), self.len)
        if self.mode == "shell":
            out = {"k": self.k.copy()}
            for f, r in zip(fields, raw):
                out["E_" + f] = r.copy()
            if all("E_" + c in out for c in "uvw"):
                out["E"] = (out["E_u"] + out["E_v"]) + out["E_w"]
            return out
        ny = self.dims[1]
        out = {"kx": self.kx.copy(), "kz": self.kz.copy(), "y": self.y.copy()}
        for f, r in zip(fields, raw):
            out["Ex_" + f] = r[:ny * self.nxm].reshape(ny, self.nxm).copy()
            out["Ez_" + f] = r[ny * self.nxm:].reshape(ny, self.nzh).copy()
        return out

    def raw(self, arrays, fields):
        """the inverse of arrays()"""
        rows = []
        for f in fields:
            if self.mode == "shell":
                rows.append(np.asarray(arrays["E_" + f], dtype=np.float64).reshape(-1))
            else:
                rows.append(np.concatenate([np.asarray(arrays["Ex_" + f], dtype=np.float64).reshape(-1),
                                            np.asarray(arrays["Ez_" + f], dtype=np.float64).reshape(-1)]))
        out = np.ascontiguousarray(np.stack(rows))
        if out.shape != (len(fields), self.len):
            raise X3dError("spectra: arrays of shape %s do not fit this layout (%d values per field)"
                           % (out.shape, self.len))
        return out


def file_name(prefix, it):
    return "%s_%06d.npz" % (prefix, int(it))


def save_spectra(prefix, it, mode, fields, sample_count, inst, mean):
    """`<prefix>_<it:06d>.npz`: mode, fields, sample_count, the axes, the instantaneous arrays under their names and the
    running means under `mean_<name>`; returns the file name"""
    payload = {"mode": np.array(mode), "fields": np.array(list(fields)), "sample_count": np.array(int(sample_count)),
               "iteration": np.array(int(it))}
    axes = ("k", "kx", "kz", "y")
    for k, v in inst.items():
        payload[k] = v
    for k, v in mean.items():
        if k not in axes:
            payload["mean_" + k] = v
    name = file_name(prefix, it)
    np.savez(name, **payload)
    return name


def load_spectra(prefix, it):
    """what write(it) wrote: {"mode", "fields", "sample_count", "iteration", "spectrum": {...}, "mean": {...}} with the
    two dicts as spectrum() and mean() return them"""
    with np.load(file_name(prefix, it), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    out = {"mode": str(d.pop("mode")), "fields": tuple(str(f) for f in d.pop("fields")),
           "sample_count": int(d.pop("sample_count")), "iteration": int(d.pop("iteration"))}
    axes = {k: d[k] for k in ("k", "kx", "kz", "y") if k in d}
    out["spectrum"] = {k: v for k, v in d.items() if not k.startswith("mean_")}
    out["mean"] = dict(axes)
    out["mean"].update({k[5:]: v for k, v in d.items() if k.startswith("mean_")})
    return out


def state_from_mean(mode, fields, sample_count, mean):
    """the checkpoint variables: spectra_sample_count, spectra_mode, spectra_fields and the running means under
    `spectra_<name>` (the axes are not state)"""
    out = {"spectra_sample_count": np.array(int(sample_count)), "spectra_mode": np.array(mode),
           "spectra_fields": np.array(list(fields))}
    for k, v in mean.items():
        if k not in ("k", "kx", "kz", "y", "E"):
            out["spectra_" + k] = np.asarray(v, dtype=np.float64)
    return out


def mean_from_state(state, mode, fields):
    """the inverse; the state must have been taken in the same mode on the same fields"""
    if str(state["spectra_mode"]) != mode:
        raise X3dError("spectra: the state was taken in mode `%s`, this run samples `%s`" % (str(state["spectra_mode"]), mode))
    stored = tuple(str(f) for f in np.asarray(state["spectra_fields"]).reshape(-1))
    if stored != tuple(fields):
        raise X3dError("spectra: the state holds the fields %s, this run samples %s" % (stored, tuple(fields)))
    names = ["E_" + f for f in fields] if mode == "shell" else [p + f for f in fields for p in ("Ex_", "Ez_")]
    return int(state["spectra_sample_count"]), {n: np.asarray(state["spectra_" + n], dtype=np.float64) for n in names}


# ---------------------------------------------------------------- the device object
class Spectra:
    """owns the library's x3d_spectra object and sample_count; BaseCase.run calls update(it) and write(it) when the case
    has one (case.spectra = Spectra(case.solver, cfg))"""

    def __init__(self, solver, cfg):
        self.solver, self.cfg = solver, cfg
        self.sample_count = 0
        self.h = None
        self.files = []
        b, m = solver.backend, solver.mesh
        if int(m.nproc) > 1 or getattr(b, "_emulate", "") or b.comm.size > 1:
            raise X3dError("Spectra: a decomposed mesh is not served (multi-rank spectra are not built)")
        per = tuple(bool(p) for p in m.periodic_BC)
        if cfg.mode == "shell" and not all(per):
            raise X3dError("Spectra: shell mode needs all three directions periodic (periodic = %s)" % (per,))
        if cfg.mode == "plane" and not (per[0] and per[2]):
            raise X3dError("Spectra: plane mode needs x and z periodic (periodic = %s)" % (per,))
        nspecies = len(getattr(solver, "species", []))
        for f in cfg.fields:
            if f.startswith("phi_") and int(f[4:]) > nspecies:
                raise X3dError("Spectra: field `%s`, but the solver transports %d species" % (f, nspecies))
        dims = tuple(int(n) for n in m.get_dims(VERT))
        self.layout = Layout(cfg.mode, dims, m.L, cfg.dk, y=m.vert_coords[1] if cfg.mode == "plane" else None)
        if cfg.mode == "shell":
            if self.layout.nbins > MAXBINS:
                raise X3dError("Spectra: dk = %g gives %d bins, at most %d are served" % (self.layout.dk, self.layout.nbins, MAXBINS))
            pf = getattr(b, "poisson_fft", None)
            from .poisson_fft import HipPoissonFFT
            if type(pf) is not HipPoissonFFT or pf.case != "000":
                raise X3dError("Spectra: shell mode needs the backend's single-rank FFT Poisson object (poisson=\"FFT\")")
            self._poisson = pf
        else:
            self._poisson = None
        if not cfg.active:
            return  # (like Stats: an inactive object owns nothing)
        h = ctypes.c_void_p()
        L = (ctypes.c_double * 3)(*[float(l) for l in m.L])
        _lib.check(b.lib.x3d_spectra_create(b.h, ctypes.byref(h), MODES.index(cfg.mode), _lib.ints(*dims),
                                            _lib.ints(*[int(p) for p in per]), L,
                                            0.0 if cfg.dk is None else float(cfg.dk), len(cfg.fields)))
        self.h = h
        sz = (ctypes.c_long * 8)()
        dk = ctypes.c_double(0.0)
        _lib.check(b.lib.x3d_spectra_sizes(h, sz, ctypes.byref(dk)))
        if int(sz[3]) != self.layout.len or (cfg.mode == "shell" and dk.value != self.layout.dk):
            raise X3dError("Spectra: the library's layout (%d values, dk = %r) is not the host's (%d, %r)"
                           % (int(sz[3]), dk.value, self.layout.len, self.layout.dk))
        self.groups = int(sz[7])

    def __del__(self):
        try:
            if self.h is not None:
                self.solver.backend.lib.x3d_spectra_destroy(self.h)
        except Exception:
            pass

    def _need_active(self):
        if self.h is None:
            raise X3dError("spectra are inactive (initspec <= 0)")

    def _field(self, name):
        s = self.solver
        if name in ("u", "v", "w"):
            return getattr(s, name)
        return s.species[int(name[4:]) - 1]

    # ------------------------------------------------------------ sampling
    def sample(self):
        """the instantaneous spectrum of every field; no running mean, no host wait"""
        self._need_active()
        s = self.solver
        b = s.backend
        s.flush_grad()  # a velocity correction left pending by step(more=True) is not in u, v, w yet
        ph = None if self._poisson is None else self._poisson.h
        for slot, name in enumerate(self.cfg.fields):
            f = self._field(name)
            if f.data_loc != VERT:
                raise X3dError("Spectra: field `%s` must be at VERT" % name)
            _lib.check(b.lib.x3d_spectra_sample(self.h, ph, f.ptr, slot))

    def reads_state(self, it):
        """does update(it) read the solver's fields?  (BaseCase.run then completes the step first)"""
        return self.cfg.sample_due(it)

    def update(self, it):
        """one sample if iteration `it` is due: every field's spectrum, then the running means; returns whether one was
        taken.  No host wait."""
        if not self.reads_state(it):
            return False
        self.sample()
        self.sample_count += 1
        _lib.check(self.solver.backend.lib.x3d_spectra_accumulate(self.h, self.sample_count))
        return True

    # ------------------------------------------------------------ results (host arrays, float64)
    def _read(self, which):
        self._need_active()
        out = np.empty((len(self.cfg.fields), self.layout.len), dtype=np.float64)
        _lib.check(self.solver.backend.lib.x3d_spectra_read(self.h, which, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def spectrum(self):
        """the last sample.  shell: k (the bin centres b dk), E_<f> per field and, when u, v, w are all sampled,
        E = E_u + E_v + E_w.  plane: kx, kz, y and per field Ex_<f>[ny, nx/2+1], Ez_<f>[ny, nz/2+1]."""
        return self.layout.arrays(self._read(0), self.cfg.fields)

    def mean(self):
        """the running mean over the samples so far, same names"""
        return self.layout.arrays(self._read(1), self.cfg.fields)

    # ------------------------------------------------------------ output, restart
    def write(self, it):
        """`<prefix>_<it:06d>.npz` when ispecout divides `it`; returns the file name or None"""
        if not self.cfg.output_due(it):
            return None
        name = save_spectra(self.cfg.spectra_prefix, it, self.cfg.mode, self.cfg.fields, self.sample_count,
                            self.spectrum(), self.mean())
        self.files.append(name)
        return name

    def state_dict(self):
        """what a restarted run needs: the sample count and the running means (a few KB to a few MB, through the host)"""
        return state_from_mean(self.cfg.mode, self.cfg.fields, self.sample_count, self.mean())

    def load_state_dict(self, state):
        self._need_active()
        count, mean = mean_from_state(state, self.cfg.mode, self.cfg.fields)
        raw = self.layout.raw(mean, self.cfg.fields)
        _lib.check(self.solver.backend.lib.x3d_spectra_load(self.h, raw.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        self.sample_count = count
