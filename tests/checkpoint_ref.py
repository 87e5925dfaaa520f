"""numpy reference for the checkpoint checksums (csrc/checkpoint.hip) and a host-only stand-in for the backend and the
solver, so that x3d2_amd/checkpoint.py can be driven without a GPU (tests/test_checkpoint_host.py)."""
import numpy as np


def bits_of(a):
    """the elements' bit patterns in dense order, zero-extended to uint64"""
    a = np.ascontiguousarray(a).reshape(-1)
    assert a.dtype in (np.dtype("float32"), np.dtype("float64"))
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)


def table_row(a):
    """(s1, s2, nonfinite): bits.sum() and (bits * (2 i + 1)).sum() in uint64, which wraps"""
    bits = bits_of(a)
    i = np.arange(bits.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        s1 = bits.sum(dtype=np.uint64)
        s2 = (bits * (np.uint64(2) * i + np.uint64(1))).sum(dtype=np.uint64)
    a = np.asarray(a)
    return np.array([s1, s2, np.count_nonzero(np.isnan(a) | np.isinf(a))], dtype=np.uint64)


def table(arrays):
    return np.stack([table_row(a) for a in arrays])


# ---------------------------------------------------------------- host stand-ins
class StubField:
    def __init__(self, shape, dtype):
        self.a = np.zeros(shape, dtype=dtype)
        self.data_loc = 0

    def set_data_loc(self, loc):
        self.data_loc = loc


class StubMesh:
    def __init__(self, dims, nproc_dir=(1, 1, 1), nrank=0):
        self.dims = tuple(dims)
        self.nproc_dir = np.array(nproc_dir)
        self.nproc, self.nrank = int(np.prod(nproc_dir)), nrank
        self.n_offset = np.zeros(3, dtype=int)

    def get_dims(self, loc):
        return self.dims

    def get_global_dims(self, loc):
        return tuple(int(d * p) for d, p in zip(self.dims, self.nproc_dir))


class StubBackend:
    """the calls Checkpoints and restore make, on numpy arrays; the copy `lands` when land() is called"""
    CKPT_MAXBLOCK = 64

    def __init__(self, real):
        self.real = np.dtype(real)
        self.waits = 0
        self.landed = True
        self.unpacked = 0

    def checkpoint_layout(self, nblock, n):
        data = nblock * n * self.real.itemsize
        off = (data + 15) // 16 * 16
        return data, off, off + nblock * 24

    def checkpoint_buffers(self, nbytes):
        import torch
        return torch.zeros(nbytes, dtype=torch.uint8), torch.zeros(nbytes, dtype=torch.uint8)

    def checkpoint_pack(self, fields, dims, buf):
        n = int(np.prod(dims))
        data, off, total = self.checkpoint_layout(len(fields), n)
        raw = buf.numpy()
        raw[:data].view(self.real)[:] = np.concatenate([f.a.reshape(-1) for f in fields])
        raw[off:total].view(np.uint64)[:] = table([f.a for f in fields]).reshape(-1)
        return total

    def snapshot_copy_async(self, host, dev, nbytes):
        host[:nbytes] = dev[:nbytes]
        return 0

    def snapshot_done(self, handle):
        return self.landed

    def snapshot_wait(self, handle):
        self.waits += 1

    def checkpoint_upload(self, buf, host, nbytes):
        buf[:nbytes] = host[:nbytes]

    def checkpoint_sums(self, buf, nblock, n):
        data, off, total = self.checkpoint_layout(nblock, n)
        raw = buf.numpy()
        raw[off:total].view(np.uint64)[:] = table(raw[:data].view(self.real).reshape(nblock, n)).reshape(-1)

    def checkpoint_table(self, buf, nblock, n):
        _, off, total = self.checkpoint_layout(nblock, n)
        return buf.numpy()[off:total].view(np.uint64).reshape(nblock, 3).copy()

    def checkpoint_unpack(self, fields, dims, buf):
        n = int(np.prod(dims))
        self.unpacked += 1
        for k, f in enumerate(fields):
            f.a[...] = buf.numpy()[:len(fields) * n * self.real.itemsize].view(self.real)[k * n:(k + 1) * n].reshape(f.a.shape)


class StubIntegrator:
    def __init__(self, sname, nvars, shape, real):
        self.sname, self.order = sname, int(sname[2])
        ab = sname[:2] == "AB"
        self.nstep, self.nolds = (self.order, self.order - 1) if ab else (1, self.order)
        self.istep, self.istage, self.gdt = 1, 1, 0.0
        self.olds = [[StubField(shape, real) for _ in range(self.nolds)] for _ in range(nvars)]


class StubSolver:
    def __init__(self, dims=(5, 4, 3), real="float64", time_intg="AB3", n_species=0, nproc_dir=(1, 1, 1), nrank=0):
        shape = (dims[2], dims[1], dims[0])
        self.mesh, self.backend = StubMesh(dims, nproc_dir, nrank), StubBackend(real)
        self.u, self.v, self.w = (StubField(shape, real) for _ in range(3))
        self.species = [StubField(shape, real) for _ in range(n_species)]
        self.time_integrator = StubIntegrator(time_intg, 3 + n_species, shape, real)
        self.dt, self.current_iter, self.flushes = 1e-3, 0, 0

    def flush_grad(self):
        self.flushes += 1

    def fields(self):
        return [self.u, self.v, self.w] + self.species + [f for row in self.time_integrator.olds for f in row]

    def randomise(self, seed):
        rng = np.random.default_rng(seed)
        for f in self.fields():
            f.a[...] = rng.standard_normal(f.a.shape).astype(f.a.dtype)


class StubCase:
    def __init__(self, solver):
        self.solver, self.stats, self.restarted, self.state = solver, None, False, {"noise_draws": np.int64(7)}

    def checkpoint_state(self):
        return dict(self.state)

    def load_checkpoint_state(self, state):
        self.state = dict(state)
