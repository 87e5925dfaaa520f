"""numpy restatement (float64) of the energy spectra of csrc/spectrum.hip, the checker of tests/test_hip_spectra.py; pinned
by tests/test_spectra_host.py to two facts that need no device.

shell   C = rfftn(f) / N;  E[b] = sum 1/2 w(kx) |C|^2 over the modes of bin b = floor(sqrt((kx^2 + ky^2) + kz^2) / dk + 0.5),
        k = 2 pi m / L with the signed mode number m, w = 1 for kx = 0 and the Nyquist mode of an even nx, else 2
plane   per y row C = rfft2 over (z, x) / (nx nz);  Ex[y, kx] = sum over kz of 1/2 w |C|^2;  Ez[y, kz] = the same summed over
        kx, the modes kz and nz - kz added in that order

Arrays are [nz, ny, nx], x fastest, as everywhere in the tests."""
import numpy as np


def k2_table(n, L, half=False):
    """(2 pi m / L)^2 for m = 0 .. n/2 (half) or the signed mode numbers of all n modes"""
    m = np.arange(n // 2 + 1) if half else np.where(np.arange(n) <= n // 2, np.arange(n), np.arange(n) - n)
    k = 2.0 * np.pi * m.astype(np.float64) / float(L)
    return k * k


def hermitian_weights(nx):
    w = np.full(nx // 2 + 1, 2.0)
    w[0] = 1.0
    if nx % 2 == 0:
        w[nx // 2] = 1.0
    return w


def default_dk(L):
    return max(2.0 * np.pi / float(l) for l in L)


def nbins(dims, L, dk):
    s2 = 0.0
    for n, l in zip(dims, L):
        s2 += (np.pi * n / float(l)) * (np.pi * n / float(l))
    return int(np.floor(np.sqrt(s2) / dk + 0.5)) + 1


def shell_bins(dims, L, dk):
    """(bin index [nz, ny, nx/2+1], distance of the nearest mode to a bin edge in units of dk)"""
    nx, ny, nz = dims
    kx2 = k2_table(nx, L[0], half=True)[None, None, :]
    ky2 = k2_table(ny, L[1])[None, :, None]
    kz2 = k2_table(nz, L[2])[:, None, None]
    q = np.sqrt((kx2 + ky2) + kz2) / dk + 0.5  # the order of operations of the kernel
    b = np.floor(q).astype(np.int64)
    frac = q - np.floor(q)
    return b, float(np.min(np.minimum(frac, 1.0 - frac)))


def shell(f, L, dk=None):
    """E[nbins] of one field"""
    f = np.asarray(f, dtype=np.float64)
    nz, ny, nx = f.shape
    dims = (nx, ny, nz)
    dk = default_dk(L) if dk is None else float(dk)
    c = np.fft.rfftn(f, axes=(0, 1, 2)) / f.size
    e = 0.5 * hermitian_weights(nx)[None, None, :] * (c.real * c.real + c.imag * c.imag)
    b, _ = shell_bins(dims, L, dk)
    return np.bincount(b.reshape(-1), weights=e.reshape(-1), minlength=nbins(dims, L, dk))


def plane(f):
    """(Ex[ny, nx/2+1], Ez[ny, nz/2+1]) of one field"""
    f = np.asarray(f, dtype=np.float64)
    nz, ny, nx = f.shape
    c = np.fft.rfft2(f, axes=(0, 2)) / (nx * nz)  # [kz, y, kx]
    e = 0.5 * hermitian_weights(nx)[None, None, :] * (c.real * c.real + c.imag * c.imag)
    ex = e.sum(axis=0)
    s = e.sum(axis=2)  # [kz, y]
    nzh = nz // 2 + 1
    ez = np.empty((ny, nzh))
    for k in range(nzh):
        km = nz - k
        ez[:, k] = s[k] + s[km] if (k > 0 and km != k) else s[k]
    return ex, ez


def running_mean(samples):
    """mean += (inst - mean) / count, the device's recurrence, in float64"""
    mean = None
    for n, x in enumerate(samples, 1):
        x = np.asarray(x, dtype=np.float64)
        mean = np.zeros_like(x) if mean is None else mean
        mean = mean + (x - mean) / np.float64(n)
    return mean


def tolerance(n_points, eps, total):
    """16 eps log2(N) sum(E_ref): a bin is a sum of non-negative terms bounded by the total, a Cooley-Tukey transform
    carries a relative l2 error of order eps log2 N, squaring doubles it"""
    return 16.0 * eps * np.log2(n_points) * total


def tgv(dims, L=None):
    """the Taylor-Green initial velocity on a periodic box (2 pi each unless L is given)"""
    nx, ny, nz = dims
    L = (2 * np.pi,) * 3 if L is None else L
    x = (np.arange(nx) * (L[0] / nx))[None, None, :]
    y = (np.arange(ny) * (L[1] / ny))[None, :, None]
    z = (np.arange(nz) * (L[2] / nz))[:, None, None]
    return np.sin(x) * np.cos(y) * np.cos(z), -np.cos(x) * np.sin(y) * np.cos(z), np.zeros((nz, ny, nx))
