"""Host restatement of the z-first 000 solve with its forward x transform inside the divergence's x operators
(csrc/xscan.hip k_xscan_tds_xfft, csrc/zfirst.hip x3d_poisson_zfirst_middle_xpacked), shared by tests/test_xfft_divergence.py
and its CPU twin.  Arrays are [z, y, x]; the x axis of a packed array holds rfft along x as n reals:
    column 0 = Re F_0, column 1 = Re F_{n/2}, columns 2k, 2k + 1 = Re F_k, Im F_k (k = 1 .. n/2 - 1)."""
import numpy as np


def pack(r):
    """rows of reals -> their unnormalised forward rfft along the last axis, packed half-complex"""
    n = r.shape[-1]
    F = np.fft.rfft(r, axis=-1)
    out = np.empty(r.shape, dtype=np.float64)
    out[..., 0] = F[..., 0].real
    out[..., 1] = F[..., n // 2].real
    out[..., 2::2] = F[..., 1:n // 2].real
    out[..., 3::2] = F[..., 1:n // 2].imag
    return out


def packed_kx(n):
    """the x mode that column c of a packed row carries: 0, n/2 for c = 0, 1 and c >> 1 otherwise"""
    return np.array([0, n // 2] + [c >> 1 for c in range(2, n)])


def untangle(C):
    """columns of complex values (the z / y-spectral images of the packed REAL columns) -> the full complex x spectrum:
    H_0 = col 0, H_{n/2} = col 1, H_m = A_m + i B_m, H_{n-m} = A_m - i B_m with A_m, B_m = cols 2m, 2m + 1"""
    n = C.shape[-1]
    H = np.empty(C.shape, dtype=np.complex128)
    H[..., 0], H[..., n // 2] = C[..., 0], C[..., 1]
    A, B = C[..., 2::2], C[..., 3::2]
    H[..., 1:n // 2] = A + 1j * B
    H[..., n - 1:n // 2:-1] = A - 1j * B
    return H


def tangle(H):
    """inverse of untangle for a spectrum H[..., kx] (any complex rows): the packed columns that untangle to it"""
    n = H.shape[-1]
    C = np.empty(H.shape, dtype=np.complex128)
    C[..., 0], C[..., 1] = H[..., 0], H[..., n // 2]
    lo, hi = H[..., 1:n // 2], H[..., n - 1:n // 2:-1]
    C[..., 2::2] = 0.5 * (lo + hi)
    C[..., 3::2] = -0.5j * (lo - hi)
    return C
