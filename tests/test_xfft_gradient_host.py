"""CPU twin of tests/test_xfft_gradient.py (no GPU): the algebra of the z-first 000 solve WITHOUT its inverse x pass, in
numpy on small all-periodic boxes, with circulant stand-ins for the y and z operators of gradient_c2v (any real circulant
along y or z is x-independent and real-linear column by column, which is all the argument uses).

  path A  spectrum packed along x -> multiplier, real and even in kx -> untangle -> inverse x transform -> inverse z
          transform (complex -> real) -> the y / z operators: the sequence with the x pass (csrc/zfirst.hip
          x3d_poisson_zfirst_middle_xpacked);
  path B  multiplier -> inverse z transform of every packed column on its own -> the y / z operators on the packed
          columns -> the packed inverse last (csrc/fft512_core.h irfft512_packed_wave inside the x operators).

They must agree to 1e-12 of the maximum.  The re-tangle formula of irfft512_packed_wave is checked against numpy.fft.irfft
at n = 512 and two small sizes, with the kernel's scaling (n x the rows)."""
import numpy as np
import pytest

import xfft_ref


def _circulant_apply(a, taps, axis):
    """sum_j taps[j] * roll(a, j - len(taps) // 2) along axis: a real circulant operator, the same for every column"""
    out = np.zeros_like(a)
    h = len(taps) // 2
    for j, t in enumerate(taps):
        out = out + t * np.roll(a, j - h, axis=axis)
    return out


def _circulant_solve(a, lhs, axis):
    """the inverse of such an operator (a compact scheme's left-hand side), through the axis' own transform"""
    n = a.shape[axis]
    col = np.zeros(n)
    h = len(lhs) // 2
    for j, t in enumerate(lhs):
        col[(j - h) % n] += t
    sym = np.fft.fft(col)
    shp = [1] * a.ndim
    shp[axis] = n
    return np.fft.ifft(np.fft.fft(a, axis=axis) / sym.reshape(shp), axis=axis).real


def irfft_packed(P):
    """the re-tangle of irfft512_packed_wave on packed rows P[..., n] -> n x the real rows:
    Z_k = (F_k + conj F_{n/2-k}) + i W_n^{-k} (F_k - conj F_{n/2-k}),  n (r[2m] + i r[2m+1]) = FFT_{n/2}<+1>(Z)_m"""
    n = P.shape[-1]
    h = n // 2
    F = np.empty(P.shape[:-1] + (h + 1,), dtype=np.complex128)
    F[..., 0], F[..., h] = P[..., 0], P[..., 1]
    F[..., 1:h] = P[..., 2::2] + 1j * P[..., 3::2]
    k = np.arange(h)
    Fk, Fp = F[..., :h], np.conj(F[..., h - k])
    Z = (Fk + Fp) + 1j * np.exp(2j * np.pi * k / n) * (Fk - Fp)
    z = np.fft.ifft(Z, axis=-1) * h   # unnormalised e^{+i} transform of n / 2 points
    r = np.empty(P.shape, dtype=np.float64)
    r[..., 0::2], r[..., 1::2] = z.real, z.imag
    return r


@pytest.mark.parametrize("n", [8, 32, 512])
def test_retangle_formula_against_numpy_irfft(n):
    rng = np.random.default_rng(n)
    P = rng.standard_normal((7, n))           # any packed row is the rfft of some real row
    h = n // 2
    F = np.empty((7, h + 1), dtype=np.complex128)
    F[:, 0], F[:, h] = P[:, 0], P[:, 1]
    F[:, 1:h] = P[:, 2::2] + 1j * P[:, 3::2]
    ref = n * np.fft.irfft(F, n=n, axis=-1)
    got = irfft_packed(P)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # ... and it inverts xfft_ref.pack
    r = rng.standard_normal((3, n))
    assert np.abs(irfft_packed(xfft_ref.pack(r)) - n * r).max() <= 1e-12 * n * np.abs(r).max()


@pytest.mark.parametrize("dims", [(16, 12, 10), (32, 8, 16)])
def test_skipped_inverse_x_pass_commutes_with_the_gradient_operators(dims):
    nx, ny, nz = dims
    rng = np.random.default_rng(nx + ny)
    # a spectrum as the y middle leaves it: packed along x, every packed column the z half-spectrum of a REAL column;
    # made from three random real fields so that nothing is special about it
    d = xfft_ref.pack(rng.standard_normal((nz, ny, nx)))
    C = np.fft.fft(np.fft.rfft(d, axis=0), axis=1)                       # [kz <= nz/2, ky, packed x]
    # spectral multiplier: real, even in kx (and in ky, kz: it is applied on full / half axes as the solve does)
    kx = np.minimum(np.arange(nx), nx - np.arange(nx))
    ky = np.minimum(np.arange(ny), ny - np.arange(ny))
    kz = np.arange(nz // 2 + 1)
    g = 1.0 / (1.0 + kx[None, None, :] ** 2 + 0.5 * ky[None, :, None] ** 2 + 0.25 * kz[:, None, None] ** 2)
    assert np.array_equal(g, g[:, :, (-np.arange(nx)) % nx])
    Cg = np.fft.ifft(C * g[:, :, xfft_ref.packed_kx(nx)], axis=1)         # the y middle, table of the columns' x modes

    def grad_yz(p):
        """stand-ins for the z pair, the y pair and the single y operator of gradient_c2v: three fields"""
        pz = _circulant_solve(_circulant_apply(p, [0.1, 0.4, 0.4, 0.1, 0.0], 0), [0.3, 1.0, 0.3], 0)     # interpl_z
        dz = _circulant_solve(_circulant_apply(p, [-0.2, -0.9, 0.9, 0.2, 0.0], 0), [0.2, 1.0, 0.2], 0)   # stagder_z
        py = _circulant_solve(_circulant_apply(pz, [0.1, 0.4, 0.4, 0.1, 0.0], 1), [0.3, 1.0, 0.3], 1)
        dy = _circulant_solve(_circulant_apply(pz, [-0.2, -0.9, 0.9, 0.2, 0.0], 1), [0.2, 1.0, 0.2], 1)
        dzy = _circulant_solve(_circulant_apply(dz, [0.1, 0.4, 0.4, 0.1, 0.0], 1), [0.3, 1.0, 0.3], 1)
        return py, dy, dzy

    # ---- path A: untangle, inverse x (unnormalised: nx x), inverse z, operators
    H = np.fft.ifft(xfft_ref.untangle(Cg), axis=2) * nx
    pA = np.fft.irfft(H, n=nz, axis=0)
    # (the untangled spectrum is Hermitian: what the complex -> real z transform of path A relies on)
    assert np.abs(H[0].imag).max() <= 1e-12 * np.abs(H).max()
    A = grad_yz(pA)
    # ---- path B: inverse z of every packed column on its own, operators on the packed columns, packed inverse last
    pB = np.fft.irfft(Cg, n=nz, axis=0)
    B = [irfft_packed(f) for f in grad_yz(pB)]
    for a, b in zip(A, B):
        err = np.abs(a - b).max()
        print("dims %s: max |A - B| = %.3e of %.3e" % (dims, err, np.abs(a).max()))
        assert err <= 1e-12 * np.abs(a).max(), (err, np.abs(a).max())
    # the packed fields themselves are pack(rfft_x(path A's fields)) / nx: what the x operators are handed
    for a, f in zip(A, grad_yz(pB)):
        assert np.abs(xfft_ref.pack(a) / nx - f).max() <= 1e-12 * np.abs(f).max()
