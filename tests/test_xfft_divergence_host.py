"""CPU twin of tests/test_xfft_divergence.py (no GPU): the four steps of the z-first 000 solve with its forward x transform
done by the divergence's x operators, restated in numpy at 16^3 and 32^3 on the oracle's periodic compact operators
(oracle/x3d_oracle.py) and the product's own modified wave numbers (x3d2_amd/poisson_fft.py), against the plain sequence.

  1. the x operators' results leave packed half-complex along x (xfft_ref.pack); the y and z operators of divergence_v2c
     run unchanged on those blocks, and the z transform is a real -> complex one of every REAL column;
  2. column 2k then holds A_k(kz), column 2k + 1 B_k(kz), and the true spectrum is A_k + i B_k;
  3. the y middle with the reciprocal wave numbers indexed by the x mode of the COLUMN (xfft_ref.packed_kx);
  4. the untangle (xfft_ref.untangle) in front of the unchanged inverse x transform.

Bound: 100 eps of the pressure's maximum.  This pins the packing, the kx(c) table and the untangle signs without a kernel."""
import types

import numpy as np
import pytest

import xfft_ref

EPS = np.finfo(np.float64).eps


class _HostFactory:
    """alloc_tdsops without a device: host factory only"""

    def alloc_tdsops(self, *a, **kw):
        from x3d2_amd.tdsops import Tdsops
        return Tdsops(*a, **kw)


def _product_multiplier(n):
    """G[kz, ky, kx] = -1 / waves / n^3 on the full axes (0 where waves < 1e-16): what process_spectral_000 amounts to once
    its rotations have cancelled (csrc/spectral000.h), from the product's wave numbers"""
    from x3d2_amd import Mesh
    from x3d2_amd.common import CELL, DIR_X, DIR_Y, DIR_Z
    from x3d2_amd.poisson_fft import HipPoissonFFT
    from x3d2_amd.solver import allocate_tdsops
    from x3d2_amd.tdsops import Dirps
    per = ("periodic",) * 2
    m = Mesh((n, n, n), (1, 1, 1), (2.0 * np.pi,) * 3, per, per, per)
    dps = []
    for d in (DIR_X, DIR_Y, DIR_Z):
        dp = Dirps(d)
        allocate_tdsops(dp, _HostFactory(), m, "compact6", "compact6", "classic", "compact6")
        dps.append(dp)
    pf = types.SimpleNamespace()
    pf.nx_glob, pf.ny_glob, pf.nz_glob = (int(v) for v in m.get_global_dims(CELL))
    pf.periodic_x, pf.periodic_y, pf.periodic_z = True, True, True
    pf.nx_spec, pf.ny_spec, pf.nz_spec = n // 2 + 1, n, n
    HipPoissonFFT._waves_set(pf, m, *dps)
    waves = HipPoissonFFT.waves_block(pf)                      # [z, y, x mode 0 .. n/2]
    assert waves.shape == (n, n, n // 2 + 1)
    kx = np.minimum(np.arange(n), n - np.arange(n))
    full = waves[:, :, kx]
    with np.errstate(divide="ignore"):
        return np.where(full < 1e-16, 0.0, -1.0 / full) / n ** 3


def _oracle_ops(n):
    """apply(a, name, axis): one periodic compact operator of the oracle along an axis of a [z, y, x] array"""
    from oracle import x3d_oracle as orc
    twopi = 2.0 * np.pi
    om = orc.Mesh([n] * 3, [1, 1, 1], [twopi] * 3, ["periodic"] * 2, ["periodic"] * 2, ["periodic"] * 2)
    o = orc.Solver(om, poisson="FFT")
    dirs = {2: (orc.DIR_X, o.xdirps), 1: (orc.DIR_Y, o.ydirps), 0: (orc.DIR_Z, o.zdirps)}

    def apply(a, name, axis):
        dr, dp = dirs[axis]
        fin, fout = o.backend.get_block(dr, orc.VERT), o.backend.get_block(dr, orc.VERT)
        o.backend.set_field_data(fin, np.ascontiguousarray(a))
        o.backend.tds_solve(fout, fin, getattr(dp, name))
        return o.backend.get_field_data(fout, orc.VERT)
    return o, apply


@pytest.mark.parametrize("n", [16, 32])
def test_packed_x_transform_commutes_with_the_divergence_and_the_division(n):
    G = _product_multiplier(n)
    # (the multiplier is real and even in every wave number: what lets the x transform move)
    idx = (-np.arange(n)) % n
    assert np.array_equal(G, G[idx]) and np.array_equal(G, G[:, idx]) and np.array_equal(G, G[:, :, idx])
    o, apply = _oracle_ops(n)
    rng = np.random.default_rng(20 + n)
    u, v, w = (rng.standard_normal((n, n, n)) for _ in range(3))
    # ---- the plain sequence: divergence_v2c (src/vector_calculus.f90:142-246), then the 3-D transform, division, back
    t1, t2, t3 = apply(u, "stagder_v2p", 2), apply(v, "interpl_v2p", 2), apply(w, "interpl_v2p", 2)

    def yz(t1, t2, t3):  # the y and z stages: column by column of x, coefficients independent of x
        a1 = apply(t1, "interpl_v2p", 1) + apply(t2, "stagder_v2p", 1)
        a2 = apply(t3, "interpl_v2p", 1)
        return apply(a1, "interpl_v2p", 0) + apply(a2, "stagder_v2p", 0)
    div = yz(t1, t2, t3)
    p_plain = np.fft.ifftn(G * np.fft.fftn(div) * n ** 3).real
    # ---- 1: packed behind the x operators; y, z operators unchanged; z real -> complex per REAL column (kz <= n / 2)
    d = yz(xfft_ref.pack(t1), xfft_ref.pack(t2), xfft_ref.pack(t3))
    C = np.fft.rfft(d, axis=0)
    # ---- 2: columns 2k, 2k + 1 are A_k, B_k of the true spectrum A_k + i B_k
    true_zx = np.fft.fft(np.fft.rfft(div, axis=0), axis=2)
    assert np.abs(xfft_ref.untangle(C) - true_zx).max() <= 100 * EPS * np.abs(true_zx).max()
    # ---- 3: the y middle with the table of the columns' x modes
    C = np.fft.ifft(np.fft.fft(C, axis=1) * (G * n ** 3)[: n // 2 + 1][:, :, xfft_ref.packed_kx(n)], axis=1)
    # ---- 4: untangle, inverse x transform, inverse z transform (complex -> real)
    H = np.fft.ifft(xfft_ref.untangle(C), axis=2)
    p_new = np.fft.irfft(H, n=n, axis=0)
    err = np.abs(p_new - p_plain).max()
    print("n = %d: max |p_new - p_plain| = %.3e, max |p| = %.3e" % (n, err, np.abs(p_plain).max()))
    assert err <= 100 * EPS * np.abs(p_plain).max(), (err, np.abs(p_plain).max())
    # the plain sequence here is the oracle's own solve (its rotations cancel): anchors G's sign and normalisation
    p_orc = o.poisson_fft.solve(div.copy())
    assert np.abs(p_orc - p_plain).max() <= 1000 * EPS * np.abs(p_plain).max()


def test_pack_tangle_untangle_round_trip():
    rng = np.random.default_rng(3)
    r = rng.standard_normal((3, 5, 32))
    P = xfft_ref.pack(r)
    F = np.fft.fft(r, axis=-1)
    assert np.abs(xfft_ref.untangle(P.astype(np.complex128)) - F).max() <= 100 * EPS * np.abs(F).max()
    H = rng.standard_normal((4, 32)) + 1j * rng.standard_normal((4, 32))
    assert np.abs(xfft_ref.untangle(xfft_ref.tangle(H)) - H).max() <= 10 * EPS * np.abs(H).max()
    assert list(xfft_ref.packed_kx(8)) == [0, 4, 1, 1, 2, 2, 3, 3]
