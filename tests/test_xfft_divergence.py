"""The z-first 000 solve with its forward x transform inside the divergence's x operators (csrc/xscan.hip k_xscan_tds_xfft,
csrc/zfirst.hip k_c2c512_x<+1, UNT> and x3d_poisson_zfirst_middle_xpacked; X3D_NO_XFFT_DIV=1 restores the plain sequence).
tests/test_xfft_divergence_host.py pins the algebra on the CPU; here the kernels:

  * x3d_tds_solve_xfft alone on a 512 x 3 x 5 block (15 pencils: two workgroups, the second with 7 of 8 waves busy, so the
    tail and the prefetch guard run) against pack(numpy.fft.rfft(plain tds_apply result)), pad columns untouched;
  * the untangling inverse x pass against the plain inverse on the unpacked spectrum;
  * one pressure correction at 512^3 on a broadband velocity against the same with X3D_NO_XFFT_DIV=1 in a child process.

The kernel tolerance is measured, not fixed: the error of the plain forward pass k_c2c512_x<-1> against numpy.fft.fft on
the same number of random rows, times 4 (a real transform adds an untangle stage to the complex one).  With
X3D_TEST_WRITE_PROFILES=1 the measured numbers are appended to profiles/xfft_div.jsonl."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import xfft_ref

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = (512, 3, 5)
NROWS = DIMS[1] * DIMS[2]
PX = 520  # row pitch of the test's spectra in complex numbers (the solver's ZH_PX)
_state = {}


def _record(**kw):
    print("xfft_div:", json.dumps(kw))
    if os.environ.get("X3D_TEST_WRITE_PROFILES") == "1":
        with open(os.path.join(os.path.dirname(HERE), "profiles", "xfft_div.jsonl"), "a") as fh:
            fh.write(json.dumps(kw) + "\n")


def _block():
    """-> (backend, x operators) of a periodic 512 x 3 x 5 block (no solver: y and z are too short for operators)"""
    if "b" not in _state:
        from x3d2_amd import Mesh
        from x3d2_amd.backend import HipBackend
        from x3d2_amd.common import DIR_X
        from x3d2_amd.solver import allocate_tdsops
        from x3d2_amd.tdsops import Dirps
        per = ("periodic",) * 2
        mesh = Mesh(DIMS, (1, 1, 1), (2.0 * np.pi, 1.0, 1.0), per, per, per)
        b = HipBackend(mesh)
        xd = Dirps(DIR_X)
        allocate_tdsops(xd, b, mesh, "compact6", "compact6", "classic", "compact6")
        _state["b"] = (b, xd)
    return _state["b"]


def _c2c_rows(b, rows, mode):
    """x3d_c2c512_x_rows on a copy of rows [nrows, 512] complex128 at pitch PX -> the transformed rows"""
    import torch
    buf = torch.zeros((rows.shape[0], PX), dtype=torch.complex128, device=b.device)
    buf[:, :512] = torch.from_numpy(np.ascontiguousarray(rows)).to(b.device)
    from x3d2_amd import _lib
    _lib.check(b.lib.x3d_c2c512_x_rows(b.h, ctypes.c_void_p(buf.data_ptr()), rows.shape[0], PX, int(mode)))
    torch.cuda.synchronize()
    assert bool((buf[:, 512:] == 0).all()), "the pass wrote beyond its 512 columns"
    return buf[:, :512].cpu().numpy()


def _yardstick():
    """the plain forward pass against numpy.fft.fft on NROWS random rows: max error relative to the largest mode"""
    if "tol" not in _state:
        b, _ = _block()
        rng = np.random.default_rng(512)
        rows = rng.standard_normal((NROWS, 512)) + 1j * rng.standard_normal((NROWS, 512))
        ref = np.fft.fft(rows, axis=1)
        e = float(np.abs(_c2c_rows(b, rows, -1) - ref).max() / np.abs(ref).max())
        assert 0.0 < e < 1e-13, e  # (a 512-point FP64 transform: a few eps sqrt(log n); anything else is a broken yardstick)
        _state["tol"] = 4.0 * e
        _record(what="k_c2c512_x<-1> vs numpy.fft.fft", rows=NROWS, relerr=e, tolerance=4.0 * e)
    return _state["tol"]


@gpu
@pytest.mark.parametrize("opname", ["stagder_v2p", "interpl_v2p"])
def test_tds_apply_xfft_on_15_pencils(opname):
    import torch
    from x3d2_amd import _lib
    from x3d2_amd.common import DIR_X, VERT
    if _lib.SINGLE:
        pytest.skip("the form is gated to FP64 (x3d_tds_solve_xfft_ok)")
    b, xd = _block()
    tol = _yardstick()
    op = getattr(xd, opname)
    assert b.tds_apply_xfft_ok(op)
    al = b.allocator
    u, plain, out = al.get_block(DIR_X, VERT), al.get_block(DIR_X, VERT), al.get_block(DIR_X, VERT)
    rng = np.random.default_rng(7 + len(opname))
    b.set_field_data(u, rng.standard_normal((DIMS[2], DIMS[1], DIMS[0])))
    b.tds_apply(plain, u, op, DIR_X)
    ref = xfft_ref.pack(b.get_field_data(plain, VERT))
    sentinel = -7.25
    out.data.fill_(sentinel)
    b.tds_apply_xfft(out, u, op)
    torch.cuda.synchronize()
    got = b.get_field_data(out, VERT)
    e = float(np.abs(got - ref).max() / np.abs(ref).max())
    _record(what="tds_apply_xfft vs pack(rfft(tds_apply))", op=opname, relerr=e, tolerance=tol)
    assert e <= tol, (e, tol)
    # the pad columns 512 .. 527 (and everything else of the block that is not a field point) are untouched
    written = int((out.data != sentinel).sum().item())
    assert written == NROWS * 512, (written, NROWS * 512)
    raw = out.data[:NROWS * b.padded_dims[0]].view(NROWS, b.padded_dims[0])
    assert b.padded_dims[0] == 528 and bool((raw[:, 512:] == sentinel).all())
    for f in (u, plain, out):
        al.release_block(f)


@gpu
def test_untangling_inverse_x_pass():
    from x3d2_amd import _lib
    if _lib.SINGLE:
        pytest.skip("the form is gated to FP64 (x3d_tds_solve_xfft_ok)")
    b, _ = _block()
    tol = _yardstick()
    rng = np.random.default_rng(99)
    # the packed forward transform on the host of two sets of real rows: the packed columns are complex once the z
    # transform has run over them, P = pack(r1) + i pack(r2), and untangle to fft(r1 + i r2)
    r1, r2 = rng.standard_normal((NROWS, 512)), rng.standard_normal((NROWS, 512))
    P = xfft_ref.pack(r1) + 1j * xfft_ref.pack(r2)
    H = xfft_ref.untangle(P)
    assert np.abs(H - np.fft.fft(r1 + 1j * r2, axis=1)).max() <= 1e-12 * np.abs(H).max()
    plain = _c2c_rows(b, H, 1)        # the parent's inverse on the unpacked spectrum
    got = _c2c_rows(b, P, 2)          # untangle + inverse
    e = float(np.abs(got - plain).max() / np.abs(plain).max())
    e_np = float(np.abs(got - 512.0 * (r1 + 1j * r2)).max() / (512.0 * np.abs(r1 + 1j * r2).max()))
    _record(what="k_c2c512_x<+1, UNT> vs k_c2c512_x<+1>", rows=NROWS, relerr=e, relerr_vs_rows=e_np, tolerance=tol)
    assert e <= tol and e_np <= tol, (e, e_np, tol)


@gpu
def test_pressure_correction_at_512_cubed_new_form_vs_plain():
    """one pressure_correction_fused on a broadband 512^3 velocity in the new form (here) and with X3D_NO_XFFT_DIV=1 (child):
    u, v, w agree to 1e-11 of the maximum (the project's bound for two forms of one solve), and max |div u| after the
    projection is no larger than twice the plain form's"""
    from x3d2_amd import _lib
    if _lib.SINGLE:
        pytest.skip("the form is gated to FP64 (x3d_tds_solve_xfft_ok)")
    import xfft_pc512_worker as wk
    assert os.environ.get("X3D_NO_XFFT_DIV") != "1", "this test compares the default against the switch"
    n = 512
    r, w = os.pipe()
    env = dict(os.environ, X3D_NO_XFFT_DIV="1")
    child = subprocess.Popen([sys.executable, os.path.join(HERE, "xfft_pc512_worker.py"), str(w), "0"], env=env,
                             pass_fds=(w,), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    os.close(w)
    case, got, after = wk.pressure_correction_512()   # (while the child works)
    s = case.solver
    assert s._xfft_div and s.n_zfirst == 1 and s.n_xfft_div == 1, (s._xfft_div, s.n_zfirst, s.n_xfft_div)
    del case, s
    ref = np.empty(3 * n ** 3 + 1, dtype=np.float64)
    view, have = memoryview(ref).cast("B"), 0
    with os.fdopen(r, "rb", buffering=0) as src:
        while have < len(view):
            k = src.readinto(view[have:])
            if not k:
                break
            have += k
    log = child.communicate(timeout=600)[0]
    assert child.returncode == 0 and have == len(view), log[-3000:]
    after_plain = float(ref[-1])
    errs = []
    for i, a in enumerate(got):
        o = ref[i * n ** 3:(i + 1) * n ** 3].reshape(n, n, n)
        errs.append(float(np.abs(a - o).max() / np.abs(o).max()))
    _record(what="pressure_correction_fused 512^3, new form vs X3D_NO_XFFT_DIV=1", relerr_uvw=errs,
            div_after_new=after, div_after_plain=after_plain)
    assert max(errs) <= 1e-11, errs
    assert after <= 2.0 * after_plain, (after, after_plain)
