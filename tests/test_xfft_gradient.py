"""The z-first 000 solve without its inverse x pass: the last three x operators of gradient_c2v take their fields still
transformed along x, packed half-complex, and invert the transform on the pencil the wave holds (csrc/fft512_core.h
irfft512_packed_wave; csrc/xscan.hip k_xscan_tds_ixfft and k_xscan_transeq2x3<XINV>; csrc/zfirst.hip
x3d_poisson_zfirst_middle_xpacked2; X3D_NO_XFFT_GRAD=1 restores the sequence with the pass).
tests/test_xfft_gradient_host.py pins the algebra on the CPU; here the kernels:

  * tds_apply_ixfft on 15 pencils and on a count whose last trip is short, against the plain accumulating tds_apply on
    512 x the rows; pad columns of u and all of g untouched;
  * transeq_x_update_xinv on 9 pairs and on a count whose last trip is short, against transeq_x_update on 512 x the rows;
  * equal bits between transeq_x_update_xinv and three tds_apply_ixfft followed by the plain transeq along x;
  * one sub-step pair at 512^3 on a broadband velocity against the same with X3D_NO_XFFT_GRAD=1 in a child process.

The kernel tolerance is measured, not fixed: the error of the plain inverse pass k_c2c512_x<+1> against 512 numpy.fft.ifft
on 15 random rows relative to the largest value, times 4 (the margin the forward test gives a real transform for its extra
stage).  With X3D_TEST_WRITE_PROFILES=1 the measured numbers are appended to profiles/xfft_grad.jsonl."""
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
PX = 520  # row pitch of the yardstick's rows in complex numbers (the solver's ZH_PX)
NU = 1.0 / 1600.0
_state = {}


def _record(**kw):
    print("xfft_grad:", json.dumps(kw))
    if os.environ.get("X3D_TEST_WRITE_PROFILES") == "1":
        with open(os.path.join(os.path.dirname(HERE), "profiles", "xfft_grad.jsonl"), "a") as fh:
            fh.write(json.dumps(kw) + "\n")


def _skip_single():
    from x3d2_amd import _lib
    if _lib.SINGLE:
        pytest.skip("the form is gated to FP64 (x3d_tds_solve_ixfft_ok)")


def _block(dims):
    """-> (backend, x operators) of a periodic 512 x ny x nz block (no solver: y and z are too short for operators)"""
    if dims not in _state:
        from x3d2_amd import Mesh
        from x3d2_amd.backend import HipBackend
        from x3d2_amd.common import DIR_X
        from x3d2_amd.solver import allocate_tdsops
        from x3d2_amd.tdsops import Dirps
        per = ("periodic",) * 2
        mesh = Mesh(dims, (1, 1, 1), (2.0 * np.pi, 1.0, 1.0), per, per, per)
        b = HipBackend(mesh)
        xd = Dirps(DIR_X)
        allocate_tdsops(xd, b, mesh, "compact6", "compact6", "classic", "compact6")
        _state[dims] = (b, xd)
    return _state[dims]


def _yardstick():
    """the plain inverse pass against 512 numpy.fft.ifft on 15 random rows: max error relative to the largest value"""
    if "tol" not in _state:
        import torch
        from x3d2_amd import _lib
        b, _ = _block((512, 3, 5))
        nrows = 15
        rng = np.random.default_rng(1512)
        rows = rng.standard_normal((nrows, 512)) + 1j * rng.standard_normal((nrows, 512))
        ref = 512.0 * np.fft.ifft(rows, axis=1)
        buf = torch.zeros((nrows, PX), dtype=torch.complex128, device=b.device)
        buf[:, :512] = torch.from_numpy(rows).to(b.device)
        _lib.check(b.lib.x3d_c2c512_x_rows(b.h, ctypes.c_void_p(buf.data_ptr()), nrows, PX, 1))
        torch.cuda.synchronize()
        e = float(np.abs(buf[:, :512].cpu().numpy() - ref).max() / np.abs(ref).max())
        assert 0.0 < e < 1e-13, e  # (a 512-point FP64 transform: a few eps sqrt(log n); anything else is a broken yardstick)
        _state["tol"] = 4.0 * e
        _record(what="k_c2c512_x<+1> vs 512 numpy.fft.ifft", rows=nrows, relerr=e, tolerance=4.0 * e)
    return _state["tol"]


def _rows(rng, dims):
    """random rows r scaled so that 512 r is of order one (the size of the velocity it corrects) -> (512 r, pack(r))"""
    r = rng.standard_normal((dims[2], dims[1], dims[0])) / 512.0
    return 512.0 * r, xfft_ref.pack(r)


def _ixfft_case(dims, opname, seed):
    """tds_apply_ixfft(u, pack(r), op, -1) against tds_apply(u, 512 r, op, accumulate, -1) on a copy -> error relative to
    the largest update; the pad columns of u and the whole of g must stay"""
    import torch
    from x3d2_amd.common import DIR_X, VERT
    b, xd = _block(dims)
    op = getattr(xd, opname)
    assert b.tds_apply_ixfft_ok(op)
    npen = dims[1] * dims[2]
    al = b.allocator
    u, uref, g, r512 = (al.get_block(DIR_X, VERT) for _ in range(4))
    rng = np.random.default_rng(seed)
    full, packed = _rows(rng, dims)
    u_old = rng.standard_normal((dims[2], dims[1], dims[0]))
    sentinel = -7.25
    for f in (u, uref, g):
        f.data.fill_(sentinel)
    b.set_field_data(u, u_old)
    b.set_field_data(uref, u_old)
    b.set_field_data(g, packed)
    b.set_field_data(r512, full)
    g_before = g.data.clone()
    b.tds_apply(uref, r512, op, DIR_X, accumulate=True, scale=-1.0)
    b.tds_apply_ixfft(u, g, op, -1.0)
    torch.cuda.synchronize()
    got, ref = b.get_field_data(u, VERT), b.get_field_data(uref, VERT)
    e = float(np.abs(got - ref).max() / np.abs(ref - u_old).max())
    # pad columns 512 .. 527 of u (and everything else of the block that is not a field point) and all of g untouched
    assert int((u.data != sentinel).sum().item()) == npen * 512
    nxp = b.padded_dims[0]
    assert nxp == 528 and bool((u.data[:npen * nxp].view(npen, nxp)[:, 512:] == sentinel).all())
    assert torch.equal(g.data, g_before)
    for f in (u, uref, g, r512):
        al.release_block(f)
    return e


@gpu
@pytest.mark.parametrize("opname", ["stagder_p2v", "interpl_p2v"])
def test_tds_apply_ixfft_on_15_pencils(opname):
    """512 x 3 x 5 = 15 pencils: two workgroups, the second with 7 of 8 waves busy (tail and prefetch guard)"""
    _skip_single()
    tol = _yardstick()
    e = _ixfft_case((512, 3, 5), opname, 11 + len(opname))
    _record(what="tds_apply_ixfft vs tds_apply(512 r, accumulate)", pencils=15, op=opname, relerr=e, tolerance=tol)
    assert e <= tol, (e, tol)


@gpu
def test_tds_apply_ixfft_on_a_count_with_a_tail():
    """x3d_xscan_tds_ixfft launches min(1024, ceil(np / 8)) workgroups of 8 waves, a pencil per wave and trip.  The
    512 x 65 x 64 block (4160 pencils) gives 520 workgroups and exactly one trip for every wave: no tail, so the count
    here is 512 x 65 x 127 = 8255 pencils: 1024 workgroups = 8192 waves take a full first trip, the waves 0 .. 62 (the
    workgroups 0 .. 7, the last of them with 7 of 8 waves busy) a second one, for which the prefetch guard let the
    first trip's loads through and stops the second trip's."""
    _skip_single()
    tol = _yardstick()
    e = _ixfft_case((512, 65, 127), "interpl_p2v", 65127)
    _record(what="tds_apply_ixfft vs tds_apply(512 r, accumulate)", pencils=8255, op="interpl_p2v", relerr=e, tolerance=tol)
    assert e <= tol, (e, tol)


def _upd_fields(dims, seed):
    """-> (backend, xd, dict of device blocks, host u_old list): u, v, w random, g* = pack(r*), f* = 512 r*"""
    from x3d2_amd.common import DIR_X, VERT
    b, xd = _block(dims)
    al = b.allocator
    rng = np.random.default_rng(seed)
    blk = {k: al.get_block(DIR_X, VERT) for k in ("u", "v", "w", "du", "dv", "dw", "gu", "gv", "gw", "fu", "fv", "fw")}
    old = []
    for c in "uvw":
        full, packed = _rows(rng, dims)
        uo = rng.standard_normal((dims[2], dims[1], dims[0]))
        old.append(uo)
        b.set_field_data(blk[c], uo)
        b.set_field_data(blk["g" + c], packed)
        b.set_field_data(blk["f" + c], full)
    return b, xd, blk, old


def _reset_velocity(b, blk, old):
    for c, uo in zip("uvw", old):
        b.set_field_data(blk[c], uo)
    for c in "uvw":
        blk["d" + c].data.zero_()


def _six(b, blk):
    from x3d2_amd.common import VERT
    return [b.get_field_data(blk[k], VERT) for k in ("u", "v", "w", "du", "dv", "dw")]


def _release(b, blk):
    for f in blk.values():
        b.allocator.release_block(f)


def _upd_case(dims, seed):
    """transeq_x_update_xinv on packed gradients against transeq_x_update on 512 x the rows -> the six relative errors
    (u, v, w, then the three rhs fields, each relative to its own maximum)"""
    b, xd, blk, old = _upd_fields(dims, seed)
    assert b.transeq_x_update_xinv_ok(xd.stagder_p2v, xd.interpl_p2v)
    assert b.transeq_x_update(blk["du"], blk["dv"], blk["dw"], blk["u"], blk["v"], blk["w"], NU, xd,
                              (blk["fu"], blk["fv"], blk["fw"]), xd.stagder_p2v, xd.interpl_p2v, -1.0)
    ref = _six(b, blk)
    _reset_velocity(b, blk, old)
    assert b.transeq_x_update_xinv(blk["du"], blk["dv"], blk["dw"], blk["u"], blk["v"], blk["w"], NU, xd,
                                   (blk["gu"], blk["gv"], blk["gw"]), xd.stagder_p2v, xd.interpl_p2v, -1.0)
    got = _six(b, blk)
    _release(b, blk)
    return [float(np.abs(a - o).max() / np.abs(o).max()) for a, o in zip(got, ref)]


@gpu
def test_transeq_x_update_xinv_on_9_pairs():
    """512 x 2 x 9 = 18 pencils = 9 pairs: two workgroups, the second with one busy wave"""
    _skip_single()
    tol = _yardstick()
    errs = _upd_case((512, 2, 9), 29)
    _record(what="transeq_x_update_xinv vs transeq_x_update(512 r)", pairs=9, relerr_uvw_rhs=errs, tolerance=tol)
    assert max(errs) <= tol, (errs, tol)


@gpu
def test_transeq_x_update_xinv_on_a_count_with_a_tail():
    """x3d_xscan_transeq3 launches min(256, ceil(pairs / 8)) workgroups (one per CU, x3d_persistent_blocks) of 8 waves, a
    pair per wave and trip: 512 x 65 x 64 = 4160 pencils = 2080 pairs want 260 workgroups and get 256 = 2048 waves -- one
    full trip, and a second one for the waves 0 .. 31 (workgroups 0 .. 3), whose prefetches of the next pair's u0 and
    packed gradient rows are the guarded ones."""
    _skip_single()
    tol = _yardstick()
    errs = _upd_case((512, 65, 64), 6564)
    _record(what="transeq_x_update_xinv vs transeq_x_update(512 r)", pairs=2080, relerr_uvw_rhs=errs, tolerance=tol)
    assert max(errs) <= tol, (errs, tol)


@gpu
def test_equal_bits_between_the_two_consumers_of_a_packed_gradient():
    """transeq_x_update_xinv against three tds_apply_ixfft + the plain transeq along x, on the same packed gradients:
    identical bits in u, v, w and the three rhs fields (the property the deferred / not-deferred pair has)"""
    _skip_single()
    from x3d2_amd.common import DIR_X
    dims = (512, 2, 9)
    b, xd, blk, old = _upd_fields(dims, 31)
    assert b.transeq_x_update_xinv(blk["du"], blk["dv"], blk["dw"], blk["u"], blk["v"], blk["w"], NU, xd,
                                   (blk["gu"], blk["gv"], blk["gw"]), xd.stagder_p2v, xd.interpl_p2v, -1.0)
    one = _six(b, blk)
    _reset_velocity(b, blk, old)
    b.tds_apply_ixfft(blk["u"], blk["gu"], xd.stagder_p2v, -1.0)
    b.tds_apply_ixfft(blk["v"], blk["gv"], xd.interpl_p2v, -1.0)
    b.tds_apply_ixfft(blk["w"], blk["gw"], xd.interpl_p2v, -1.0)
    b.transeq_dir(DIR_X, blk["du"], blk["dv"], blk["dw"], blk["u"], blk["v"], blk["w"], NU, xd, accumulate=False)
    two = _six(b, blk)
    _release(b, blk)
    for name, a, o in zip(("u", "v", "w", "du", "dv", "dw"), one, two):
        assert np.array_equal(a, o), (name, float(np.abs(a - o).max()))


def _child(consumer, want, env):
    """start tests/xfft_grad512_worker.py -> (process, read end of its pipe)"""
    r, w = os.pipe()
    child = subprocess.Popen([sys.executable, os.path.join(HERE, "xfft_grad512_worker.py"), str(w), consumer, str(want)],
                             env=env, pass_fds=(w,), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    os.close(w)
    return child, r


@gpu
def test_substep_pair_at_512_cubed_packed_gradient_vs_plain():
    """one RK sub-step that leaves its velocity correction pending + the next transeq on a broadband 512^3 velocity, in
    the new form (here) and with X3D_NO_XFFT_GRAD=1 (child): u, v, w agree to 1e-11 of the maximum (the project's bound for
    two forms of one solve), max |div u| of the corrected velocity is no larger than twice the plain form's, and
    n_xfft_grad == 1; a flush_grad() in place of the second transeq gives a velocity within the same bound."""
    _skip_single()
    import xfft_grad512_worker as wk
    assert os.environ.get("X3D_NO_XFFT_GRAD") != "1" and os.environ.get("X3D_NO_XFFT_DIV") != "1", \
        "this test compares the default against the switch"
    n = 512
    child, r = _child("transeq", 0, dict(os.environ, X3D_NO_XFFT_GRAD="1"))
    case, got, after = wk.substep_pair_512("transeq")   # (while the child works)
    s = case.solver
    assert s._xfft_grad and s.n_zfirst == 1 and s.n_xfft_div == 1 and s.n_xfft_grad == 1, \
        (s._xfft_grad, s.n_zfirst, s.n_xfft_div, s.n_xfft_grad)
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

    def errs_of(fields):
        out = []
        for i, a in enumerate(fields):
            o = ref[i * n ** 3:(i + 1) * n ** 3].reshape(n, n, n)
            out.append(float(np.abs(a - o).max() / np.abs(o).max()))
        return out
    errs = errs_of(got)
    del got
    case, got_f, after_f = wk.substep_pair_512("flush")
    assert case.solver.n_xfft_grad == 1
    del case
    errs_f = errs_of(got_f)
    _record(what="sub-step pair 512^3, packed gradient vs X3D_NO_XFFT_GRAD=1", relerr_uvw_transeq=errs,
            relerr_uvw_flush=errs_f, div_after_new=after, div_after_flush=after_f, div_after_plain=after_plain)
    assert max(errs) <= 1e-11, errs
    assert max(errs_f) <= 1e-11, errs_f
    assert after <= 2.0 * after_plain and after_f <= 2.0 * after_plain, (after, after_f, after_plain)
