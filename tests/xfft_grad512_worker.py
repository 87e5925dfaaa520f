"""child process of test_substep_pair_at_512_cubed_packed_gradient_vs_plain: on the ROUGH 512^3 velocity of
tests/pc512_worker.py one RK sub-step that is not the step's last (transeq, stage, pressure correction with its velocity
correction left pending), then the consumer of the pending gradient: the next sub-step's transeq ("transeq": the x kernel
applies it, csrc/xscan.hip k_xscan_transeq2x3<UPD>, <XINV> where the gradient stayed packed along x) or Solver.flush_grad
("flush": k_xscan_tds<ACC> / k_xscan_tds_ixfft), with whatever X3D_NO_XFFT_GRAD says in the environment (the switch is
resolved once per backend: hence a child).  u, v, w and max |div u| go to the file descriptor given on the command line as
raw float64: 3 n^3 values, then the divergence.

    python xfft_grad512_worker.py <fd> <transeq|flush> <expected Solver.n_xfft_grad>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def substep_pair_512(consumer):
    """-> (case, [u, v, w] once the pending correction is applied, max |div u| of that velocity)"""
    from util import noisy_tgv
    from x3d2_amd import make_tgv
    from x3d2_amd.common import DIR_X, DIR_Z, VERT
    n = 512
    dims = (n, n, n)
    data = [np.ascontiguousarray(a) for a in noisy_tgv(dims, (0, 0, 0), dims, amp=0.1)]
    case = make_tgv(n, fused=True)
    s = case.solver
    b, al = s.backend, s.backend.allocator
    for f, d in zip((s.u, s.v, s.w), data):
        f.set_data_loc(VERT)
        b.set_field_data(f, d)
    del data
    case.substep(1, last=False)
    assert s.pending_grad is not None, "the sub-step did not leave its velocity correction pending"
    if consumer == "transeq":
        deriv = [al.get_block(DIR_X) for _ in range(3)]
        s.transeq(deriv, [s.u, s.v, s.w])
        for f in deriv:
            al.release_block(f)
    else:
        s.flush_grad()
    assert s.pending_grad is None and not s.pending_grad_packed
    got = [b.get_field_data(f) for f in (s.u, s.v, s.w)]
    div_u = al.get_block(DIR_Z)
    s.divergence_v2p(div_u, s.u, s.v, s.w)
    after, _ = b.field_max_mean(div_u)
    al.release_block(div_u)
    return case, got, float(after)


def main():
    fd, consumer, want = int(sys.argv[1]), sys.argv[2], int(sys.argv[3])
    case, got, after = substep_pair_512(consumer)
    s = case.solver
    assert s.n_zfirst == 1 and s.n_xfft_div == 1 and s.n_xfft_grad == want, (s.n_zfirst, s.n_xfft_div, s.n_xfft_grad, want)
    with os.fdopen(fd, "wb") as out:
        for a in got:
            out.write(memoryview(np.ascontiguousarray(a, dtype=np.float64)).cast("B"))
        out.write(np.array([after], dtype=np.float64).tobytes())
    print("XFFT_GRAD512 %s n_xfft_grad=%d max|div u| after %.3e" % (consumer, s.n_xfft_grad, after), flush=True)


if __name__ == "__main__":
    main()
