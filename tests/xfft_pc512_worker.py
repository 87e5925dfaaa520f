"""child process of test_pressure_correction_at_512_cubed_new_form_vs_plain: one pressure_correction_fused on the ROUGH 512^3
velocity of tests/pc512_worker.py (Taylor-Green + 10 % noise: every wave number present), with whatever X3D_NO_XFFT_DIV says
in the environment (the switch is resolved once per backend: hence a child).  u, v, w and max |div u| after the projection
go to the file descriptor given on the command line as raw float64: 3 n^3 values, then the divergence.

    python xfft_pc512_worker.py <fd> <expected Solver.n_xfft_div>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def pressure_correction_512():
    """-> (solver, [u, v, w] after one pressure_correction_fused, max |div u| after it)"""
    from util import noisy_tgv
    from x3d2_amd import make_tgv
    from x3d2_amd.common import DIR_Z, VERT
    n = 512
    dims = (n, n, n)
    data = [np.ascontiguousarray(a) for a in noisy_tgv(dims, (0, 0, 0), dims, amp=0.1)]
    case = make_tgv(n, fused=True)
    s = case.solver
    b, al = s.backend, s.backend.allocator
    for f, d in zip((s.u, s.v, s.w), data):
        f.set_data_loc(VERT)
        b.set_field_data(f, d)
    s.pressure_correction_fused(s.u, s.v, s.w)
    got = [b.get_field_data(f) for f in (s.u, s.v, s.w)]
    div_u = al.get_block(DIR_Z)
    s.divergence_v2p(div_u, s.u, s.v, s.w)
    after, _ = b.field_max_mean(div_u)
    al.release_block(div_u)
    return case, got, float(after)


def main():
    fd, want = int(sys.argv[1]), int(sys.argv[2])
    case, got, after = pressure_correction_512()
    s = case.solver
    assert s.n_zfirst == 1 and s.n_xfft_div == want, (s.n_zfirst, s.n_xfft_div, want)
    with os.fdopen(fd, "wb") as out:
        for a in got:
            out.write(memoryview(np.ascontiguousarray(a, dtype=np.float64)).cast("B"))
        out.write(np.array([after], dtype=np.float64).tobytes())
    print("XFFT_PC512 n_xfft_div=%d max|div u| after %.3e" % (s.n_xfft_div, after), flush=True)


if __name__ == "__main__":
    main()
