"""The FP32 yardstick of the Poisson paths (tests/fp32_ref.py), on the host:
  cap          the yardstick of every case the GPU tests use stays below fp32_ref.CAP in max norm -- a condition on the
               inputs (zero mean, no degenerate mode excited), not a measurement of anything;
  sensitivity  the same pipeline with ONE table off by a relative 1e-5 at pseudo-random entries exceeds the acceptance
               bound: a path is accepted when BOTH its norms stay within fp32_ref.BOUND x the yardstick, so exceeding it
               in one norm is a rejection (the L2 norm does in every case; the max norm, which a few low modes dominate, in
               most): the bound the GPU tests assert can fail."""
import json
import os

import numpy as np
import pytest

import fp32_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _table_in_use(pf):
    """the table the division (or the pentadiagonal solve) of this case reads; the symmetric stretchings keep theirs as two
    arrays, the odd and the even rows' systems.  (What the bound resolves: a_odd alone off by 1e-5 at half of its entries
    moves the 32 x 257 x 16 top-bottom solution by 7.8 x the yardstick in L2, just inside the bound; both arrays by 47 x.)"""
    if pf.case == "100":
        return ("waves100",)
    if pf.case == "110":
        return ("waves110",)
    if pf.stretched_y:
        return ("a_odd", "a_even") if pf.stretched_y_sym else ("a_full",)
    return ("waves",)


@pytest.mark.parametrize("tag", sorted(fp32_ref.CASES))
def test_yardstick_is_capped_and_the_acceptance_bound_can_fail(tag):
    pf = fp32_ref.oracle_poisson(tag)
    f = fp32_ref.rhs_of(tag)
    assert f.dtype == np.float32 and f.shape == (pf.nz, pf.ny, pf.nx) and abs(float(f.mean(dtype=np.float64))) < 1e-7
    (l2, mx), ref = fp32_ref.yardstick(pf, f)
    print("yardstick %-28s l2 %.3e max %.3e" % (tag, l2, mx))
    assert np.all(np.isfinite(ref))
    assert l2 > 1e-8 and 1e-8 < mx <= fp32_ref.CAP, (tag, l2, mx)  # (below 1e-8 the pipeline would not be rounding to FP32 at all)
    # the tables were put back: the FP64 solve gives the same bits as before
    assert np.array_equal(pf.solve(f.astype(np.float64)), ref)
    (pl2, pmx), _ = fp32_ref.yardstick(pf, f, perturbed=(_table_in_use(pf), 1e-5))
    print("perturbed %-28s l2 %.3e max %.3e  (x %.1f, x %.1f)" % (tag, pl2, pmx, pl2 / l2, pmx / mx))
    assert not fp32_ref.accepted((pl2, pmx), (l2, mx)), (tag, pl2 / l2, pmx / mx)
    assert pl2 > fp32_ref.BOUND * l2, (tag, pl2 / l2)


def test_stored_full_size_yardsticks():
    """the two full-size cases' yardsticks (oracle/gen_fp32_yardsticks.py): present, for the shapes and seeds of
    fp32_ref.FULL_SIZE, and under the same cap"""
    with open(os.path.join(HERE, "golden", "fp32_yardsticks_full_size.json")) as fh:
        stored = json.load(fh)
    assert sorted(stored) == sorted(fp32_ref.FULL_SIZE)
    for tag, (case, dims, _, stretching, beta, seed) in fp32_ref.FULL_SIZE.items():
        y = stored[tag]
        assert (y["case"], tuple(y["dims"]), y["stretching"], y["beta"], y["seed"]) == (case, dims, stretching, beta, seed)
        assert y["l2"] > 1e-8 and 1e-8 < y["max"] <= fp32_ref.CAP, (tag, y)
