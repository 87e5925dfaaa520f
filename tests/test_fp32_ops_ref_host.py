"""The FP32 yardstick of the compact operators (tests/fp32_ops_ref.py), on the host, for every case the GPU tests use:
  dtypes       the float32 pipeline stays in float32 (asserted inside apply32 / transeq32, and here on the results);
  cap          every yardstick -- operators, accumulating forms, pairs, transeq of the direction and of the solver -- stays below
               fp32_ops_ref.CAP in max norm: a condition on the inputs, not a measurement of anything;
  reference    the FP64 dense pipeline and the oracle agree to 1e-12 on every operator, pair, accumulating form and the
               direction's transeq, on the stretched cases too (the dense result times the oracle's stretch tables), so either
               can be the reference.  Solver.transeq is left out of this: its two short periodic directions (8 .. 16 points)
               are where the dense solve is no reference of the distributed algorithm (util.dense_operator);
  sensitivity  the pipeline with every off-diagonal of A, or the largest coefficient of row 1 of B, off by a relative 1e-5
               (the size of a table formed in FP32 arithmetic) exceeds BOUND x the yardstick in the max norm for every
               operator of every case: the bound the GPU tests assert can fail;
  old bounds   the same defects stay under the tolerances the FP32 operators were held to before (2e-5; 5e-4 for der2nd*),
               which is why the new bound exists.  One family is the exception and is asserted as such: the first derivatives
               of the Dirichlet cases with the defect in A.  Their one-sided closure (an off-diagonal of 2 in the first and
               last row of A) carries the defect to 2.4e-5 .. 3.1e-5 of the result's maximum at the wall, just above 2e-5."""
import numpy as np
import pytest

import fp32_ops_ref as ops_ref
import util

_pipelines = {}


def _pipeline(tag):
    if tag not in _pipelines:
        p = ops_ref.Pipeline(tag)
        _pipelines[tag] = (p, p.checks())
    return _pipelines[tag]


def test_case_table():
    """33 cases, the last 11 the count-edge cases (COUNTS); the inputs are float32 and differ between the cases and between
    the three fields"""
    assert len(ops_ref.CASES) == 33 and len({c[-1] for c in ops_ref.CASES.values()}) == 33
    assert list(ops_ref.CASES)[22:] == ops_ref.COUNTS
    for tag, (dims, d, bc, stretching, beta, L, seed) in ops_ref.CASES.items():
        u, v, w = ops_ref.inputs_of(tag)
        assert all(f.dtype == np.float32 and f.shape == dims[::-1] for f in (u, v, w)), tag
        assert not np.array_equal(u, v) and not np.array_equal(v, w), tag
        assert (stretching == "uniform") == (beta == 1.0), tag


@pytest.mark.parametrize("tag", list(ops_ref.CASES))
def test_yardsticks_are_float32_and_capped(tag):
    p, checks = _pipeline(tag)
    assert len(checks) == 8 + 8 + 6 + 3 + 3 + 3
    for name, (r32, r64) in checks.items():
        assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == r64.shape, (tag, name)
        assert np.all(np.isfinite(r64)), (tag, name)
        l2, mx = ops_ref.errors(r32, r64)
        print("yardstick %-36s %-34s l2 %.3e max %.3e" % (tag, name, l2, mx))
        assert l2 > 1e-8 and 1e-8 < mx <= ops_ref.CAP, (tag, name, l2, mx)  # (below 1e-8 nothing was rounded to FP32)


@pytest.mark.parametrize("tag", list(ops_ref.CASES))
def test_dense_solve_and_oracle_agree(tag):
    p, checks = _pipeline(tag)
    orc = ops_ref.oracle_results(p)
    assert sorted(orc) == sorted(checks)
    for name, (_, r64) in checks.items():
        if name.startswith("transeq."):
            continue
        e = util.relerr(r64, orc[name])
        assert orc[name].shape == r64.shape and e < 1e-12, (tag, name, e)


def _old_tolerance_catches(tag, defect, op):
    return defect == "A" and ".dirichlet." in tag and op in ("der1st", "der1st_sym")


@pytest.mark.parametrize("defect", ["A", "B"])
@pytest.mark.parametrize("tag", list(ops_ref.CASES))
def test_the_bound_rejects_a_1e_5_defect_that_the_old_tolerances_accept(tag, defect):
    p, checks = _pipeline(tag)
    q = ops_ref.Pipeline(tag, defect)
    for op in util.OPNAMES:
        r32, r64 = q.both(op, "u")
        assert r32.dtype == np.float32 and np.array_equal(r64, checks["tds." + op][1])  # (the defect is on the FP32 side only)
        err, yard = ops_ref.errors(r32, r64), ops_ref.errors(*checks["tds." + op])
        print("defect %s %-36s %-12s l2 %.3e (x %.1f) max %.3e (x %.1f)" % (defect, tag, op, err[0], err[0] / yard[0], err[1],
                                                                           err[1] / yard[1]))
        assert err[1] > ops_ref.BOUND * yard[1], (tag, defect, op, err[1] / yard[1])
        assert not ops_ref.accepted(err, yard)
        if _old_tolerance_catches(tag, defect, op):
            assert ops_ref.old_tolerance(op) < err[1] < 2 * ops_ref.old_tolerance(op), (tag, defect, op, err[1])
        else:
            assert err[1] < ops_ref.old_tolerance(op), (tag, defect, op, err[1])
