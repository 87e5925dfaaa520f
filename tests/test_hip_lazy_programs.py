"""Generated call sequences through the deferred-execution layer (csrc/lazy.hip; generator, model and minimiser in
tests/lazy_programs.py, the executor in tests/lazy_fuzz_worker.py).  What test_hip_lazy.py runs through the rewriter is
the solver's own sequences; here every rewrite's pattern is run unmutated (its counter must fire) and with each guard's
precondition broken one at a time -- a temporary read once more, an accumulator that is also an input, an operand aliased
to the same buffer, a coefficient that is not exactly 1, a flush in the middle ... -- plus seeded random interleavings:
  1. lazy == eager bit for bit (FP64 and FP32; S1 = 20 x 12 x 16 periodic, D1 = 24 x 17 x 16 Dirichlet + stretched y);
  2. eager and lazy against the CPU float64 model, max|got - model| <= 1e-12 (1 + chain) scale per handle;
  3. positive controls: the unmutated idioms raise their counters, `declined` and `materialised` stay 0;
  4. the fast-path shape F1 (256-point x pencils, 256 rows in z: rules 8 and 10 engage), lazy against eager within the
     bound of 2. and bit for bit with the pair rewrites masked;
  5. after x3d_lazy_sync every block holds its handle's data (every program of 1.), and ten runs in a row leave
     `extra_buffers` where it stood after the second.
Each test is one worker process; X3D_LAZY_PROFILE=<file> appends one line per test (programs, worst ratio, seconds)."""
import json
import os
import subprocess
import sys
import time

import pytest

import lazy_programs as lp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NOPAIRS = str(0xFFFF - 2 - 4)  # X3D_LAZY_RULES: every rewrite but the two pair rewrites (rules 2 and 3)


def _worker(request, tmp_path, args, single=False, rules=None, timeout=300):
    env = dict(os.environ)
    for k in ("X3D_SINGLE_PREC", "X3D_LAZY_RULES", "X3D_LAZY_KEEP_ZERO_TERMS", "X3D_LAZY"):
        env.pop(k, None)
    if single:
        env["X3D_SINGLE_PREC"] = "1"
    if rules is not None:
        env["X3D_LAZY_RULES"] = rules
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "lazy_fuzz_worker.py"), "run"] + args + ["--tmp", str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=timeout)
    seconds = time.time() - t0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    tail = "\n".join([ln for ln in r.stdout.splitlines() if not ln.startswith("PROG ")][-30:]) + "\n" + r.stderr[-3000:]
    assert lines, "the worker ended without a RESULT line (exit status %d)\n%s" % (r.returncode, tail)
    res = json.loads(lines[-1][len("RESULT "):])
    prof = os.environ.get("X3D_LAZY_PROFILE")
    if prof:
        with open(prof, "a") as fh:
            fh.write(json.dumps({"test": request.node.name, "programs": res.get("programs"), "worst_model_ratio": res.get("ratio"),
                                 "worst_lazy_vs_eager_ratio": res.get("lazy_vs_eager"), "seconds": round(seconds, 2),
                                 "ok": res.get("ok")}) + "\n")
    assert r.returncode == 0 and res["ok"], tail
    assert res["single"] == single, "the worker did not run the %s library" % ("FP32" if single else "FP64")
    return res


@pytest.mark.parametrize("shape", ["S1", "D1"])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_enumerated_programs_lazy_equals_eager(request, tmp_path, shape, prec):
    """every idiom and every (idiom, mutation) pair: lazy == eager bit for bit at every observer and at the end, every
    block home after x3d_lazy_sync; FP64 also against the model; every unmutated idiom fires its counter"""
    res = _worker(request, tmp_path, [shape, "enum"] + (["--model"] if prec == "fp64" else []), single=prec == "fp32")
    assert res["programs"] == lp.expected_count(shape)
    assert res["controls"] == len(lp.idioms_for(shape)) and not res["controls_failed"], res["controls_failed"]
    assert prec == "fp32" or 0.0 < res["ratio"] <= 1.0


SEEDS = [(0, 50), (50, 100)]


@pytest.mark.parametrize("seeds", SEEDS, ids=["%d-%d" % s for s in SEEDS])
@pytest.mark.parametrize("shape", ["S1", "D1"])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_random_programs_lazy_equals_eager(request, tmp_path, shape, prec, seeds):
    """100 seeds per shape, up to 48 ops each: bit for bit, home after sync; FP64 also against the model"""
    res = _worker(request, tmp_path, [shape, "random", "--seeds", "%d:%d" % seeds] + (["--model"] if prec == "fp64" else []),
                  single=prec == "fp32")
    assert res["programs"] == seeds[1] - seeds[0]
    assert prec == "fp32" or 0.0 < res["ratio"] <= 1.0


FAST_GROUPS = [[k for k in lp.FAST_IDIOMS if k.split(":")[0] in g] for g in (("r1", "r2"), ("r3", "r4"), ("r6", "r8", "r10"))]
FAST_IDS = ["r1-r2", "r3-r4", "r6-r8-r10"]


@pytest.mark.parametrize("idioms", FAST_GROUPS, ids=FAST_IDS)
def test_fast_path_shape_within_the_model_bound(request, tmp_path, idioms):
    """F1: the pair rewrites move sums onto the tile kernels (1-2 ulp against the single solves, test_hip_lazy.py), so lazy
    against eager within the bound of the model check; both against the model; rules 8 and 10 must really engage"""
    res = _worker(request, tmp_path, ["F1", "fast:" + ",".join(idioms), "--model", "--bound"])
    assert res["programs"] == lp.expected_count("F1", idioms) and res["controls"] == len(idioms), res
    assert not res["controls_failed"], res["controls_failed"]
    assert 0.0 < res["ratio"] <= 1.0 and res["lazy_vs_eager"] <= 1.0


@pytest.mark.parametrize("idioms", FAST_GROUPS, ids=FAST_IDS)
def test_fast_path_shape_bit_for_bit_without_the_pair_rewrites(request, tmp_path, idioms):
    """F1 with rules 2 and 3 masked (X3D_LAZY_RULES, as test_deferred_run_with_the_distributed_poisson_solvers_forced
    masks them): bit for bit"""
    res = _worker(request, tmp_path, ["F1", "fast:" + ",".join(idioms)], rules=NOPAIRS)
    assert res["programs"] == lp.expected_count("F1", idioms) and not res["controls_failed"], res


def test_rule_8_on_generic_pencils_runs_the_four_calls_it_stands_for(request, tmp_path):
    """S1: x3d_transeq_x_update declines 20-point pencils and exec() runs three accumulating solves and transeq_x"""
    res = _worker(request, tmp_path, ["S1", "fast:r8"])
    # CONTROLS["r8"]: ONE launched operation (the fused one; unfused there are four) with six ops dropped behind the
    # rewrite, and inside it the fallback's counters: tds_acc 3, transeq_upd 0
    want = lp.CONTROLS["r8"]
    assert want["launched"] == 1 and want["dropped"] == 6 and want["tds_acc"] == 3 and want["transeq_upd"] == 0
    assert res["controls"] == 1 and not res["controls_failed"], res


@pytest.mark.parametrize("shape", ["S1", "D1"])
def test_ten_runs_in_a_row_leave_no_buffer_behind(request, tmp_path, shape):
    res = _worker(request, tmp_path, [shape, "leak", "--seeds", "0:20"])
    assert res["programs"] == lp.expected_count(shape) + 20 and not res["leaks"], res["leaks"]
