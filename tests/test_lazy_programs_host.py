"""tests/lazy_programs.py without a GPU: the generator is constructive and deterministic, every (idiom, mutation) pair of
the module's table is there, every program runs on the CPU float64 model, BLAS-1 programs equal their closed form bit for
bit, programs survive JSON, the minimiser finds a planted pair."""
import re

import numpy as np
import pytest

import lazy_programs as lp
from util import OPNAMES

SEEDS = list(range(100))
GENERIC = ["S1", "D1"]


def test_vocabulary_names_the_eight_operators():
    assert lp.OPNAMES == list(OPNAMES)


@pytest.mark.parametrize("shape", GENERIC)
def test_enumerated_set_is_complete_and_runs_on_the_model(shape):
    """every idiom and every applicable (idiom, mutation) pair is a fixed, named program; the count is the table's"""
    progs = lp.enumerated(shape, model=True)  # (built ON the model: an exception here is a failure)
    names = [p["name"] for p in progs]
    want = [k + ("/" + m if m else "") for k in lp.idioms_for(shape) for m in [""] + lp.TABLE[k][2]]
    assert names == want and len(set(names)) == len(names) == lp.expected_count(shape)
    assert lp.expected_count("S1") == 317 and lp.expected_count("D1") == 310  # (D1: no 000 Poisson solver, no rule 7)
    assert set(lp.CONTROLS) == set(lp.TABLE)
    for p in progs:
        lp.check(p)
        lp.Model(shape).run(p)  # ... and replays from its printed form
    for k, (_, _, muts, _) in lp.TABLE.items():
        assert len(set(muts)) == len(muts), k


def test_every_mutation_class_is_applied_to_every_idiom_or_has_a_reason():
    """per idiom: each of M1 .. M10 has at least one program, or NOT_APPLICABLE says why it cannot have one"""
    for idiom, (_, _, muts, _) in lp.TABLE.items():
        have = {re.match(r"M\d+", m).group(0) for m in muts}
        why = lp.NOT_APPLICABLE.get(idiom.split(":")[0], {})
        for k in range(1, 11):
            assert "M%d" % k in have or why.get("M%d" % k), (idiom, "M%d" % k)
    # the same kind of pattern carries the same mutations: the species form of rule 1 everything of rule 1 that one sum
    # allows, both forms of rule 10 the same list, every form of rule 6 the coefficient positions of the chain it consumes
    one_sum = [m for m in lp.R1M if m not in lp.M8P + ["M4acc", "M10two"]]
    assert set(one_sum) <= set(lp.R1BM) and "M4uvw" in lp.R1BM
    assert lp.TABLE["r10:save"][2] == lp.TABLE["r10:plain"][2]
    for k in ("r6:plain", "r6:face", "r6:ring"):
        assert set(lp.R6C + lp.M9 + ["M10six"]) <= set(lp.TABLE[k][2]), k
    assert set(lp.M9) <= set(lp.TABLE["r8"][2])


@pytest.mark.parametrize("shape", GENERIC)
def test_random_programs_are_constructive_deterministic_and_bounded(shape):
    """no seed of the list is skipped, no candidate discarded: every seed yields one valid program of at most 48 ops that
    runs on the model; the same seed gives the same program; the conditioning keeps every handle O(1)"""
    idiom_ops = 0
    for seed in SEEDS:
        p, B = lp.random_program(shape, seed)
        assert 1 <= len(p["ops"]) <= lp.MAXLEN and p["seed"] == seed
        lp.check(p)
        if seed % 5 == 0:
            assert lp.dumps(lp.random_program(shape, seed)[0]) == lp.dumps(p)
        for h in B.sym.defined():
            chain, scale = B.model.meta[h]
            assert chain <= 9 and 1e-3 <= B.model.norm(h) <= 1e3, (seed, h, chain)
        idiom_ops += sum(op[0] in ("transeq", "species", "tds", "fft_fwd") for op in p["ops"])
    assert idiom_ops > 2 * len(SEEDS)  # (the programs are not just BLAS-1)


def test_json_round_trip_is_the_identity():
    for p in lp.enumerated("S1") + [lp.random_program("S1", s)[0] for s in range(10)]:
        q = lp.loads(lp.dumps(p))
        assert q == p and lp.dumps(q) == lp.dumps(p)
    assert lp.loads(lp.dumps({"c": lp.NA}))["c"] == np.nextafter(1.0, 2.0)


def _blas1_program(seed):
    rng = np.random.default_rng(seed)
    B = lp.Builder("S1", "blas%d" % seed, rng=rng, model=True)
    B.rng = None  # (fresh handles)
    hs = [B.pick() for _ in range(3)]
    B.rng = rng
    for _ in range(25):
        x, y = (int(v) for v in rng.choice(hs, 2))
        k = int(rng.integers(6))
        if k == 0:
            B.emit("vecadd", float(rng.choice([0.5, -1.0, lp.NA, 0.0])), x, float(rng.choice([1.0, -0.5])), y)
        elif k == 1:
            B.emit("vecmult", y, x)
        elif k == 2:
            B.emit("scale", x, 0.75)
        elif k == 3:
            B.emit("shift", x, -0.25)
        elif k == 4:
            h = B.new("x")
            B.emit("veccopy", h, x)
            hs.append(h)
        else:
            h = B.new("y")
            B.emit("reorder", h, x)
            g = B.new("x")
            B.emit("reorder", g, h)
            B.emit("sum", "y", y, h)
            hs.append(g)
    return B


@pytest.mark.parametrize("seed", range(5))
def test_model_equals_the_closed_form_on_blas1_programs(seed):
    B = _blas1_program(seed)
    want = lp.closed_form(B.program(), lp.SHAPES["S1"]["dims"])
    for h in B.sym.defined():
        assert np.array_equal(B.model.get(h), want[h]), h


def test_the_symbolic_check_refuses_what_the_eager_backend_refuses():
    for ops in ([["get", 0, "x"], ["scale", 0, 2.0]],                                              # undefined read
                [["get", 0, "x"], ["upload", 0, 1, 0], ["get", 1, "y"], ["vecadd", 1.0, 0, 1.0, 1]],  # DIR mismatch
                [["get", 0, "x"], ["upload", 0, 1, 0], ["tds", 0, 0, "der1st"]],                    # in place
                [["get", 0, "x"], ["upload", 0, 1, 0], ["get", 1, "x"], ["tds", 1, 0, "interpl_p2v"]],  # p2v at VERT
                [["get", 0, "x"], ["rel", 0], ["obs_get", 0]]):
        with pytest.raises(lp.Invalid):
            lp.check({"name": "bad", "shape": "S1", "ops": ops})


def test_minimiser_shrinks_a_planted_failure_to_the_planted_ops():
    p, _ = lp.random_program("S1", 7)
    planted = [op for op in p["ops"] if op[0] == "upload"][:2]
    assert len(planted) == 2
    calls = []

    def fails(cand):  # the fake executor "fails" when both planted ops are present
        calls.append(1)
        return all(op in cand["ops"] for op in planted)

    small, runs = lp.minimise(p, fails, budget=200)
    assert runs == len(calls) <= 200
    kept = [op for op in small["ops"] if op[0] != "get"]
    assert kept == planted and len(small["ops"]) == 4, small["ops"]  # (the two uploads and the blocks they need)
    lp.check(small)
