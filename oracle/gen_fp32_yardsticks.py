#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: write tests/golden/fp32_yardsticks_full_size.json -- the FP32 yardstick (tests/fp32_ref.py: the oracle's
Poisson solve as a correctly rounded FP32 pipeline, its error against the FP64 solve of the same float32 right-hand side,
L2-relative and max norm relative to the solution's maximum) of the two Poisson cases whose kernel paths engage only at full
size, so that the GPU box does not pay minutes of host transforms for two numbers:

  000.512x512x512               the z-first solve, the x-first solve with the single-kernel r2c x pass, the y-slab solver
  010.1024x257x512.top-bottom   the channel's 010 solve, x-first and z-first rows

(tests/test_hip_single_prec.py holds the FP32 library to fp32_ref.BOUND x these numbers.)  A yardstick is a statistic of
the case, not of the draw; shape, stretching and seed are stored with it all the same.  A yardstick above fp32_ref.CAP is a
badly chosen input and is not written.

    python oracle/gen_fp32_yardsticks.py [tag ...]       (~25 GB of memory, tens of seconds of host time)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fp32_ref  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "fp32_yardsticks_full_size.json")


def main():
    want = sys.argv[1:] or list(fp32_ref.FULL_SIZE)
    out = {}
    if os.path.exists(PATH):
        with open(PATH) as fh:
            out = json.load(fh)
    for tag in want:
        case, dims, L, stretching, beta, seed = fp32_ref.FULL_SIZE[tag]
        t0 = time.perf_counter()
        pf = fp32_ref.oracle_poisson(tag)
        (l2, mx), _ = fp32_ref.yardstick(pf, fp32_ref.rhs_of(tag))
        del pf
        print("%-30s l2 %.4e max %.4e   %.1f s" % (tag, l2, mx, time.perf_counter() - t0), flush=True)
        if not mx <= fp32_ref.CAP:
            raise SystemExit("%s: yardstick %.3e above the cap %.0e: nothing written" % (tag, mx, fp32_ref.CAP))
        out[tag] = {"case": case, "dims": list(dims), "L": list(L), "stretching": stretching, "beta": beta, "seed": seed,
                    "l2": l2, "max": mx}
        with open(PATH, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print("wrote", PATH)


if __name__ == "__main__":
    main()
