"""Worker of tests/test_hip_lazy_programs.py (one process per test, like tests/sp_worker.py; X3D_SINGLE_PREC and
X3D_LAZY_RULES come from the parent's environment): runs generated programs (tests/lazy_programs.py) on HipBackend(mesh)
and HipBackend(mesh, lazy=True) with the same uploads and compares, at every observer and at the end, every defined
handle's interior and every reduction value; optionally also against the CPU float64 model.

  python tests/lazy_fuzz_worker.py run SHAPE SET [--seeds A:B] [--model] [--bound] [--tmp DIR]
      SET: enum (every idiom x mutation), fast[:IDIOM,...] (the fast-path idioms, or some), random (the seeds A..B-1), leak
      --model: eager and lazy against the model, max|got - model| <= 1e-12 (1 + chain) scale per handle
      --bound: lazy against eager within that bound instead of bit for bit (pair rewrites on the tile kernels)
  python tests/lazy_fuzz_worker.py replay FILE     one saved program, in the precision / rules of the environment

One PROG line (JSON) per program, one RESULT line at the end; exit status 0 all equal, 1 a value mismatch (the program,
the first differing handle and op index and the lazy_stats() delta are printed, a greedy minimiser runs and the minimised
program is written to --tmp), 2 an X3dError (nothing further is started: no release, no flush, no orderly teardown of the
backends).  Reduction observers are compared with == only; --bound (fast-path sets, which hold none) refuses them."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import lazy_programs as lp  # noqa: E402
from x3d2_amd import Mesh, _lib  # noqa: E402
from x3d2_amd.backend import HipBackend  # noqa: E402
from x3d2_amd.common import Y_FACE, X3dError  # noqa: E402
from x3d2_amd.solver import Solver, SolverConfig  # noqa: E402

TOL = 1e-12  # tests/test_hip_parity.py holds one operator to it; every op on a chain gets that budget once


class Mismatch(Exception):
    def __init__(self, what, op_index, handle):
        Exception.__init__(self, what)
        self.what, self.op_index, self.handle = what, op_index, handle


class HipExec:
    """one backend (eager or deferred) of one shape, interpreting programs"""

    def __init__(self, shape, lazy, env=None):
        c = lp.SHAPES[shape]
        per = ("periodic",) * 2
        mesh = Mesh(tuple(c["dims"]), (1, 1, 1), tuple(c["L"]), per, (c["bc_y"],) * 2, per,
                    ("uniform", c["stretching"], "uniform"), (1.0, c["beta"], 1.0))
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            self.b = HipBackend(mesh, lazy=lazy)  # (the layer reads its switches when it is switched on)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        self.periodic = c["bc_y"] == "periodic"
        self.s = Solver(self.b, mesh, SolverConfig(poisson_solver_type="FFT" if self.periodic else "CG", fused=False))
        self.mesh, self.lazy = mesh, lazy
        self.dirps = {"x": self.s.xdirps, "y": self.s.ydirps, "z": self.s.zdirps}
        self.f, self.pf2, self.ptr = {}, None, {}

    def get(self, h):
        return self.b.get_field_data(self.f[h])

    def poisson(self, k):
        """0: the backend's own poisson_fft object; 1: a second one on the same backend"""
        if k == 0:
            return self.b.poisson_fft
        if self.pf2 is None:
            from x3d2_amd.poisson_fft import make_poisson_fft
            self.pf2 = make_poisson_fft(self.b, self.mesh, self.s.xdirps, self.s.ydirps, self.s.zdirps)
        return self.pf2

    def apply(self, op):
        k, a = op[0], op[1:]
        b, F, al = self.b, self.f, self.b.allocator
        if k == "get":
            F[a[0]] = al.get_block(lp.DIRN[a[1]])
            self.ptr[a[0]] = F[a[0]].ptr
        elif k == "rel":
            al.release_block(F.pop(a[0]))
        elif k == "upload":
            F[a[0]].set_data_loc(a[2])
            nx, ny, nz = (int(v) for v in self.mesh.get_dims(a[2]))
            b.set_field_data(F[a[0]], lp.field_data(a[1], nx, ny, nz))
        elif k == "veccopy":
            b.veccopy(F[a[0]], F[a[1]])
            F[a[0]].set_data_loc(F[a[1]].data_loc)
        elif k == "reorder":
            b.reorder(F[a[0]], F[a[1]], 10 * F[a[1]].dir + F[a[0]].dir)
        elif k == "vecadd":
            b.vecadd(a[0], F[a[1]], a[2], F[a[3]])
        elif k == "vecmult":
            b.vecmult(F[a[0]], F[a[1]])
        elif k == "scale":
            b.field_scale(F[a[0]], a[1])
        elif k == "shift":
            b.field_shift(F[a[0]], a[1])
        elif k == "sum":
            (b.sum_yintox if a[0] == "y" else b.sum_zintox)(F[a[1]], F[a[2]])
        elif k == "tds":
            b.tds_solve(F[a[0]], F[a[1]], getattr(self.dirps["xyz"[F[a[1]].dir - 1]], a[2]))
        elif k == "transeq":
            getattr(b, "transeq_" + a[0])(*[F[h] for h in a[1]], *[F[h] for h in a[2]], lp.NU, self.dirps[a[0]])
        elif k == "species":
            b.transeq_species(F[a[1]], F[a[2]], F[a[3]], lp.NU, self.dirps[a[0]])
        elif k == "setface":
            b.field_set_face_from_field(F[a[0]], F[a[1]], 0.0, Y_FACE)
        elif k == "fft_fwd":
            self.poisson(a[1]).fft_forward(F[a[0]])
        elif k == "fft_post":
            self.poisson(a[0]).fft_postprocess_000()
        elif k == "fft_bwd":
            self.poisson(a[1]).fft_backward(F[a[0]])
        elif k == "obs_get":
            return self.get(a[0])
        elif k == "obs_dot":
            return b.scalar_product(F[a[0]], F[a[1]])
        elif k == "obs_maxmean":
            return b.field_max_mean(F[a[0]])
        elif k == "lincomb":
            b.lincomb(F[a[0]], F[a[1]], a[2], [F[h] for h in a[3]])
            F[a[0]].set_data_loc(F[a[1]].data_loc)
        elif k == "flush":
            _lib.check(b.lib.x3d_lazy_flush(b.h))
        elif k == "sync":
            _lib.check(b.lib.x3d_lazy_sync(b.h))
        else:
            raise ValueError(k)
        return None

    def release_all(self):
        self.ptr = {}
        for h in sorted(self.f):
            self.b.allocator.release_block(self.f.pop(h))

    def home(self, sym):
        """after x3d_lazy_sync the raw memory of every block holds its handle's data"""
        import torch
        want = {h: self.get(h) for h in sym.defined()}
        _lib.check(self.b.lib.x3d_lazy_sync(self.b.h))
        torch.cuda.synchronize()
        nxp, nyp, nzp = self.b.padded_dims
        for h, w in want.items():
            nz, ny, nx = w.shape
            raw = self.f[h].data.cpu().numpy().reshape(nzp, nyp, nxp)[:nz, :ny, :nx]
            if not np.array_equal(raw, w):
                raise Mismatch("block %d is not home after x3d_lazy_sync" % h, -1, h)


_EXEC = {}


def backends(shape, env):
    key = (shape, tuple(sorted((env or {}).items())))
    if ("eager", shape) not in _EXEC:
        _EXEC[("eager", shape)] = HipExec(shape, False)
    if key not in _EXEC:
        _EXEC[key] = HipExec(shape, True, env)
    return _EXEC[("eager", shape)], _EXEC[key]


def _eq(x, y):
    if isinstance(x, np.ndarray):
        return np.array_equal(x, y)
    return x == y


def run_program(program, model=False, bound=False, home=True):
    """the program on both backends (and the model); returns {"ratio", "lazy_vs_eager", "stats"}; raises Mismatch"""
    shape = program["shape"]
    eager, lazy = backends(shape, program.get("env"))
    md = lp.Model(shape) if (model or bound) else None
    sym = md.sym if md is not None else lp.Sym()
    before = lazy.b.lazy_stats()
    worst = {"ratio": 0.0, "lazy_vs_eager": 0.0}

    def fields(idx):
        for h in sym.defined():
            e, g = eager.get(h), lazy.get(h)
            if md is not None:
                chain, scale = md.meta[h]
                lim = TOL * (1 + chain) * scale
            if bound:
                d = float(np.max(np.abs(e.astype(np.float64) - g))) / lim
                worst["lazy_vs_eager"] = max(worst["lazy_vs_eager"], d)
                if not d <= 1.0:
                    raise Mismatch("lazy vs eager: %.3g of the bound" % d, idx, h)
            elif not np.array_equal(e, g):
                raise Mismatch("lazy != eager, max |diff| %.3g" % float(np.max(np.abs(e.astype(np.float64) - g))), idx, h)
            if model:
                want = md.get(h)
                for who, got in (("eager", e), ("lazy", g)):
                    r = float(np.max(np.abs(got - want))) / lim
                    worst["ratio"] = max(worst["ratio"], r)
                    if not r <= 1.0:
                        raise Mismatch("%s vs model: %.3g of the bound (chain %d, scale %.3g)" % (who, r, chain, scale), idx, h)

    def tidy():
        eager.release_all()
        lazy.release_all()
        _lib.check(lazy.b.lib.x3d_lazy_flush(lazy.b.h))

    # (an X3dError -- how a failed HIP call surfaces -- passes through untouched: no release, no flush, nothing further
    #  reaches the GPU; only a value mismatch, after which the minimiser reuses the backends, tidies up)
    try:
        for idx, op in enumerate(program["ops"]):
            if md is not None:
                md.apply(op)
            else:
                sym.apply(op)
            ve, vl = eager.apply(op), lazy.apply(op)
            if op[0] in lp.OBSERVERS:
                if bound and op[0] in ("obs_dot", "obs_maxmean"):
                    # (reductions have no per-handle bound of their own: the fast-path sets hold none, and a random
                    #  program, which does, never runs under --bound)
                    raise ValueError("--bound does not serve reduction observers")
                if not bound and not _eq(ve, vl):  # (--bound: obs_get is covered by the comparison of every handle)
                    raise Mismatch("observer %s: lazy != eager" % op[0], idx, op[1])
                fields(idx)
        fields(len(program["ops"]))
        for a, c in program.get("same_block", []):
            for ex in (eager, lazy):
                if ex.ptr[a] != ex.ptr[c]:
                    raise Mismatch("handle %d did not get the block handle %d gave back" % (c, a), -1, c)
        if home:
            lazy.home(sym)
    except Mismatch:
        tidy()
        raise
    tidy()
    after = lazy.b.lazy_stats()
    worst["stats"] = {k: after[k] - before[k] for k in after if after[k] != before[k] and k != "extra_buffers"}
    return worst


def report_and_minimise(program, err, tmp, **kw):
    print("MISMATCH %s at op %d, handle %s: %s" % (program["name"], err.op_index, err.handle, err.what), flush=True)
    print("PROGRAM " + lp.dumps(program), flush=True)

    def fails(cand):
        try:
            run_program(cand, **kw)
        except Mismatch:
            return True
        return False

    small, runs = lp.minimise(program, fails, budget=200)
    print("MINIMISED (%d executions, %d of %d ops) %s" % (runs, len(small["ops"]), len(program["ops"]), lp.dumps(small)),
          flush=True)
    if tmp:
        path = os.path.join(tmp, "minimised_%s.json" % program["name"].replace("/", "_").replace(":", "_"))
        with open(path, "w") as fh:
            fh.write(lp.dumps(small))
        print("WROTE " + path, flush=True)


def controls(program, stats, fast):
    """an unmutated idiom raises its counter; nothing is declined, no reorder / veccopy moves data"""
    name = program["name"]
    if "/" in name or name not in lp.CONTROLS:
        return None
    want = dict(lp.CONTROLS[name])
    if fast:
        want.update(lp.CONTROLS_FAST.get(name, {}))
    if os.environ.get("X3D_LAZY_RULES"):
        want = {k: v for k, v in want.items() if k != "pairs"}  # (the parent masked the pair rewrites)
    bad = {k: stats.get(k, 0) for k, v in want.items() if stats.get(k, 0) != v}
    for k in ("declined", "materialised"):
        if stats.get(k, 0) != 0:
            bad[k] = stats[k]
    return bad or None


def leak(programs):
    """the same program ten times in a row on one backend: extra_buffers stays where it stood after the second run"""
    bad = []
    for p in programs:
        _, lazy = backends(p["shape"], p.get("env"))
        n = []
        for _ in range(10):
            for op in p["ops"]:
                lazy.apply(op)
            lazy.release_all()  # (not reached behind an X3dError: nothing further is started then)
            _lib.check(lazy.b.lib.x3d_lazy_flush(lazy.b.h))
            n.append(lazy.b.lazy_stats()["extra_buffers"])
        if n[-1] != n[1]:
            bad.append((p["name"], n))
    return bad


def main(argv):
    t0 = time.time()
    if argv[0] == "replay":
        with open(argv[1]) as fh:
            program = lp.loads(fh.read())
        try:
            out = run_program(program, model="--model" in argv)
        except Mismatch as e:
            print("MISMATCH at op %d, handle %s: %s" % (e.op_index, e.handle, e.what))
            print("RESULT " + json.dumps({"ok": False}))
            return 1
        print("RESULT " + json.dumps(dict(out, ok=True)))
        return 0
    shape, which = argv[1], argv[2]
    opt = {a: True for a in argv[3:] if a.startswith("--")}
    val = {a: argv[i + 1] for i, a in enumerate(argv) if a in ("--seeds", "--tmp")}
    model, bound, tmp = "--model" in opt, "--bound" in opt, val.get("--tmp")
    if which == "enum":
        programs = lp.enumerated(shape)
    elif which.startswith("fast"):  # fast, or fast:IDIOM
        programs = lp.enumerated(shape, idioms=which.split(":", 1)[1].split(",") if ":" in which else lp.FAST_IDIOMS)
    elif which in ("random", "leak"):
        lo, hi = (int(v) for v in val["--seeds"].split(":"))
        programs = [lp.random_program(shape, s)[0] for s in range(lo, hi)]
        if which == "leak":
            programs = lp.enumerated(shape) + programs
    else:
        raise SystemExit("unknown set " + which)
    res = {"shape": shape, "set": which, "programs": 0, "ratio": 0.0, "lazy_vs_eager": 0.0, "controls_failed": [],
           "controls": 0, "single": bool(_lib.SINGLE), "ok": True}
    try:
        if which == "leak":
            bad = leak(programs)
            res.update(programs=len(programs), leaks=bad, ok=not bad)
        else:
            for p in programs:
                try:
                    out = run_program(p, model=model, bound=bound, home=True)
                except Mismatch as e:
                    res["ok"] = False
                    res["mismatch"] = {"name": p["name"], "op": e.op_index, "handle": e.handle, "what": e.what}
                    print("STATS " + json.dumps(lazy_delta(p)), flush=True)
                    report_and_minimise(p, e, tmp, model=model, bound=bound, home=True)
                    break
                res["programs"] += 1
                res["ratio"] = max(res["ratio"], out["ratio"])
                res["lazy_vs_eager"] = max(res["lazy_vs_eager"], out["lazy_vs_eager"])
                bad = controls(p, out["stats"], shape == "F1")
                if "/" not in p["name"] and p["name"] in lp.CONTROLS:
                    res["controls"] += 1
                if bad:
                    res["controls_failed"].append([p["name"], bad, out["stats"]])
                print("PROG " + json.dumps({"name": p["name"], "stats": out["stats"], "ratio": out["ratio"],
                                            "lazy_vs_eager": out["lazy_vs_eager"]}), flush=True)
    except X3dError as e:
        print("X3DERROR %s" % e, flush=True)
        res["ok"] = False
        res["error"] = str(e)
        print("RESULT " + json.dumps(res), flush=True)
        return 2
    res["seconds"] = round(time.time() - t0, 2)
    print("RESULT " + json.dumps(res), flush=True)
    return 0 if res["ok"] else 1


def lazy_delta(program):
    """lazy_stats() of the program run by itself on the deferred backend"""
    _, lazy = backends(program["shape"], program.get("env"))
    before = lazy.b.lazy_stats()
    for op in program["ops"]:
        lazy.apply(op)
    lazy.release_all()
    _lib.check(lazy.b.lib.x3d_lazy_flush(lazy.b.h))
    after = lazy.b.lazy_stats()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


if __name__ == "__main__":
    try:
        rc = main(sys.argv[1:])
    except X3dError as e:
        print("X3DERROR %s" % e, flush=True)
        rc = 2
    sys.stdout.flush()
    sys.stderr.flush()
    if rc == 2:
        # behind an X3dError nothing further may reach the GPU: an ordinary exit would destroy the backends, which
        # brings every handle home first (x3d_lazy_sync) and so runs what is left in the queue
        os._exit(2)
    sys.exit(rc)
