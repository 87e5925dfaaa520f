"""Generated call sequences for the deferred-execution layer (x3d2_amd/csrc/lazy.hip): programs on the op-granular
interface, the generator (one template per rewrite, every mutation of it enumerated, seeded random interleavings), the
CPU float64 model (oracle.x3d_oracle: plain arrays, value semantics, no aliases, no deferral), the closed-form
evaluation of BLAS-1 programs and the greedy minimiser.  Pure Python: nothing here imports the GPU side; the executor
for the HIP backends lives in tests/lazy_fuzz_worker.py and shares `Sym` (the per-handle symbolic state) with it.

A program is {"name", "ops", "env"?, "seed"?}; an op is a JSON list, handles are small integers:
  ["get", h, d]  ["rel", h]  ["upload", h, seed, loc] (sync)       d in "xyz"; loc a data_loc
  ["veccopy", dst, src] (dst also takes src's data_loc)  ["reorder", dst, src]
  ["vecadd", a, x, b, y]  ["vecmult", y, x]  ["scale", f, a]  ["shift", f, a]
  ["sum", d, u, u_]  ["tds", du, u, opname]  ["transeq", d, [du, dv, dw], [u, v, w]] (d == "x": sync)
  ["species", d, dspec, uvw, spec]  ["setface", f, f_start]  ["fft_fwd", f, k]  ["fft_post", k]  ["fft_bwd", f, k]
      (k: which poisson_fft object, 0 the backend's own, 1 a second one on the same backend)
  observers (sync): ["obs_get", h]  ["obs_dot", x, y]  ["obs_maxmean", f]  ["lincomb", y, base, [c..], [x..]]
                    ["flush"]  ["sync"]
Every handle still live when the program ends is released by the executor."""
import functools
import json
import os
import sys

import numpy as np

VERT, CELL, NULL_LOC = 0, 1110, -1
DIRN = {"x": 1, "y": 2, "z": 3}
OPNAMES = ["der1st", "der1st_sym", "der2nd", "der2nd_sym", "stagder_v2p", "stagder_p2v", "interpl_v2p", "interpl_p2v"]
MOVE = {"stagder_v2p": 1, "interpl_v2p": 1, "stagder_p2v": -1, "interpl_p2v": -1}
NA = float(np.nextafter(1.0, 2.0))
NU = 0.05
MAXLEN = 48

TWOPI = 6.283185307179586
SHAPES = {
    # the shape of test_blas1_reorder_faces: generic kernels on both sides
    "S1": dict(dims=(20, 12, 16), L=(TWOPI, 2.0, 3.0), bc_y="periodic", stretching="uniform", beta=1.0),
    # Dirichlet + stretched y: data_loc changes extents, the Y_FACE stamp means something
    "D1": dict(dims=(24, 17, 16), L=(TWOPI, 2.0, 3.0), bc_y="dirichlet", stretching="top-bottom", beta=0.259065151),
    # the smallest shape x3d_transeq_x_update and the z tile kernel's stage serve (rules 8 and 10): 256-point x pencils,
    # 64 * Q = 256 rows in z (csrc/xscan.hip, x3d_ytile_applicable); y is free, 8 rows keep it cheap
    "F1": dict(dims=(256, 8, 256), L=(TWOPI, 2.0, TWOPI), bc_y="periodic", stretching="uniform", beta=1.0),
}


class Invalid(Exception):
    """the program asks for something the eager backend refuses, or reads an undefined block"""


def digit(loc, d):
    return (loc // 10 ** DIRN[d]) % 10


# ---------------------------------------------------------------- symbolic state
class Sym:
    """per handle: direction tag, data_loc, whether its contents are defined"""

    def __init__(self):
        self.h = {}
        self.fft = {}  # per poisson_fft object: 1 forward done, 2 post-processed

    def _live(self, *hs):
        for h in hs:
            if h not in self.h:
                raise Invalid("handle %r is not live" % (h,))

    def _read(self, *hs):
        self._live(*hs)
        for h in hs:
            if not self.h[h]["def"]:
                raise Invalid("handle %d is read undefined" % h)

    def _same(self, *hs):
        a = self.h[hs[0]]
        for h in hs[1:]:
            if self.h[h]["dir"] != a["dir"] or self.h[h]["loc"] != a["loc"]:
                raise Invalid("handles %r differ in direction or data_loc" % (hs,))

    def _write(self, h, loc):
        self.h[h]["def"], self.h[h]["loc"] = True, loc

    def defined(self):
        return [h for h in sorted(self.h) if self.h[h]["def"]]

    def apply(self, op):
        k, a = op[0], op[1:]
        H = self.h
        if k == "get":
            if a[0] in H or a[1] not in DIRN:
                raise Invalid("get: handle in use or bad direction")
            H[a[0]] = {"dir": a[1], "loc": NULL_LOC, "def": False}
        elif k == "rel":
            self._live(a[0])
            del H[a[0]]
        elif k == "upload":
            self._live(a[0])
            self._write(a[0], a[2])
        elif k == "veccopy":
            self._read(a[1]); self._live(a[0])
            if a[0] == a[1] or H[a[0]]["dir"] != H[a[1]]["dir"]:
                raise Invalid("veccopy: incompatible fields")
            self._write(a[0], H[a[1]]["loc"])
        elif k == "reorder":
            self._read(a[1]); self._live(a[0])
            if H[a[0]]["dir"] == H[a[1]]["dir"]:
                raise Invalid("reorder: the same direction")
            self._write(a[0], H[a[1]]["loc"])
        elif k == "vecadd":
            self._read(a[1], a[3]); self._same(a[1], a[3])
        elif k == "vecmult":
            self._read(a[0], a[1]); self._same(a[0], a[1])
        elif k in ("scale", "shift", "obs_get", "obs_maxmean"):
            self._read(a[0])
        elif k == "sum":
            self._read(a[1], a[2])
            if H[a[1]]["dir"] != "x" or H[a[2]]["dir"] != a[0] or a[0] == "x" or H[a[1]]["loc"] != H[a[2]]["loc"]:
                raise Invalid("sum_%sintox: directions or data_loc" % a[0])
        elif k == "tds":
            du, u, name = a
            self._read(u); self._live(du)
            d = H[u]["dir"]
            if du == u or H[du]["dir"] != d:
                raise Invalid("tds_solve: in place or DIR mismatch")
            mv = MOVE.get(name, 0)
            if digit(H[u]["loc"], d) != (1 if mv < 0 else 0):
                raise Invalid("tds_solve: %s on data_loc %d" % (name, H[u]["loc"]))
            self._write(du, H[u]["loc"] + mv * 10 ** DIRN[d])
        elif k in ("transeq", "species"):
            d, outs, ins = (a[0], a[1], a[2]) if k == "transeq" else (a[0], [a[1]], [a[2], a[3]])
            self._read(*ins); self._live(*outs)
            if len(set(outs)) != len(outs) or set(outs) & set(ins) or any(H[h]["loc"] != VERT for h in ins):
                raise Invalid("%s: outputs among the inputs, or inputs not at VERT" % k)
            for h in outs:
                self._write(h, VERT)
        elif k == "setface":
            self._read(a[0], a[1])
            if a[0] == a[1] or any(H[h]["dir"] != "x" or H[h]["loc"] != VERT for h in a[:2]):
                raise Invalid("setface: DIR_X fields at VERT")
        elif k == "fft_fwd":
            self._read(a[0])
            if H[a[0]]["loc"] != CELL:
                raise Invalid("fft_forward: a CELL field")
            self.fft[a[1]] = 1
        elif k == "fft_post":
            if self.fft.get(a[0]) != 1:
                raise Invalid("fft_postprocess without a forward transform")
            self.fft[a[0]] = 2
        elif k == "fft_bwd":
            self._read(a[0])
            if self.fft.get(a[1]) != 2 or H[a[0]]["loc"] != CELL:
                raise Invalid("fft_backward: no processed spectrum, or not a CELL field")
            self.fft[a[1]] = 0
        elif k == "obs_dot":
            self._read(a[0], a[1])
            if H[a[0]]["loc"] != H[a[1]]["loc"]:
                raise Invalid("scalar_product: data_loc")
        elif k == "lincomb":
            y, base, cs, xs = a
            self._read(base, *xs); self._live(y); self._same(base, *xs)
            if H[y]["dir"] != H[base]["dir"] or len(cs) != len(xs) or not 1 <= len(xs) <= 5:
                raise Invalid("lincomb: directions or term count")
            self._write(y, H[base]["loc"])
        elif k in ("flush", "sync"):
            pass
        else:
            raise Invalid("unknown op %r" % (k,))


OBSERVERS = ("obs_get", "obs_dot", "obs_maxmean", "lincomb", "flush", "sync")


def check(program):
    """replay the symbolic state: raises Invalid where the eager backend would refuse or an undefined block is read"""
    s = Sym()
    for op in program["ops"]:
        s.apply(op)
    return s


def dumps(program):
    return json.dumps(program)


def loads(text):
    return json.loads(text)


@functools.lru_cache(maxsize=32)
def field_data(seed, nx, ny, nz):
    """the upload of `seed`: a few low modes plus 1 % noise, O(1) (cached: callers copy, never write)"""
    rng = np.random.default_rng(1000 + int(seed))
    ax = [np.arange(n) / float(n) for n in (nx, ny, nz)]
    a = np.zeros((nz, ny, nx))
    for _ in range(3):
        k = rng.integers(1, 3, size=3)
        p = rng.uniform(0.0, TWOPI, size=3)
        amp = rng.uniform(0.3, 1.0)
        a += amp * (np.cos(TWOPI * k[0] * ax[0] + p[0])[None, None, :] * np.cos(TWOPI * k[1] * ax[1] + p[1])[None, :, None]
                    * np.cos(TWOPI * k[2] * ax[2] + p[2])[:, None, None])
    return a + 0.01 * rng.standard_normal(a.shape)


# ---------------------------------------------------------------- the model
def _oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from oracle import x3d_oracle
    return x3d_oracle


_MODEL_CACHE = {}


def model_setup(shape):
    """(oracle module, mesh, backend, dirps by direction name, Poisson solver or None) of one shape, built once"""
    if shape not in _MODEL_CACHE:
        ox = _oracle()
        c = SHAPES[shape]
        per = ("periodic",) * 2
        mesh = ox.Mesh(c["dims"], (1, 1, 1), c["L"], per, (c["bc_y"],) * 2, per,
                       stretching=("uniform", c["stretching"], "uniform"), beta=(1.0, c["beta"], 1.0))
        dirps = {}
        for d, n in DIRN.items():
            dirps[d] = ox.Dirps(n)
            ox.allocate_tdsops(dirps[d], mesh)
        pf = ox.PoissonFFT(mesh, dirps["x"], dirps["y"], dirps["z"]) if c["bc_y"] == "periodic" else None
        _MODEL_CACHE[shape] = (ox, mesh, ox.Backend(mesh), dirps, pf)
    return _MODEL_CACHE[shape]


class Model:
    """interprets a program on oracle.x3d_oracle's backend; per handle `chain` (arithmetic ops on its longest dependency
    chain) and `scale` (the largest max norm met along it)"""

    def __init__(self, shape):
        self.ox, self.mesh, self.b, self.dirps, self.pf = model_setup(shape)
        self.f, self.meta, self.spec = {}, {}, {}
        self.sym = Sym()

    def _field(self, d, loc=NULL_LOC):
        n = self.ox.DIR_X + DIRN[d] - 1
        return self.ox.Field(np.zeros(self.b.shape(n)), n, loc)

    def _as(self, f, d):
        """f's data in direction d's layout (all tags share one layout on the device: an op along d takes any tag)"""
        n = DIRN[d]
        if f.dir == n:
            return f
        t = self._field(d, f.data_loc)
        self.b.reorder(t, f, self.ox.RDR[(f.dir, n)])
        return t

    def _back(self, t, f):
        if t is not f:
            loc = t.data_loc
            self.b.reorder(f, t, self.ox.RDR[(t.dir, f.dir)])
            f.data_loc = loc

    def norm(self, h):
        return float(np.max(np.abs(self.get(h))))

    def get(self, h):
        return self.b.get_field_data(self.f[h])

    def _wrote(self, h, ins, arith=True):
        chain = max([self.meta[i][0] for i in ins if i in self.meta] + [0]) + (1 if arith else 0)
        scale = max([self.meta[i][1] for i in ins if i in self.meta] + [self.norm(h)])
        self.meta[h] = (chain, scale)

    def apply(self, op):
        """returns the observer's value (None for the others)"""
        self.sym.apply(op)
        k, a = op[0], op[1:]
        b, F = self.b, self.f
        if k == "get":
            F[a[0]] = self._field(a[1])
        elif k == "rel":
            del F[a[0]]
            self.meta.pop(a[0], None)
        elif k == "upload":
            F[a[0]].data_loc = a[2]
            nx, ny, nz = (int(v) for v in self.mesh.get_dims(a[2]))
            b.set_field_data(F[a[0]], field_data(a[1], nx, ny, nz))
            self.meta[a[0]] = (0, self.norm(a[0]))
        elif k == "veccopy":
            b.veccopy(F[a[0]], F[a[1]])
            F[a[0]].data_loc = F[a[1]].data_loc
            self.meta[a[0]] = self.meta[a[1]]
        elif k == "reorder":
            b.reorder(F[a[0]], F[a[1]], self.ox.RDR[(F[a[1]].dir, F[a[0]].dir)])
            self.meta[a[0]] = self.meta[a[1]]
        elif k == "vecadd":
            b.vecadd(a[0], F[a[1]], a[2], F[a[3]])
            self._wrote(a[3], [a[1], a[3]])
        elif k == "vecmult":
            b.vecmult(F[a[0]], F[a[1]])
            self._wrote(a[0], [a[0], a[1]])
        elif k == "scale":
            b.field_scale(F[a[0]], a[1])
            self._wrote(a[0], [a[0]])
        elif k == "shift":
            b.field_shift(F[a[0]], a[1])
            self._wrote(a[0], [a[0]])
        elif k == "sum":
            (b.sum_yintox if a[0] == "y" else b.sum_zintox)(F[a[1]], F[a[2]])
            self._wrote(a[1], [a[1], a[2]])
        elif k == "tds":
            d = "xyz"[F[a[1]].dir - 1]
            b.tds_solve(F[a[0]], F[a[1]], getattr(self.dirps[d], a[2]))
            self._wrote(a[0], [a[1]])
        elif k == "transeq":
            d, outs, ins = a
            ti = [self._as(F[h], d) for h in ins]
            to = [F[h] if F[h].dir == DIRN[d] else self._field(d) for h in outs]
            getattr(b, "transeq_" + d)(*to, *ti, NU, self.dirps[d])
            for t, h in zip(to, outs):
                self._back(t, F[h])
                F[h].data_loc = VERT
            for h in outs:
                self._wrote(h, ins)
        elif k == "species":
            d, out, uvw, spec = a
            t = F[out] if F[out].dir == DIRN[d] else self._field(d)
            b.transeq_species(t, self._as(F[uvw], d), self._as(F[spec], d), NU, self.dirps[d])
            self._back(t, F[out])
            F[out].data_loc = VERT
            self._wrote(out, [uvw, spec])
        elif k == "setface":
            b.field_set_face_from_field(F[a[0]], F[a[1]], 0.0, self.ox.Y_FACE)
            self._wrote(a[0], [a[0], a[1]], arith=False)
        elif k == "fft_fwd":
            self.spec[a[1]] = (self.get(a[0]), self.meta[a[0]])
        elif k == "fft_post":
            pass
        elif k == "fft_bwd":
            b.set_field_data(F[a[0]], self.pf.solve(self.spec[a[1]][0]))
            chain, scale = self.spec[a[1]][1]
            self.meta[a[0]] = (chain + 1, max(scale, self.norm(a[0])))
        elif k == "obs_get":
            return self.get(a[0])
        elif k == "obs_dot":
            return b.scalar_product(F[a[0]], F[a[1]])
        elif k == "obs_maxmean":
            return b.field_max_mean(F[a[0]])
        elif k == "lincomb":
            y, base, cs, xs = a
            acc = F[base].data.copy()
            for c, x in zip(cs, xs):
                acc += c * F[x].data
            F[y].data[...] = acc
            F[y].data_loc = F[base].data_loc
            self._wrote(y, [base] + list(xs))
        return None

    def run(self, program):
        return [self.apply(op) for op in program["ops"]]


def closed_form(program, dims):
    """plain numpy evaluation of a program of BLAS-1 ops, copies, reorders and uploads at VERT: {handle: [nz, ny, nx]}
    (every DIR tag holds the same Cartesian field)"""
    nx, ny, nz = dims
    v = {}
    for op in program["ops"]:
        k, a = op[0], op[1:]
        if k == "upload":
            assert a[2] == VERT
            v[a[0]] = field_data(a[1], nx, ny, nz)
        elif k in ("veccopy", "reorder"):
            v[a[0]] = v[a[1]].copy()
        elif k == "vecadd":
            v[a[3]] = a[0] * v[a[1]] + a[2] * v[a[3]]
        elif k == "vecmult":
            v[a[0]] = v[a[0]] * v[a[1]]
        elif k == "scale":
            v[a[0]] = v[a[0]] * a[1]
        elif k == "shift":
            v[a[0]] = v[a[0]] + a[1]
        elif k == "sum":
            v[a[1]] = v[a[1]] + v[a[2]]
        elif k == "rel":
            v.pop(a[0], None)
        elif k not in ("get", "flush", "sync", "obs_get"):
            raise ValueError("closed_form: %s is not a BLAS-1 op" % k)
    return v


# ---------------------------------------------------------------- building programs
class Builder:
    def __init__(self, shape, name, rng=None, seed0=0, model=True):
        self.shape, self.name, self.rng = shape, name, rng
        self.ops, self.env, self.same_block = [], {}, []
        self.model = Model(shape) if model else None
        self.sym = self.model.sym if model else Sym()
        self.nh, self.nseed, self.taken = 0, seed0, set()

    def emit(self, *op):
        op = list(op)
        if self.model is not None:
            self.model.apply(op)  # (applies the symbolic state too)
        else:
            self.sym.apply(op)
        self.ops.append(op)

    def new(self, d="x"):
        h = self.nh
        self.nh += 1
        self.emit("get", h, d)
        return h

    def up(self, h, loc=VERT):
        self.nseed += 1
        self.emit("upload", h, self.nseed, loc)

    def pick(self, d="x", loc=VERT):
        """a defined handle of this direction and data_loc for one role of an idiom: fresh in the enumerated programs;
        in random ones a live handle not yet given a role in this idiom, more often than not"""
        if self.rng is not None and self.rng.random() < 0.65:
            c = [h for h in self.sym.defined() if h not in self.taken and self.sym.h[h]["dir"] == d
                 and self.sym.h[h]["loc"] == loc]
            if c:
                h = int(c[int(self.rng.integers(len(c)))])
                self.taken.add(h)
                return h
        h = self.new(d)
        self.up(h, loc)
        self.taken.add(h)
        return h

    def rel(self, *hs):
        for h in hs:
            if h in self.sym.h:
                self.emit("rel", h)

    def program(self):
        p = {"name": self.name, "shape": self.shape, "ops": self.ops}
        if self.env:
            p["env"] = dict(self.env)
        if self.same_block:
            p["same_block"] = [list(v) for v in self.same_block]  # [a, b]: handle b is the block handle a gave back
        return p


def _bystanders(B, m):
    """what a window split needs, made BEFORE the pattern starts (an upload is a sync point itself)"""
    if m == "M9get":
        return [B.pick()]
    if m == "M9tx":
        return [B.pick(), B.pick(), B.pick()]
    return []


def _split(B, m, by):
    if m == "M9flush":
        B.emit("flush")
    elif m == "M9get":
        B.emit("obs_get", by[0])
    elif m == "M9tx":
        B.emit("transeq", "x", [B.new(), B.new(), B.new()], by)


def _to_dir(B, h, d):
    if d == "x":
        return h, None
    t = B.new(d)
    B.emit("reorder", t, h)
    return t, t


M9 = ["M9flush", "M9get", "M9tx"]
M8P = ["M8_021", "M8_102", "M8_120", "M8_201", "M8_210"]  # the three steps of a pattern in every other order


def _order(m):
    return [int(c) for c in m[3:]] if (m or "").startswith("M8_") else [0, 1, 2]


def r1(B, m=None, d="y"):
    """rule 1: transeq_<d> followed by three sum_<d>intox"""
    vel = [B.pick() for _ in range(3)]
    acc = [B.pick() for _ in range(3)]
    by = _bystanders(B, m)
    t = B.new(d if m == "M1" else "x") if m in ("M1", "M3a") else None
    al = None
    if m in ("M5same", "M5earlier"):
        al = B.new()
        B.emit("veccopy", al, acc[0])
        if m == "M5earlier":
            B.emit("flush")
    ins, temps = [], []
    for k, f in enumerate(vel):
        if k == 0 and m == "M4in":
            ins.append(acc[0])
        elif k == 0 and al is not None:
            ins.append(al)
        else:
            g = B.new(d)
            B.emit("reorder", g, f)
            ins.append(g)
            temps.append(g)
    od = "z" if d == "y" else "y"
    outs = [B.new(d), B.new(d), B.new(od if m == "M7" else d)]
    B.emit("transeq", d, outs, ins)
    if m == "M3b":
        B.emit("scale", ins[1], 2.0)
    if m != "M8rel":
        B.rel(*temps)
    if m == "M3a":
        B.emit("veccopy", t, acc[0])
    if m == "M3c":
        B.emit("scale", outs[0], 0.5)
    _split(B, m, by)
    for k in _order(m):
        if m == "M10two" and k == 2:
            continue
        a = acc[0] if (m == "M4acc" and k == 1) else acc[k]
        sd = od if (m == "M7" and k == 2) else d
        B.emit("sum", sd, a, outs[k])
        if m == "M10twice" and k == 0:
            B.emit("sum", sd, a, outs[k])
        if m == "M8rel":
            B.rel(outs[k])
    if m == "M8rel":
        B.rel(*temps)
    if m == "M1":
        B.emit("veccopy", t, outs[0])
    if m != "M2":
        B.rel(*outs)


def r1b(B, m=None, d="y"):
    """rule 1b: transeq_species followed by its sum_<d>intox"""
    uvw, spec, acc = B.pick(), B.pick(), B.pick()
    by = _bystanders(B, m)
    t = B.new(d if m == "M1" else "x") if m in ("M1", "M3a") else None
    al = None
    if m in ("M5same", "M5earlier"):  # the species input is an alias of the accumulator's buffer
        al = B.new()
        B.emit("veccopy", al, acc)
        if m == "M5earlier":
            B.emit("flush")
    i0, t0 = (acc, None) if m == "M4uvw" else _to_dir(B, uvw, d)
    i1, t1 = (acc, None) if m == "M4in" else ((al, None) if al is not None else _to_dir(B, spec, d))
    od = "z" if d == "y" else "y"
    out = B.new(od if m == "M7" else d)
    B.emit("species", d, out, i0, i1)
    if m == "M3b":
        B.emit("scale", i0, 2.0)
    if m != "M8rel":
        B.rel(*[x for x in (t0, t1) if x is not None])
    if m == "M3a":
        B.emit("veccopy", t, acc)
    if m == "M3c":
        B.emit("scale", out, 0.5)
    _split(B, m, by)
    B.emit("sum", od if m == "M7" else d, acc, out)
    if m == "M10twice":
        B.emit("sum", d, acc, out)
    if m == "M1":
        B.emit("veccopy", t, out)
    if m != "M2":
        B.rel(out)
    if m == "M8rel":
        B.rel(*[x for x in (t0, t1) if x is not None])


def r2(B, m=None, d="y"):
    """rule 2: a = A(i1); b = B(i2); a += b"""
    dd = "x" if m == "M7x" else d
    opa, opb = ("der1st", "der2nd") if m in ("M4", "M4b", "M5same") else ("interpl_v2p", "stagder_v2p")
    u, v = B.pick(), B.pick()
    by = _bystanders(B, m)
    t = B.new(dd) if m in ("M1", "M3a") else None
    i1, t1 = _to_dir(B, u, dd)
    if m == "M5earlier":
        i2 = t2 = B.new(dd)
        B.emit("veccopy", i2, i1)
        B.emit("flush")
    else:
        i2, t2 = _to_dir(B, v, dd)
    a, b = B.new(dd), B.new(dd)
    al = B.new(dd) if m == "M5same" else None
    if m == "M8swap":
        B.emit("tds", b, i2, opb)
        B.emit("tds", a, i1, opa)
    elif m == "M4":
        B.emit("tds", a, i1, opa)
        B.emit("tds", b, a, opb)
    elif m == "M4b":
        B.emit("tds", b, i2, opb)
        B.emit("tds", a, b, opa)
    elif m == "M5same":
        B.emit("tds", a, i1, opa)
        B.emit("veccopy", al, a)
        B.emit("tds", b, al, opb)
    else:
        B.emit("tds", a, i1, opa)
        if m == "M8rel" and t1 is not None:
            B.rel(t1)
        if m == "M3b":
            B.emit("scale", i1, 2.0)
        B.emit("tds", b, i2, opb)
    if m == "M3a":
        B.emit("veccopy", t, a)
    if m == "M3c":
        B.emit("scale", b, 0.5)
    _split(B, m, by)
    c0 = {"M6a_na": NA, "M6a_m1": -1.0, "M6a_0": 0.0}.get(m, 1.0)
    c1 = {"M6b_na": NA, "M6b_m1": -1.0, "M6b_0": 0.0}.get(m, 1.0)
    B.emit("vecadd", c0, b, c1, a)
    if m == "M1":
        B.emit("veccopy", t, b)
    if m != "M2":
        B.rel(b)
    B.rel(*[x for x in (t1, t2, al) if x is not None])


def r3(B, m=None, d="y"):
    """rule 3: a = A(i); b = B(i)"""
    dd = "x" if m == "M7x" else d
    i = B.pick(dd, VERT + 10 ** DIRN[dd])
    u = B.pick() if m == "M3a" else None
    by = _bystanders(B, m)
    t = B.new() if m == "M3a" else None
    junk = B.new() if m == "M8rel" else None
    a, b = B.new(dd), B.new(dd)
    c = B.new(dd) if m == "M10three" else None
    i2 = None
    if m in ("M5same", "M5earlier"):
        i2 = B.new(dd)
        B.emit("veccopy", i2, i)
        if m == "M5earlier":
            B.emit("flush")
    first, second = ("interpl_p2v", a), ("stagder_p2v", b)
    if m == "M8swap":
        first, second = second, first
    B.emit("tds", first[1], i, first[0])
    if m == "M3a":
        B.emit("veccopy", t, u)
    if m == "M3b":
        B.emit("scale", i, 2.0)
    if m == "M8rel":
        B.rel(junk)
    _split(B, m, by)
    B.emit("tds", a if m == "M4out" else second[1], i if i2 is None else i2, second[0])
    if c is not None:
        B.emit("tds", c, i, "interpl_p2v")
    if m == "M4out":
        B.rel(b)


def r4(B, m=None, d="x"):
    """rule 4: g = A(p); u += s g"""
    u = B.pick(d)  # (uploaded in its own direction: a reordered copy would share its buffer and the update copy it first)
    p, tp = (u, None) if m == "M4" else (B.pick(d), None)
    by = _bystanders(B, m)
    t = B.new(d) if m in ("M1", "M3a") else None
    ua = None
    if m in ("M5same", "M5earlier"):
        ua = B.new(d)
        B.emit("veccopy", ua, u)
        if m == "M5earlier":
            B.emit("flush")
        p = ua
    g = B.new(d)
    B.emit("tds", g, p, "der1st")
    if m == "M3a":
        B.emit("veccopy", t, u)
    if m == "M3b":
        B.emit("scale", p, 2.0)
    if m == "M3c":
        B.emit("scale", g, 0.5)
    _split(B, m, by)
    s = {"M6a_0": 0.0, "M6a_1": 1.0}.get(m, -0.37)
    c1 = {"M6b_na": NA, "M6b_m1": -1.0, "M6b_0": 0.0}.get(m, 1.0)
    B.emit("vecadd", s, g, c1, u)
    if m == "M1":
        B.emit("veccopy", t, g)
    if m != "M2":
        B.rel(g)
    B.rel(*[x for x in (tp, ua) if x is not None])


def r5(B, m=None):
    """rule 5: veccopy followed by a vecadd chain"""
    b, x1, x2 = B.pick(), B.pick(), B.pick()
    by = _bystanders(B, m)
    y = B.new()
    t = B.new() if m == "M3a" else None
    if m == "M5earlier":
        x2 = B.new()
        B.emit("veccopy", x2, b)
        B.emit("flush")
    y2 = B.new() if m == "M5same" else None
    if m == "M6zero_keep":
        B.env["X3D_LAZY_KEEP_ZERO_TERMS"] = "1"
    B.emit("veccopy", y, b)
    B.emit("vecadd", 0.25, b if m == "M4b" else x1, 1.0, y)
    if m == "M3a":
        B.emit("veccopy", t, y)
    if m == "M3b":
        B.emit("scale", x2, 2.0)
    if m == "M3c":
        B.emit("scale", y, 0.5)
    _split(B, m, by)
    if m == "M5same":
        B.emit("veccopy", y2, y)
        x2 = y2
    c2 = 0.0 if m in ("M6zero", "M6zero_keep") else -0.5
    c1 = {"M6b_na": NA, "M6b_m1": -1.0, "M6b_0": 0.0}.get(m, 1.0)
    B.emit("vecadd", c2, y if m == "M4" else x2, c1, y)
    if m == "M10six":
        for k in range(4):
            B.emit("vecadd", 0.125 * (k + 1), (x1, x2)[k % 2], 1.0, y)


def r6(B, m=None, variant="plain"):
    """rule 6: lincomb; tds_solve along x -- plain, with the Y_FACE stamp in between, and the ring form (the solve's
    output handle still in use under its previous life: L_BIND)"""
    dd = "y" if m == "M7y" else "x"
    b0, x10, x20 = B.pick(), B.pick(), B.pick()
    wall = B.pick() if variant == "face" else None
    r = B.pick() if variant == "ring" else None
    by = _bystanders(B, m)
    (b, tb), (x1, t1), (x2, t2) = _to_dir(B, b0, dd), _to_dir(B, x10, dd), _to_dir(B, x20, dd)
    y = B.new(dd)
    t = B.new(dd) if (m == "M3a" or variant == "ring") else None
    x1a = None
    if m in ("M5same", "M5earlier"):
        x1a = B.new(dd)
        B.emit("veccopy", x1a, x1)
        if m == "M5earlier":
            B.emit("flush")
    du = None if variant == "ring" else B.new(dd)
    if m == "M6zero_keep":
        B.env["X3D_LAZY_KEEP_ZERO_TERMS"] = "1"
    B.emit("veccopy", y, b)
    B.emit("vecadd", 0.25, x1, 1.0, y)
    B.emit("vecadd", 0.0 if m in ("M6zero", "M6zero_keep") else -0.5, x2,
           {"M6b_na": NA, "M6b_m1": -1.0, "M6b_0": 0.0}.get(m, 1.0), y)
    if m == "M10six":
        for k in range(4):
            B.emit("vecadd", 0.125 * (k + 1), (x1, x2)[k % 2], 1.0, y)
    if wall is not None:
        B.emit("setface", y, wall)
    if m == "M3a":
        B.emit("veccopy", t, y)
    if m == "M3b":
        B.emit("scale", x1, 2.0)
    _split(B, m, by)
    if variant == "ring":
        if m != "M3a":
            B.emit("veccopy", t, r)
        B.emit("scale", x1, 2.0)
        B.rel(r)
        du = B.new(dd)  # (the allocator hands r's block back: the executor asserts it)
        B.same_block.append([r, du])
    if m == "M4":
        du = x1
    elif m == "M4wall":
        du = wall
    elif x1a is not None:
        du = x1a
    B.emit("tds", du, y, "der1st")
    B.rel(*[x for x in (tb, t1, t2) if x is not None and x != du])


def r7(B, m=None):
    """rule 7: fft_forward; fft_postprocess_000; fft_backward"""
    f = B.pick("z", CELL)
    g = B.pick("z", CELL) if m == "M7field" else f
    by = _bystanders(B, m if m != "M9post" else "M9get")
    if m == "M7obj":
        # the backward hook of ANOTHER poisson object, which holds the processed spectrum of h, on the same field:
        # f = solve(h), and the transform of f stays where it is
        h = B.pick("z", CELL)
        B.emit("fft_fwd", h, 1)
        B.emit("fft_post", 1)
    B.emit("fft_fwd", f, 0)
    if m == "M3b":
        B.emit("scale", f, 2.0)
    _split(B, m, by)
    B.emit("fft_post", 0)
    if m == "M9post":
        B.emit("obs_get", by[0])
    B.emit("fft_bwd", g, 1 if m == "M7obj" else 0)


def r8(B, m=None):
    """rule 8: three accumulating x solves followed by transeq_x"""
    vel = [B.pick() for _ in range(3)]
    grad = [B.pick("x", VERT + 10) for _ in range(3)]
    by = _bystanders(B, m)
    t = B.new() if m == "M3a" else None
    outs = [B.new(), B.new(), B.new()]
    if m == "M4":
        outs[0] = grad[0]
    if m in ("M5same", "M5earlier"):
        outs[0] = B.new()
        B.emit("veccopy", outs[0], grad[0])
        if m == "M5earlier":
            B.emit("flush")
    ops = ["stagder_p2v", "interpl_p2v", "stagder_p2v" if m == "M7" else "interpl_p2v"]
    s = [-0.37, -0.37 * (NA if m == "M6" else 1.0), -0.37]
    for k in _order(m):
        if m == "M10two" and k == 2:
            continue
        tk = B.new()
        B.emit("tds", tk, grad[k], ops[k])
        B.emit("vecadd", s[k], tk, 1.0, vel[k])
        B.rel(tk)
    if m == "M3a":
        B.emit("veccopy", t, vel[0])
    if m == "M3b":
        B.emit("scale", grad[1], 2.0)
    _split(B, m, by)
    B.emit("transeq", "x", outs, vel)


def r10(B, m=None, variant="plain"):
    """rule 10: transeq_acc_z, then [save; release], then three combinations that read the derivative blocks"""
    vel = [B.pick() for _ in range(3)]
    der = [B.pick() for _ in range(3)]
    by = _bystanders(B, m)
    t = B.new() if m in ("M1", "M3a") else None
    olds = [B.new() for _ in range(3)] if variant == "save" else None
    dua = B.new() if m in ("M5same", "M5earlier") else None
    if m == "M5earlier":
        B.emit("veccopy", dua, der[0])
        B.emit("flush")
    temps = []
    for f in vel:
        g = B.new("z")
        B.emit("reorder", g, f)
        temps.append(g)
    outs = [B.new("z") for _ in range(3)]
    B.emit("transeq", "z", outs, temps)
    B.rel(*temps)
    for k in range(3):
        B.emit("sum", "z", der[k], outs[k])
    B.rel(*outs)
    if m == "M3a":
        B.emit("veccopy", t, der[0])
    if m == "M3c":
        B.emit("scale", der[0], 0.5)
    if m == "M5same":
        B.emit("veccopy", dua, der[0])
    _split(B, m, by)
    coef = [0.011, -0.007, 0.013]
    for k in _order(m):
        if m == "M10two" and k == 2:
            continue
        if m == "M4" and k == 0:
            B.emit("vecadd", coef[k], der[0], 1.0, der[1])  # the result IS a derivative block
        else:
            term = dua if (dua is not None and k == 0 and m == "M5same") else der[k]
            B.emit("vecadd", coef[k], term, NA if (m == "M6" and k == 1) else 1.0, vel[k])
        if olds is not None:
            B.emit("veccopy", olds[k], der[k])
    if m == "M1":
        B.emit("veccopy", t, der[0])
    if m != "M2":
        B.rel(*der)
    if dua is not None:
        B.rel(dua)


M6AB = ["M6a_na", "M6a_m1", "M6a_0", "M6b_na", "M6b_m1", "M6b_0"]
R1M = ["M1", "M2", "M3a", "M3b", "M3c", "M4in", "M4acc", "M5same", "M5earlier", "M7"] + M8P + ["M8rel"] + M9 + ["M10two", "M10twice"]
R1BM = ["M1", "M2", "M3a", "M3b", "M3c", "M4in", "M4uvw", "M5same", "M5earlier", "M7", "M8rel"] + M9 + ["M10twice"]
R2M = ["M1", "M2", "M3a", "M3b", "M3c", "M4", "M4b", "M5same", "M5earlier"] + M6AB + ["M7x", "M8swap", "M8rel"] + M9
R3M = ["M3a", "M3b", "M4out", "M5same", "M5earlier", "M7x", "M8swap", "M8rel"] + M9 + ["M10three"]
R4M = ["M1", "M2", "M3a", "M3b", "M3c", "M4", "M5same", "M5earlier", "M6a_0", "M6a_1", "M6b_na", "M6b_m1", "M6b_0"] + M9
R5M = ["M3a", "M3b", "M3c", "M4", "M4b", "M5same", "M5earlier", "M6b_na", "M6b_m1", "M6b_0", "M6zero", "M6zero_keep"] + M9 + ["M10six"]
R6C = ["M6b_na", "M6b_m1", "M6b_0", "M6zero", "M6zero_keep"]  # the chain rule 6 consumes: rule 5's coefficient positions
R6M = ["M3a", "M3b", "M4", "M5same", "M5earlier"] + R6C + M9 + ["M10six"]
R10M = ["M1", "M2", "M3a", "M3c", "M4", "M5same", "M5earlier", "M6"] + M8P + M9 + ["M10two"]
# idiom -> (template, its keyword arguments, the mutations applicable to it, periodic shapes only)
TABLE = {
    "r1:y": (r1, {"d": "y"}, R1M, False), "r1:z": (r1, {"d": "z"}, R1M, False),
    "r1b:y": (r1b, {"d": "y"}, R1BM, False), "r1b:z": (r1b, {"d": "z"}, R1BM, False),
    "r2:y": (r2, {"d": "y"}, R2M, False), "r2:z": (r2, {"d": "z"}, R2M, False),
    "r3:y": (r3, {"d": "y"}, R3M, False), "r3:z": (r3, {"d": "z"}, R3M, False),
    "r4:x": (r4, {"d": "x"}, R4M, False), "r4:y": (r4, {"d": "y"}, R4M, False), "r4:z": (r4, {"d": "z"}, R4M, False),
    "r5": (r5, {}, R5M, False),
    "r6:plain": (r6, {"variant": "plain"}, R6M + ["M7y"], False),
    "r6:face": (r6, {"variant": "face"}, R6M + ["M4wall"], False),
    "r6:ring": (r6, {"variant": "ring"}, ["M3a"] + R6C + M9 + ["M10six"], False),
    "r7": (r7, {}, ["M3b", "M7field", "M7obj", "M9flush", "M9get", "M9post"], True),
    "r8": (r8, {}, ["M3a", "M3b", "M4", "M5same", "M5earlier", "M6", "M7"] + M8P + M9 + ["M10two"], False),
    "r10:plain": (r10, {"variant": "plain"}, R10M, False),
    "r10:save": (r10, {"variant": "save"}, R10M, False),
}
# the counter an unmutated idiom must raise on the generic shapes (S1, D1), and on the fast-path shape where it differs
CONTROLS = {
    "r1:y": {"transeq_acc": 1}, "r1:z": {"transeq_acc": 1}, "r1b:y": {}, "r1b:z": {},
    "r2:y": {"pairs": 1}, "r2:z": {"pairs": 1}, "r3:y": {"pairs": 1}, "r3:z": {"pairs": 1},
    "r4:x": {"tds_acc": 1}, "r4:y": {"tds_acc": 1}, "r4:z": {"tds_acc": 1}, "r5": {"lincombs": 1},
    "r6:plain": {"tds_lincomb": 1}, "r6:face": {"tds_lincomb": 1}, "r6:ring": {"tds_lincomb": 1, "launched": 2, "dropped": 2}, "r7": {"solve_000": 1},
    "r8": {"tds_acc": 3, "transeq_upd": 0, "launched": 1, "dropped": 6}, "r10:plain": {"transeq_acc": 1, "lincombs": 3},
    "r10:save": {"transeq_acc": 1, "lincombs": 3},
}
_STAGE = {"transeq_stage": 1, "transeq_acc": 0, "lincombs": 0}
CONTROLS_FAST = {"r8": {"transeq_upd": 1, "tds_acc": 0}, "r10:plain": _STAGE, "r10:save": _STAGE}
FAST_IDIOMS = ["r1:y", "r1:z", "r2:y", "r2:z", "r3:y", "r3:z", "r4:x", "r4:y", "r4:z", "r6:plain", "r6:face", "r6:ring", "r8",
               "r10:plain", "r10:save"]


# Why a mutation class has no program for an idiom (every class of M1..M10 is either in the idiom's list above or here;
# tests/test_lazy_programs_host.py holds the table to that)
RULE2_DIRS = "the two solves in different directions: the eager backend refuses the vecadd (DIR mismatch)"
NOT_APPLICABLE = {
    "r1": {"M6": "no coefficient in the pattern"},
    "r1b": {"M6": "no coefficient in the pattern", "M8": "one sum only: M8rel (hoisted release) is the only other order",
            "M10": "one sum: only `the same sum twice` (M10twice) applies"},
    "r2": {"M10": "the pattern has no repeated step to add or drop", "M7": RULE2_DIRS + "; along x is M7x"},
    "r3": {"M1": "rule 3 drops no temporary", "M2": "rule 3 drops no temporary", "M6": "no coefficient in the pattern"},
    "r4": {"M7": "tds_solve and vecadd of different directions are refused by the eager backend",
           "M8": "two steps, one data-flow order", "M10": "no repeated step"},
    "r5": {"M1": "rule 5 drops no temporary", "M2": "rule 5 drops no temporary", "M7": "BLAS-1 only: no direction or operator",
           "M8": "the chain's order is its data flow"},
    "r6": {"M1": "rule 6 drops no temporary (y stays a result)", "M2": "rule 6 drops no temporary",
           "M8": "combination before solve is the data flow",
           "M7": "face / ring: field_set_face_from_field takes DIR_X fields only; the plain form has M7y",
           "M4": "ring: du is the block the allocator hands back, it cannot also be a term or the wall",
           "M5": "ring: as M4", "M3": "ring: writing a term (M3b) is part of the ring pattern itself"},
    "r7": {"M1": "no temporary", "M2": "no temporary", "M4": "one field role", "M5": "the spectrum lives in the poisson object, "
           "not in a block: an alias of f is another field (M7field)", "M6": "no coefficient", "M8": "the hooks' order is fixed "
           "by the symbolic state (post needs forward, backward needs post)", "M10": "a repeated hook is refused by the "
           "symbolic state (the model has no meaning for it)"},
    "r8": {"M1": "the temporaries are rule 4's (r4 M1)", "M2": "the temporaries are rule 4's (r4 M2)"},
    "r10": {"M7": "rule 10's transeq is rule 1's (r1 M7); the combinations are BLAS-1"},
}


def idioms_for(shape):
    per = SHAPES[shape]["bc_y"] == "periodic"
    return [k for k, v in TABLE.items() if per or not v[3]]


def expected_count(shape, idioms=None):
    return sum(1 + len(TABLE[k][2]) for k in (idioms_for(shape) if idioms is None else idioms))


def build_named(shape, name, model=True):
    """the enumerated program `idiom` or `idiom/mutation`"""
    idiom, _, m = name.partition("/")
    fn, kw, muts, _ = TABLE[idiom]
    if m and m not in muts:
        raise KeyError(name)
    B = Builder(shape, name, model=model)
    fn(B, m or None, **kw)
    return B


def enumerated(shape, idioms=None, model=False):
    """every idiom and every (idiom, mutation) pair, each a fixed, named program"""
    out = []
    for idiom in (idioms_for(shape) if idioms is None else idioms):
        for m in [""] + TABLE[idiom][2]:
            out.append(build_named(shape, idiom + ("/" + m if m else ""), model=model).program())
    return out


# ---------------------------------------------------------------- random programs
FREE = ["vecadd", "vecmult", "scale", "shift", "veccopy", "reorder", "tds", "lincomb", "sum"]


def _free_op(B):
    rng, S = B.rng, B.sym
    live = S.defined()
    kind = FREE[int(rng.integers(len(FREE)))]
    if not live:
        B.pick()
        return
    x = int(live[int(rng.integers(len(live)))])
    hx = S.h[x]
    mates = [h for h in live if S.h[h]["dir"] == hx["dir"] and S.h[h]["loc"] == hx["loc"]]
    y = int(mates[int(rng.integers(len(mates)))])
    if kind == "vecadd":
        B.emit("vecadd", float(rng.choice([1.0, -1.0, 0.5, 0.0, NA])), x, float(rng.choice([1.0, 1.0, -1.0, 0.5])), y)
    elif kind == "vecmult":
        B.emit("vecmult", y, x)
    elif kind == "scale":
        B.emit("scale", x, float(rng.choice([2.0, -0.5, 0.75])))
    elif kind == "shift":
        B.emit("shift", x, float(rng.choice([0.5, -0.25])))
    elif kind == "veccopy":
        B.emit("veccopy", B.new(hx["dir"]), x)
    elif kind == "reorder":
        B.emit("reorder", B.new([d for d in "xyz" if d != hx["dir"]][int(rng.integers(2))]), x)
    elif kind == "tds":
        dg = digit(hx["loc"], hx["dir"])
        names = [n for n in OPNAMES if (MOVE.get(n, 0) < 0) == (dg == 1)]
        B.emit("tds", B.new(hx["dir"]), x, names[int(rng.integers(len(names)))])
    elif kind == "lincomb":
        B.emit("lincomb", B.new(hx["dir"]) if rng.random() < 0.5 else y, x, [0.3, -0.6], [y, x])
    elif kind == "sum":
        c = [(u, v) for u in live for v in live if S.h[u]["dir"] == "x" and S.h[v]["dir"] in "yz"
             and S.h[u]["loc"] == S.h[v]["loc"]]
        if c:
            u, v = c[int(rng.integers(len(c)))]
            B.emit("sum", S.h[v]["dir"], int(u), int(v))
        else:
            B.emit("scale", x, 0.5)


def _observe(B):
    rng, S = B.rng, B.sym
    live = S.defined()
    k = int(rng.integers(5))
    if not live or k == 0:
        B.emit("flush")
    elif k == 1:
        B.emit("sync")
    else:
        x = int(live[int(rng.integers(len(live)))])
        B.emit(("obs_get", "obs_maxmean", "obs_dot")[k - 2], *([x] if k < 4 else [x, x]))


def _condition(B):
    """keep the comparison with the model meaningful: norms back to O(1), long dependency chains re-seeded"""
    for h in B.sym.defined():
        chain, _ = B.model.meta[h]
        n = B.model.norm(h)
        if chain > 8 or n < 1e-3 or not np.isfinite(n):
            # (a small norm is what cancellation leaves, e.g. nextafter(1, 2) x - x: its digits are rounding noise that a
            #  scale back to O(1) would only blow up -- re-seeded by an upload like a chain that grew too long)
            B.up(h, B.sym.h[h]["loc"])
        elif n > 1e3:
            B.emit("scale", h, float(2.0 ** -np.round(np.log2(n))))


_LEN = {}


def worst_len(shape, idiom, m):
    """ops of the idiom with every role on a fresh handle: what it takes at most"""
    key = (shape, idiom, m)
    if key not in _LEN:
        _LEN[key] = len(build_named(shape, idiom + ("/" + m if m else ""), model=False).ops)
    return _LEN[key]


def random_program(shape, seed, maxlen=MAXLEN, idioms=None):
    """the seeded interleaving of idioms (mutated or not), free single ops, releases and observers"""
    rng = np.random.default_rng(seed)
    B = Builder(shape, "seed%d" % seed, rng=rng, seed0=100 * int(seed))
    names = idioms_for(shape) if idioms is None else list(idioms)
    while True:
        room = maxlen - len(B.ops) - len(B.sym.defined()) - 3  # (the conditioning behind the item: one op per handle)
        if room < 3:
            break
        B.taken = set()
        r = rng.random()
        done = False
        if r < 0.45:
            idiom = names[int(rng.integers(len(names)))]
            fn, kw, muts, _ = TABLE[idiom]
            muts = [m for m in muts if m != "M6zero_keep"]  # (an environment switch: enumerated programs only)
            m = muts[int(rng.integers(len(muts)))] if rng.random() < 0.6 else None
            if worst_len(shape, idiom, m) + 8 <= room:
                fn(B, m, **kw)
                done = True
        if done:
            pass
        elif r < 0.75:
            _free_op(B)
        elif r < 0.87:
            live = sorted(B.sym.h)
            if live:
                B.rel(int(live[int(rng.integers(len(live)))]))
        else:
            _observe(B)
        _condition(B)
    p = B.program()
    p["seed"] = int(seed)
    return p, B


# ---------------------------------------------------------------- the minimiser
def minimise(program, fails, budget=200):
    """greedy: drop one op at a time, keep the drop while `fails(program)` still holds, pass after pass until a pass
    drops nothing; at most `budget` executions.  Candidates the symbolic check rejects are not executed."""
    ops, runs, changed = list(program["ops"]), 0, True
    while changed and runs < budget:
        changed = False
        k = len(ops) - 1
        while k >= 0 and runs < budget:
            cand = dict(program, ops=ops[:k] + ops[k + 1:])
            k -= 1
            try:
                check(cand)
            except Invalid:
                continue
            runs += 1
            if fails(cand):
                ops, changed = cand["ops"], True
    return dict(program, ops=ops), runs
