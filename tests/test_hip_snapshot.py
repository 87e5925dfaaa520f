"""Snapshots on the device (csrc/snapshot.hip, x3d2_amd/snapshot.py) against tests/snapshot_ref.py and the composed path
(get_field_data, compute_vorticity / compute_qcriterion, a host slice).

Bounds, with eps of the working precision, none tuned to the kernel:
  COPY    bit-equal to the numpy slice (scale 1), to a * (1 / dt) in the working precision, to np.float32 of that.
  QCRIT   |dQ| <= 8 eps (1/2 (a11^2 + a22^2 + a33^2) + |a12 a21| + |a13 a31| + |a23 a32|): six products and five
          additions, each rounded at most once, fused or not.
  VORT    |d|omega|| <= 8 eps |omega|: each difference is one rounding; squares, sum and root add at most four more.
  4-byte output adds 2^-24 relative."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import snapshot_ref
from test_hip_stats import PER, WALL, Fields, eps_real, make_backend

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DT = 0.0075
FIRSTS = ((0, 0, 0), (1, 2, 1), (2, 1, 0))
SHAPES = [((17, 6, 5), PER, ((1, 1, 1), (2, 3, 2), (4, 1, 5))),     # odd length, padded rows
          ((64, 5, 3), PER, ((1, 1, 1), (3, 2, 1))),                # pitch a multiple of 64: the +16 padding
          ((20, 7, 9), PER, ((32, 8, 16),)),                        # one kept point
          ((33, 33, 4), WALL, ((2, 2, 1),))]                        # non-periodic y


# ---------------------------------------------------------------- helpers (also used by the worker processes)
def real_dtype():
    from x3d2_amd import _lib
    return np.dtype(_lib.NP_REAL)


def random_blocks(b, dims, n, seed):
    """n blocks with standard_normal data exactly representable in both flavours; returns (fields, float64 arrays)"""
    from x3d2_amd.common import DIR_X, VERT
    rng = np.random.default_rng(seed)
    arrays = [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(n)]
    fields = [b.allocator.get_block(DIR_X, VERT) for _ in range(n)]
    for f, a in zip(fields, arrays):
        b.set_field_data(f, a)
    return fields, arrays


def counts(dims, first, stride):
    return tuple((n - f + s - 1) // s for n, f, s in zip(dims, first, stride))


def pack(b, variables, dims, first, stride, out_dtype, extra=1):
    """one launch into a buffer that holds `extra` variables more, pre-filled with the byte 0xA5; returns
    (array [nvar, cz, cy, cx], the bytes behind the last variable)"""
    import torch
    cnt = counts(dims, first, stride)
    npts = int(np.prod(cnt))
    size = np.dtype(out_dtype).itemsize
    out = torch.full(((len(variables) + extra) * npts * size,), 0xA5, dtype=torch.uint8, device=b.device)
    n = b.snapshot_pack(variables, first, stride, cnt, out, out_dtype)
    assert n == len(variables) * npts * size
    raw = out.cpu().numpy()
    return raw[:n].view(out_dtype).reshape(len(variables), cnt[2], cnt[1], cnt[0]), raw[n:]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def usable(dims, first):
    return all(f < n for f, n in zip(first, dims))


def copy_case(dims, ybc, stride, first):
    """five COPY variables in one launch, the three output flavours of the issue; returns the number of checks made"""
    b = make_backend(dims, ybc)
    fields, arrays = random_blocks(b, dims, 5, 7)
    real = real_dtype()
    inv_dt = real.type(1.0 / DT)
    checks = 0
    for scale, out_dtype in ((1.0, np.float64), (1.0 / DT, real), (1.0 / DT, np.float32)):
        got, tail = pack(b, [("copy", f, scale) for f in fields], dims, first, stride, out_dtype)
        assert np.all(tail == 0xA5), "bytes behind the last variable were written"
        for k, a in enumerate(arrays):
            want = snapshot_ref.strided(a, first, stride).astype(real)
            if scale != 1.0:
                want = want * inv_dt  # rounded once in the working precision
            assert same_bits(got[k], np.ascontiguousarray(want.astype(out_dtype))), (dims, stride, first, scale, out_dtype, k)
            checks += 1
    return checks


def derived_case(dims, ybc, stride, first, against_existing=False):
    """VORT and QCRIT in one launch against snapshot_ref in float64; returns rows (name, err / bound max, 1.0)"""
    from x3d2_amd.common import DIR_X, VERT
    b = make_backend(dims, ybc)
    g, arrays = random_blocks(b, dims, 9, 19)
    eps = eps_real()
    kept = [snapshot_ref.strided(a, first, stride) for a in arrays]
    ref = {"vort": snapshot_ref.vorticity(kept), "qcrit": snapshot_ref.qcriterion(kept)}
    mag = {"vort": np.abs(ref["vort"]), "qcrit": snapshot_ref.q_scale(kept)}
    rows = []
    for out_dtype in (real_dtype(), np.float32):
        got, tail = pack(b, [("vort", g), ("qcrit", g)], dims, first, stride, out_dtype)
        assert np.all(tail == 0xA5)
        for k, name in enumerate(("vort", "qcrit")):
            bound = 8 * eps * mag[name]
            if np.dtype(out_dtype) == np.float32:
                bound = bound + 2.0 ** -24 * np.abs(ref[name])
            err = np.abs(got[k].astype(np.float64) - ref[name])
            ratio = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
            rows.append(("%s %s" % (name, np.dtype(out_dtype).name), ratio, 1.0))
    if against_existing:  # the parent's behaviour: whole-block compute_*, on the same blocks
        out = b.allocator.get_block(DIR_X, VERT)
        got, _ = pack(b, [("vort", g), ("qcrit", g)], dims, (0, 0, 0), (1, 1, 1), real_dtype())
        whole = [a for a in arrays]
        for k, (name, fn) in enumerate((("vort", b.compute_vorticity), ("qcrit", b.compute_qcriterion))):
            fn(out, *g)
            out.set_data_loc(VERT)
            old = b.get_field_data(out).astype(np.float64)
            m = np.abs(snapshot_ref.vorticity(whole)) if name == "vort" else snapshot_ref.q_scale(whole)
            ratio = float(np.max(np.abs(got[k].astype(np.float64) - old) / np.maximum(8 * eps * m, np.finfo(np.float64).tiny)))
            rows.append((name + " against compute_*", ratio, 1.0))
    return rows


def check_rows(rows):
    for r in rows:
        print("snapshot check:", *r)
    bad = [r for r in rows if not r[-2] <= r[-1]]
    assert not bad, bad


# ---------------------------------------------------------------- 1. pack, COPY
@pytest.mark.parametrize("dims,ybc,strides", SHAPES)
def test_pack_copy_is_bit_equal_to_the_numpy_slice(dims, ybc, strides):
    n = 0
    for stride in strides:
        for first in FIRSTS:
            if usable(dims, first):
                n += copy_case(dims, ybc, stride, first)
    assert n == 15 * len(strides) * len(FIRSTS)


def test_copy_ring_of_two_slots_waits_at_the_third_acquire():
    """CopyRing(b, 2) with 4 KiB slots on a fresh backend: three buffers of distinct bytes submitted without a poll in
    between.  The host waits once, at the third acquire; the callbacks run in submission order, each on its own bytes."""
    import torch
    from x3d2_amd.copyring import CopyRing
    b = make_backend((17, 6, 5))
    seen = []
    ring = CopyRing(b, 2, lambda k, raw: seen.append((k, raw.tobytes())) or k)
    patterns = [bytes((85 * k + 3 * i + 1) % 256 for i in range(4096)) for k in range(3)]
    assert ring.allocated == 0 and len(set(patterns)) == 3
    start = b.sync_count()
    for k, p in enumerate(patterns):
        n0 = b.sync_count()
        slot = ring.acquire(4096)
        assert b.sync_count() - n0 == (1 if k == 2 else 0), k
        slot.dev.copy_(torch.frombuffer(bytearray(p), dtype=torch.uint8))
        ring.submit(slot, 4096, k)
    assert b.sync_count() - start == 1 and ring.waits == 1 and ring.allocated == 2
    assert seen == [(0, patterns[0])] and [k for _, k in ring.pending()] == [1, 2]
    assert ring.drain() == [1, 2] and ring.pending() == []
    assert seen == list(enumerate(patterns))


# ---------------------------------------------------------------- 2. pack, VORT and QCRIT
@pytest.mark.parametrize("dims,ybc,strides", SHAPES)
def test_pack_vorticity_and_qcriterion_within_the_rounding_bounds(dims, ybc, strides):
    rows = []
    for stride in strides:
        for first in FIRSTS[:2]:
            rows += derived_case(dims, ybc, stride, first, against_existing=(stride == (1, 1, 1) and first == (0, 0, 0)))
    check_rows(rows)


def test_bad_calls_raise_and_write_nothing():
    import torch
    from x3d2_amd.common import X3dError
    dims = (17, 6, 5)
    b = make_backend(dims)
    fields, _ = random_blocks(b, dims, 1, 1)
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=b.device)
    with pytest.raises(X3dError, match="outside dims"):
        b.snapshot_pack([("copy", fields[0], 1.0)], (0, 0, 0), (2, 1, 1), (10, 1, 1), out, np.float32)  # 0 + 9 * 2 = 18 > 16
    with pytest.raises(X3dError, match="smaller"):
        b.snapshot_pack([("copy", fields[0], 1.0)], (0, 0, 0), (1, 1, 1), (17, 6, 5), out[:64], np.float64)
    with pytest.raises(X3dError, match="unknown kind"):
        b.snapshot_pack([("curl", fields[0], 1.0)], (0, 0, 0), (1, 1, 1), (1, 1, 1), out, np.float64)
    with pytest.raises(X3dError, match="handle"):
        b.snapshot_wait(0)
    assert bool(torch.all(out == 0xA5))


# ---------------------------------------------------------------- 3. Snapshots end to end
STRIDE = (2, 1, 4)


def make_case(kind, fused):
    from x3d2_amd import make_channel, make_cylinder, make_tgv
    if kind == "tgv":
        return make_tgv(32, fused=fused)
    if kind == "channel":
        return make_channel((32, 33, 16), fused=fused)
    return make_cylinder((33, 16, 8), time_intg="AB3", fused=fused, centre=(5.0, 6.0), radius=1.3)


def composed_derived(s):
    """the composed path on the solver's velocity: nine operator calls, compute_*, a host copy each"""
    from x3d2_amd.common import DIR_X, DIR_Y, DIR_Z, VERT
    b, al = s.backend, s.backend.allocator
    s.flush_grad()
    g = []
    for f in (s.u, s.v, s.w):
        for dirps, d in ((s.xdirps, DIR_X), (s.ydirps, DIR_Y), (s.zdirps, DIR_Z)):
            o = al.get_block(DIR_X, VERT)
            b.tds_apply(o, f, dirps.der1st, d)
            g.append(o)
    out = al.get_block(DIR_X, VERT)
    res = {}
    for name, fn in (("vort", b.compute_vorticity), ("qcrit", b.compute_qcriterion)):
        fn(out, *g)
        out.set_data_loc(VERT)
        res[name] = b.get_field_data(out).astype(np.float64)
    grads = []
    for o in g:
        o.set_data_loc(VERT)
        grads.append(b.get_field_data(o).astype(np.float64))
    for f in g + [out]:
        al.release_block(f)
    return res, grads


def pressure_vert_host(s):
    """interpl_c2v(solver.pressure) through the backend's own operators, then * (1 / dt) in the working precision"""
    from x3d2_amd.common import DIR_X, DIR_Y, DIR_Z, VERT
    b, al = s.backend, s.backend.allocator
    t1, t2 = al.get_block(DIR_X, VERT), al.get_block(DIR_X, VERT)
    b.tds_apply(t1, s.pressure, s.zdirps.interpl_p2v, DIR_Z)
    b.tds_apply(t2, t1, s.ydirps.interpl_p2v, DIR_Y)
    b.tds_apply(t1, t2, s.xdirps.interpl_p2v, DIR_X)
    t1.set_data_loc(VERT)
    a = b.get_field_data(t1)
    for f in (t1, t2):
        al.release_block(f)
    return a * real_dtype().type(1.0 / s.dt)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kind", ["tgv", "channel", "cylinder"])
def test_snapshots_end_to_end(kind, fused, tmp_path):
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots
    fields = ("pressure", "vorticity", "qcriterion") + (("ibm",) if kind == "cylinder" else ())
    names = ["u", "v", "w", "p", "vort", "qcrit"] + (["ibm"] if kind == "cylinder" else [])
    prefix = str(tmp_path / "snapshot")
    cfg = dict(snapshot_freq=2, snapshot_prefix=prefix, output_stride=STRIDE, output_fields=fields)
    case = make_case(kind, fused)
    case.snapshots = Snapshots(case.solver, SnapshotConfig(**cfg))
    case.run(n_iters=4)
    assert case.snapshots.files == [prefix + "_000002.npz", prefix + "_000004.npz"]
    dims = tuple(int(n) for n in case.solver.mesh.vert_dims)
    shape = counts(dims, (0, 0, 0), STRIDE)
    eps, rows = eps_real(), []
    # a second, identical case stopped at the same iterations: its fields are what the files must hold
    twin = make_case(kind, fused)
    twin.snapshots = Snapshots(twin.solver, SnapshotConfig(**dict(cfg, snapshot_prefix=str(tmp_path / "twin"))))
    for stop in (2, 4):
        f = np.load(prefix + "_%06d.npz" % stop)
        meta = ["time", "iteration", "stride", "shape", "start", "count", "origin", "spacing", "vtk.xml"]
        assert sorted(f.files) == sorted(names + meta)
        assert int(f["iteration"]) == stop and float(f["time"]) == stop * case.solver.dt
        assert tuple(f["stride"]) == STRIDE and tuple(f["shape"]) == shape == tuple(f["count"]) and tuple(f["start"]) == (0, 0, 0)
        assert np.array_equal(f["spacing"], case.solver.mesh.d * np.array(STRIDE))
        assert str(f["vtk.xml"]) == case.snapshots.vtk_xml and '<DataArray Name="qcrit">' in str(f["vtk.xml"])
        for n in names:
            assert f[n].shape == shape[::-1] and f[n].dtype == real_dtype(), n
        twin.run(n_iters=stop)
        s = twin.solver
        for n, fld in (("u", s.u), ("v", s.v), ("w", s.w)):
            assert same_bits(f[n], np.ascontiguousarray(snapshot_ref.strided(s.backend.get_field_data(fld), (0, 0, 0), STRIDE))), (n, stop)
        res, grads = composed_derived(s)
        kept = [snapshot_ref.strided(a, (0, 0, 0), STRIDE) for a in grads]
        for n, mag in (("vort", np.abs(snapshot_ref.vorticity(kept))), ("qcrit", snapshot_ref.q_scale(kept))):
            err = np.abs(f[n].astype(np.float64) - snapshot_ref.strided(res[n], (0, 0, 0), STRIDE))
            rows.append(("%s it %d" % (n, stop), float(np.max(err / np.maximum(8 * eps * mag, np.finfo(np.float64).tiny))), 1.0))
        assert s.pressure is not None
        assert same_bits(f["p"], np.ascontiguousarray(snapshot_ref.strided(pressure_vert_host(s), (0, 0, 0), STRIDE))), stop
        assert float(np.max(np.abs(f["p"]))) > 0.0
        if kind == "cylinder":
            assert same_bits(f["ibm"], np.ascontiguousarray(snapshot_ref.strided(s.ibm.ep1.astype(real_dtype()), (0, 0, 0), STRIDE)))
            assert float(f["ibm"].min()) == 0.0 and float(f["ibm"].max()) == 1.0
    check_rows(rows)
    if fused:  # (channel: the interleaved 010 branch serves the steps whose pressure is not kept)
        print("snapshot check: corrections through the interleaved / z-first solve", case.solver.n_interleaved, case.solver.n_zfirst)


# ---------------------------------------------------------------- 4. fused against op-granular pressure
def test_fused_and_op_granular_pressure_agree():
    """one AB1 step from one saved state (TGV 32^3 advanced two RK3 steps) in each driver; p is one inverse-Laplacian
    solve from the same u*, and the solve damps every mode but the lowest, so rel dp <= 10 rel du (floor 64 eps), the
    difference of the corrected u between the two drivers being measured in this same test.
    Measured on an MI355X, FP64: rel du = 0, rel dp = 0 -- at this size both drivers give the same bits
    (profiles/README.md, "Snapshots")."""
    from x3d2_amd import make_tgv
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots
    start = make_tgv(32, fused=True)
    start.run(n_iters=2)
    sv = start.solver
    state = [sv.backend.get_field_data(f) for f in (sv.u, sv.v, sv.w)]
    out = {}
    for fused in (True, False):
        case = make_tgv(32, fused=fused, time_intg="AB1")
        s = case.solver
        for f, a in zip((s.u, s.v, s.w), state):
            s.backend.set_field_data(f, a)
        case.snapshots = Snapshots(s, SnapshotConfig(snapshot_freq=1, snapshot_prefix=os.devnull, output_fields=("pressure",)))
        case.step(1, want_pressure=True)
        s.flush_grad()
        out[fused] = (s.backend.get_field_data(s.u).astype(np.float64), pressure_vert_host(s).astype(np.float64))
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    du, dp = rel(out[True][0], out[False][0]), rel(out[True][1], out[False][1])
    print("snapshot check: fused against op-granular, rel du %.3e rel dp %.3e" % (du, dp))
    assert dp <= max(10 * du, 64 * eps_real()), (du, dp)


# ---------------------------------------------------------------- 5. no host wait
def test_write_does_not_wait_for_the_host(tmp_path):
    from x3d2_amd import make_tgv
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots
    prefix = str(tmp_path / "snapshot")
    case = make_tgv(32, fused=True)
    s, b = case.solver, case.solver.backend
    snap = Snapshots(s, SnapshotConfig(snapshot_freq=1, snapshot_prefix=prefix, output_stride=(1, 2, 2),
                                       output_fields=("vorticity", "qcriterion")))
    want = {}
    for it, expect in ((1, 0), (2, 0), (3, 1)):  # the third snapshot without a poll in between waits for the first
        case.step(it)
        want[it] = [snapshot_ref.strided(b.get_field_data(f), (0, 0, 0), (1, 2, 2)) for f in (s.u, s.v, s.w)]
        n0 = b.sync_count()
        assert snap.write(it)
        assert b.sync_count() - n0 == expect, it
    assert snap.files == [prefix + "_000001.npz"]
    snap.finalise()
    assert snap.files == [prefix + "_%06d.npz" % it for it in (1, 2, 3)]
    for it in (1, 2, 3):
        f = np.load(prefix + "_%06d.npz" % it)
        for n, a in zip("uvw", want[it]):
            assert same_bits(f[n], np.ascontiguousarray(a)), (it, n)
        assert float(np.max(f["vort"])) > 0.0
    assert snap.poll() == [] and snap.finalise() == []


def test_nothing_changes_without_snapshots(tmp_path):
    """a 2-step TGV 32^3 run with no Snapshots and with an attached Snapshots that is never due: the same bits, the same
    number of host waits and z-first solves, the same blocks taken"""
    from x3d2_amd import make_tgv
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots
    res = []
    for cfg in (None, SnapshotConfig(snapshot_prefix=str(tmp_path / "s"))):
        case = make_tgv(32, fused=True)
        assert case.snapshots is None and case.solver.keep_pressure is False and case.solver.pressure is None
        if cfg is not None:
            case.snapshots = Snapshots(case.solver, cfg)
        free = len(case.solver.backend.allocator.free)
        case.run(n_iters=2)
        s = case.solver
        res.append(([s.backend.get_field_data(f) for f in (s.u, s.v, s.w)], s.backend.sync_count(), s.n_zfirst,
                    len(s.backend.allocator.free) - free))
        assert s.pressure is None
    for other in res[1:]:
        for a, c in zip(res[0][0], other[0]):
            assert same_bits(a, c)
    assert res[0][1:] == res[1][1:]


# ---------------------------------------------------------------- 6. two ranks, 7. the FP32 flavour
def test_two_ranks_sharing_the_gpu(tmp_path):
    """dims (16, 12, 20) on two z slabs, stride (1, 2, 3): rank 1's offset of 10 is not a multiple of 3, its first kept
    plane is local index 2; load_snapshot of the two pieces equals the one-rank snapshot of the same fields"""
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots, load_snapshot
    dims, stride = (16, 12, 20), (1, 2, 3)
    out = str(tmp_path / "mp")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", "29543", os.path.join(HERE, "mp_snapshot_worker.py"),
           ",".join(map(str, dims)), ",".join(map(str, stride)), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(out + "_000003.r0.npz") and os.path.exists(out + "_000003.r1.npz")
    with np.load(out + "_000003.r1.npz") as z:
        assert tuple(z["start"]) == (0, 0, 4) and tuple(z["count"]) == (16, 6, 3)
    two = load_snapshot(out, 3)
    b = make_backend(dims, WALL)
    s = Fields(b)
    s.dt = 1e-3
    rng = np.random.default_rng(31)
    s.set([rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(3)])
    one_prefix = str(tmp_path / "one")
    snap = Snapshots(s, SnapshotConfig(snapshot_freq=3, snapshot_prefix=one_prefix, output_stride=stride))
    assert snap.write(3) and snap.finalise() == [one_prefix + "_000003.npz"]
    one = load_snapshot(one_prefix, 3)
    assert tuple(two["shape"]) == tuple(one["shape"]) == (16, 6, 7)
    for n in "uvw":
        assert same_bits(two[n], one[n]), n
    assert str(two["vtk.xml"]) == str(one["vtk.xml"])


def test_pack_in_the_fp32_flavour():
    """tests 1 and 2 at one shape on 4-byte reals (libx3d2_hip_sp.so), in a process of its own; the 8-byte output
    converts upward"""
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "snapshot_sp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("SNAPRESULT ")][-1][11:])
    assert res["eps"] == float(np.finfo(np.float32).eps) and res["copy_checks"] == 15 * 2 * len(FIRSTS)
    check_rows([tuple(x) for x in res["derived"]])
