"""Device-resident flow statistics (csrc/stats.hip, x3d2_amd/stats.py) against the numpy restatement of the reference's
stats_manager_t (tests/stats_ref.py, pinned to the reference's known answers by tests/test_stats_host.py).

Bounds (none is tuned to the kernels):
  3-D update   |err| <= (n + 4) eps max|val| after n samples, max|val| the largest sampled value of the moment: one update
               commits at most eps (|mean| + 2 |val - mean| / k); the recurrence gives err_n = (1/n) sum k delta_k
               <= ((n + 1) / 2 + 2) eps max|val|; n + 4 doubles that (covers the product fused into the subtraction).
  derive       8 eps max(uu).
  profiles     (n + 4 + P) eps max|val|, P = points per plane: the worst case of ANY summation order.  One dropped or
               doubled point moves a plane mean by |val| / P, orders of magnitude more."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import stats_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2


# ---------------------------------------------------------------- helpers (also used by the worker processes)
class Fields:
    """the part of Solver that Stats reads: u, v, w, species, mesh, backend, flush_grad"""

    def __init__(self, backend, nspecies=0):
        from x3d2_amd.common import DIR_X, VERT
        self.backend, self.mesh = backend, backend.mesh
        self.u, self.v, self.w = (backend.allocator.get_block(DIR_X, VERT) for _ in range(3))
        self.species = [backend.allocator.get_block(DIR_X, VERT) for _ in range(nspecies)]
        self.flushes = 0

    def flush_grad(self):
        self.flushes += 1

    def set(self, arrays):
        for f, a in zip([self.u, self.v, self.w] + self.species, arrays):
            self.backend.set_field_data(f, a)


def make_backend(dims, ybc=PER, lazy=False, nproc_dir=(1, 1, 1), rank=0, comm=None):
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    mesh = Mesh(tuple(dims), nproc_dir, (1.0, 1.0, 1.0), PER, ybc, PER, nrank=rank)
    return HipBackend(mesh, lazy=lazy, comm=comm)


def eps_real():
    from x3d2_amd import _lib
    return float(np.finfo(np.dtype(_lib.NP_REAL)).eps)


def sample_arrays(dims, seed, count=3):
    """standard_normal fields [nz, ny, nx], exactly representable in both flavours"""
    rng = np.random.default_rng(seed)
    shape = (dims[2], dims[1], dims[0])
    return [rng.standard_normal(shape, dtype=np.float32).astype(np.float64) for _ in range(count)]


def zero_blocks(b, n):
    from x3d2_amd.common import DIR_X, VERT
    out = [b.allocator.get_block(DIR_X, VERT) for _ in range(n)]
    for f in out:
        f.fill(0.0)
    return out


def update_case(dims, ybc, checkpoints=(1, 7, 40), seed=11):
    """n samples through x3d_stats_update_uvw; at every checkpoint the nine accumulators against the float64 numpy
    recurrence.  Returns [(n, moment, err, bound)], and the backend + accumulators for further use."""
    b = make_backend(dims, ybc)
    s = Fields(b)
    means = zero_blocks(b, 9)
    ref, vmax, rows = None, [0.0] * 9, []
    eps = eps_real()
    for n in range(1, max(checkpoints) + 1):
        arrays = sample_arrays(dims, seed * 1000 + n)
        s.set(arrays)
        b.stats_update_uvw(s.u, s.v, s.w, means, 1.0 / n)
        vals = stats_ref.moments(*arrays)
        if ref is None:
            ref = [np.zeros_like(x) for x in vals]
        for k, x in enumerate(vals):
            vmax[k] = max(vmax[k], float(np.max(np.abs(x))))
            ref[k] += (x - ref[k]) * (1.0 / n)
        if n in checkpoints:
            for k, name in enumerate(stats_ref.MOMENTS):
                got = b.get_field_data(means[k]).astype(np.float64)
                rows.append((n, name, float(np.max(np.abs(got - ref[k]))), (n + 4) * eps * vmax[k]))
    return rows, b, s, means


def profile_case(dims, ybc, dir_keep, n=3, seed=5):
    """n samples through x3d_stats_profile_sums + _accumulate against numpy longdouble plane means; every sample's
    sums are formed twice and must agree bit for bit.  Returns [(moment, err, bound)]."""
    import torch
    from x3d2_amd import _lib
    b = make_backend(dims, ybc)
    s = Fields(b)
    nk = dims[dir_keep - 1]
    axes = tuple(a for a in range(3) if a != 3 - dir_keep)  # arrays are [z, y, x]
    P = int(np.prod([d for i, d in enumerate(dims) if i != dir_keep - 1]))
    z = lambda: torch.zeros(9 * nk, dtype=_lib.torch_real(), device=b.device)
    prof, sums, again = z(), z(), z()
    ref, vmax = [np.zeros(nk, dtype=np.longdouble) for _ in range(9)], [0.0] * 9
    for it in range(1, n + 1):
        arrays = sample_arrays(dims, seed * 1000 + it)
        s.set(arrays)
        b.stats_profile_sums(s.u, s.v, s.w, dir_keep, sums)
        b.stats_profile_sums(s.u, s.v, s.w, dir_keep, again)
        assert torch.equal(sums, again), "the profile reduction is not deterministic"
        b.stats_profile_accumulate(prof, sums, 1.0 / P, 1.0 / it)
        for k, x in enumerate(stats_ref.moments(*arrays)):
            vmax[k] = max(vmax[k], float(np.max(np.abs(x))))
            plane = x.astype(np.longdouble).sum(axis=axes) / np.longdouble(P)
            ref[k] += (plane - ref[k]) / np.longdouble(it)
    got = prof.view(9, nk).cpu().numpy()
    eps = eps_real()
    return [(name, float(np.max(np.abs(got[k].astype(np.longdouble) - ref[k]))), (n + 4 + P) * eps * vmax[k])
            for k, name in enumerate(stats_ref.MOMENTS)]


def check_rows(rows):
    for r in rows:
        print("stats check:", *r)
    bad = [r for r in rows if not r[-2] <= r[-1]]
    assert not bad, bad


# ---------------------------------------------------------------- 1. the fused update
@pytest.mark.parametrize("dims,ybc", [((32, 32, 32), PER), ((64, 33, 48), WALL), ((256, 256, 256), PER)])
def test_update_uvw_against_the_numpy_recurrence(dims, ybc):
    """all nine moments, element-wise over the unpadded extent, after 1, 7 and 40 samples of standard_normal fields"""
    rows, _, _, _ = update_case(dims, ybc)
    assert len(rows) == 27
    check_rows(rows)


def _worker(script, *args, timeout=600, env=None):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(HERE, script)] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("STATSRESULT ")][-1][12:])


def test_update_and_profiles_in_the_fp32_flavour():
    """the same case on 4-byte reals (libx3d2_hip_sp.so), in a process of its own: the bound scales with FP32's eps; the
    profile's partial sums are FP64 in both flavours and round once"""
    res = _worker("stats_sp_worker.py", env={"X3D_SINGLE_PREC": "1"})
    assert res["eps"] == float(np.finfo(np.float32).eps)
    assert len(res["update"]) == 27 and len(res["profile"]) == 9
    check_rows([tuple(r) for r in res["update"]])
    check_rows([tuple(r[:3]) for r in res["profile"]])
    # carried in FP64 and rounded once: what is left is the rounding of the sum, of its scaling and of the running-mean
    # recurrence -- the 3-D update's (n + 4) eps max|val|, without the P of an FP32 summation
    check_rows([(r[0], r[1], r[3]) for r in res["profile"]])


# ---------------------------------------------------------------- 2. the reference's known answers on the device
@pytest.mark.parametrize("name", sorted(stats_ref.SERIES))
def test_reference_series_on_the_device(name):
    """whole fields filled with the series of the reference's tests/unit/test_statistics.f90; its assertions, its tolerances"""
    n, fu, fv = stats_ref.SERIES[name]
    b = make_backend((32, 32, 32))
    s = Fields(b)
    means, outs = zero_blocks(b, 9), zero_blocks(b, 6)
    s.w.fill(0.0)
    for k in range(1, n + 1):
        s.u.fill(fu(k))
        s.v.fill(fv(k))
        b.stats_update_uvw(s.u, s.v, s.w, means, 1.0 / k)
    b.stats_derive(outs, means)
    stats_ref.check_series(name, [b.get_field_data(f) for f in means], [b.get_field_data(f) for f in outs])


# ---------------------------------------------------------------- 3. write-time fluctuations
def test_derive_against_numpy_on_the_accumulators():
    rows, b, s, means = update_case((64, 33, 48), WALL, checkpoints=(7,))
    outs = zero_blocks(b, 6)
    b.stats_derive(outs, means)
    host = [b.get_field_data(f).astype(np.float64) for f in means]
    bound = 8 * eps_real() * float(np.max(host[3]))
    check_rows([(n, float(np.max(np.abs(b.get_field_data(f) - w))), bound)
                for n, f, w in zip(("uprime", "vprime", "wprime", "uv", "uw", "vw"), outs, stats_ref.derive(host))])
    # the scalar entry point on the same samples of u: phi, phi^2 within the update's bound
    m1, m2 = zero_blocks(b, 2)
    us = []
    for n in range(1, 8):
        arrays = sample_arrays((64, 33, 48), 11 * 1000 + n)
        us.append(arrays[0])
        s.set(arrays)
        b.stats_update_scalar(s.u, m1, m2, 1.0 / n)
    ref = stats_ref.running_means((a, a, a) for a in us)
    check_rows([(name, float(np.max(np.abs(b.get_field_data(f) - ref[k]))),
                 (7 + 4) * eps_real() * max(float(np.max(np.abs(a))) ** p for a in us))
                for name, f, k, p in (("phi", m1, 0, 1), ("phiphi", m2, 3, 2))])
    only = zero_blocks(b, 1)[0]
    b.stats_update_scalar(s.u, only, None, 1.0)  # first moment only
    assert np.array_equal(b.get_field_data(only), b.get_field_data(s.u))


@pytest.mark.parametrize("consts,exact", [((1.0, 2.0, -0.5), True), ((0.1, 1.0 / 3.0, -0.7), False)])
def test_derive_clamps_a_constant_field(consts, exact):
    """constant fields, 100 samples.  Constants whose squares are exact (the reference's own case is c = 1): every mean
    is exact and uprime <= 1e-12.  Others: uu and u^2 each carry at most (n + 4) eps c^2 and 2 (n + 4) eps c^2, the
    difference has either sign, and the clamp must leave 0 <= uprime <= sqrt(3 (n + 4) eps) |c| -- never a NaN"""
    b = make_backend((32, 32, 32))
    s = Fields(b)
    means, outs = zero_blocks(b, 9), zero_blocks(b, 6)
    for f, c in zip((s.u, s.v, s.w), consts):
        f.fill(c)
    for k in range(1, 101):
        b.stats_update_uvw(s.u, s.v, s.w, means, 1.0 / k)
    b.stats_derive(outs, means)
    for f, c in zip(outs[:3], consts):
        a = b.get_field_data(f)
        print("stats check: uprime of a constant", c, float(np.max(a)))
        assert np.all(np.isfinite(a)) and float(np.min(a)) >= 0.0
        assert float(np.max(a)) <= (1e-12 if exact else np.sqrt(3 * 104 * eps_real()) * abs(c))


# ---------------------------------------------------------------- 4. profiles
@pytest.mark.parametrize("dir_keep", [1, 2, 3])
@pytest.mark.parametrize("dims", [(64, 33, 48), (1024, 257, 8)])
def test_profile_sums_against_longdouble_plane_means(dims, dir_keep):
    check_rows(profile_case(dims, WALL, dir_keep))


# ---------------------------------------------------------------- 5. the driver
def _case(kind, dims):
    from x3d2_amd import make_channel, make_tgv
    if kind == "tgv":
        return make_tgv(dims[0], fused=True)
    return make_channel(dims, fused=True, rotation=True, omega_rot=0.12, n_rotate=2)


def _run_with_stats(kind, dims, n_output, profile_dir=None):
    from x3d2_amd.stats import Stats, StatsConfig
    case = _case(kind, dims)
    case.solver.n_output = n_output
    case.stats = Stats(case.solver, StatsConfig(initstat=2, istatfreq=2, profile_dir=profile_dir))
    rows = case.run(n_iters=6)
    return case, np.array(rows)


@pytest.mark.parametrize("kind,dims", [("tgv", (32, 32, 32)), ("channel", (24, 33, 16)), ("channel", (1024, 33, 8))])
def test_driver_samples_the_right_fields_and_leaves_the_run_alone(kind, dims):
    """6 steps, RK3, fused driver, initstat = 2, istatfreq = 2: three samples, at iterations 2, 4 and 6"""
    # (a) the means are those of the fields of three runs without statistics that stop at 2, 4 and 6
    case, _ = _run_with_stats(kind, dims, 0)
    assert case.stats.sample_count == 3
    got = case.stats.means()
    plain = _case(kind, dims)
    snaps = []
    for stop in (2, 4, 6):
        plain.run(n_iters=stop)
        sv = plain.solver
        snaps.append([sv.backend.get_field_data(f).astype(np.float64) for f in (sv.u, sv.v, sv.w)])
    ref = stats_ref.running_means(snaps)
    eps, rows = eps_real(), []
    for k, name in enumerate(stats_ref.MEAN_NAMES):
        vmax = max(float(np.max(np.abs(stats_ref.moments(*s)[k]))) for s in snaps)
        rows.append((name, float(np.max(np.abs(got[name] - ref[k]))), (3 + 4) * eps * vmax))
    check_rows(rows)
    # (b) the monitoring rows of a run with statistics are those of the run without, bit for bit
    _, rows_stats = _run_with_stats(kind, dims, 2)
    plain2 = _case(kind, dims)
    plain2.solver.n_output = 2
    rows_plain = np.array(plain2.run(n_iters=6))
    assert rows_stats.shape == rows_plain.shape == (4, 4)
    assert np.array_equal(rows_stats, rows_plain)
    if kind != "channel":
        return
    # (c) the profile mode along y agrees with the plane means of the 3-D mode
    pcase, _ = _run_with_stats(kind, dims, 0, profile_dir=2)
    assert pcase.stats.sample_count == 3
    prof = pcase.stats.profiles()
    P = dims[0] * dims[2]
    rows = []
    for k, name in enumerate(stats_ref.MEAN_NAMES):
        vmax = max(float(np.max(np.abs(stats_ref.moments(*s)[k]))) for s in snaps)
        want = got[name].astype(np.longdouble).mean(axis=(0, 2))
        assert prof[name].shape == (dims[1],)
        rows.append((name, float(np.max(np.abs(prof[name] - want))), (3 + 4 + P) * eps * vmax))
    check_rows(rows)
    fl = pcase.stats.fluctuations()
    assert np.array_equal(prof["uprime"], fl["uprime"]) and np.array_equal(prof["uv"], fl["uvmean"])


# ---------------------------------------------------------------- 6. deferred execution
@pytest.mark.parametrize("profile_dir", [None, 2])
def test_update_behind_queued_blas1_calls_equals_the_eager_result(profile_dir):
    from x3d2_amd.stats import Stats, StatsConfig
    dims = (32, 32, 32)
    out = {}
    for lazy in (False, True):
        b = make_backend(dims, lazy=lazy)
        s = Fields(b, nspecies=1)
        s.set(sample_arrays(dims, 3, count=4))
        st = Stats(s, StatsConfig(initstat=1, profile_dir=profile_dir))
        for it in range(1, 4):
            b.vecadd(0.5, s.v, 1.0, s.u)   # recorded, not run, while the deferred layer is on
            b.vecmult(s.w, s.u)
            b.veccopy(s.species[0], s.w)
            b.field_scale(s.v, 1.25)
            st.update(it)
        if lazy:
            assert b.lazy_stats()["recorded"] >= 12
        assert s.flushes == 3 and st.sample_count == 3
        out[lazy] = st.means()
    assert sorted(out[True]) == sorted(out[False]) and len(out[True]) == 11
    for name in out[False]:
        assert np.array_equal(out[True][name], out[False][name]), name
        assert float(np.max(np.abs(out[False][name]))) > 0.0


# ---------------------------------------------------------------- 7. restart, output
@pytest.mark.parametrize("profile_dir", [None, 2])
def test_restart_continues_the_means_exactly(profile_dir, tmp_path):
    from x3d2_amd.stats import Stats, StatsConfig
    dims = (32, 20, 24)
    b = make_backend(dims, WALL)
    s = Fields(b, nspecies=1)
    cfg = StatsConfig(initstat=1, istatout=8, stats_prefix=str(tmp_path / "statistics"), profile_dir=profile_dir)
    whole = Stats(s, cfg)
    for it in range(1, 5):
        s.set(sample_arrays(dims, 100 + it, count=4))
        assert whole.update(it)
    state = whole.state_dict()
    assert int(state["stats_sample_count"]) == 4
    want = ["stats_sample_count"] + ["stats_" + n for n in stats_ref.MEAN_NAMES] + ["stats_phimean_1", "stats_phiphimean_1"]
    assert sorted(state) == sorted(want)  # write_checkpoint's names, src/io/stats.f90:315-357
    resumed = Stats(s, cfg)
    resumed.load_state_dict(state)
    for it in range(5, 9):
        s.set(sample_arrays(dims, 100 + it, count=4))
        whole.update(it)
        resumed.update(it)
    a, c = whole.means(), resumed.means()
    assert whole.sample_count == resumed.sample_count == 8
    for name in a:
        assert np.array_equal(a[name], c[name]), name
    assert whole.write(7) is None
    path = resumed.write(8)
    assert path == str(tmp_path / "statistics_000008.npz")
    f = np.load(path)
    names = ["sample_count", "umean", "vmean", "wmean", "uprime", "vprime", "wprime", "uvmean", "uwmean", "vwmean",
             "phimean_1", "phiprime_1"]  # write_stats' variables, src/io/stats.f90:245-288
    assert sorted(f.files) == sorted(names) and int(f["sample_count"]) == 8
    host = [a[n].astype(np.float64) for n in stats_ref.MEAN_NAMES]
    for n, w in zip(("uprime", "vprime", "wprime", "uvmean", "uwmean", "vwmean"), stats_ref.derive(host)):
        assert np.max(np.abs(f[n] - w)) <= 8 * eps_real() * float(np.max(host[3])), n
    assert np.array_equal(f["umean"], a["umean"])


# ---------------------------------------------------------------- 8. errors
def test_bad_calls_raise_and_do_nothing_else():
    import torch
    from x3d2_amd import _lib
    from x3d2_amd.common import CELL, VERT, X3dError
    dims = (32, 20, 24)
    b = make_backend(dims, WALL)
    s = Fields(b)
    s.set(sample_arrays(dims, 1))
    means = zero_blocks(b, 9)
    sums = torch.zeros(9 * 32, dtype=_lib.torch_real(), device=b.device)

    def untouched():
        return all(not np.any(b.get_field_data(f)) for f in means) and not bool(torch.any(sums != 0))

    s.v.set_data_loc(CELL)  # a non-VERT input (src/io/stats.f90:15-16)
    with pytest.raises(X3dError, match="VERT"):
        b.stats_update_uvw(s.u, s.v, s.w, means, 1.0)
    with pytest.raises(X3dError, match="VERT"):
        b.stats_profile_sums(s.u, s.v, s.w, 2, sums)
    s.v.set_data_loc(VERT)
    assert untouched()
    with pytest.raises(X3dError, match="one of u, v, w"):  # an accumulator aliased to an input
        b.stats_update_uvw(s.u, s.v, s.w, means[:4] + [s.w] + means[5:], 1.0)
    with pytest.raises(X3dError, match="same block"):
        b.stats_update_uvw(s.u, s.v, s.w, means[:8] + [means[2]], 1.0)
    with pytest.raises(X3dError, match="distinct"):
        b.stats_update_scalar(s.u, means[0], means[0], 1.0)
    with pytest.raises(X3dError, match="one of the accumulators"):
        b.stats_derive(means[:6], means)
    assert untouched()
    with pytest.raises(X3dError, match="dir_keep"):  # a bad dir_keep, at the Python layer ...
        b.stats_profile_sums(s.u, s.v, s.w, 4, sums)
    rc = b.lib.x3d_stats_profile_sums(b.h, s.u.ptr, s.v.ptr, s.w.ptr, _lib.ints(*dims), 0, sums.data_ptr())
    assert rc != 0 and b"dir_keep" in b.lib.x3d_last_error()  # ... and at the C ABI
    rc = b.lib.x3d_stats_profile_sums(b.h, s.u.ptr, s.v.ptr, s.w.ptr, _lib.ints(64, 20, 24), 1, sums.data_ptr())
    assert rc != 0 and b"outside the block" in b.lib.x3d_last_error()
    assert untouched()


# ---------------------------------------------------------------- 9. two ranks
def test_profiles_on_two_z_slabs_equal_the_one_rank_profiles(tmp_path):
    """two processes share the GPU and exchange through gloo (tests/mp_stats_worker.py): profiles along y (both other
    directions reduced, z over the two ranks) and along z (the kept direction is the decomposed one: every rank holds its
    rows) against the same samples on one rank"""
    from x3d2_amd.stats import Stats, StatsConfig
    dims, n = (32, 20, 24), 3
    out = str(tmp_path / "mp")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", "29541", os.path.join(HERE, "mp_stats_worker.py"),
           ",".join(map(str, dims)), str(n), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    parts = [dict(np.load(out + ".%d.npz" % k)) for k in range(2)]
    eps = eps_real()
    for dir_keep in (2, 3):
        b = make_backend(dims, WALL)
        s = Fields(b)
        st = Stats(s, StatsConfig(initstat=1, profile_dir=dir_keep))
        vmax = [0.0] * 9
        for it in range(1, n + 1):
            arrays = sample_arrays(dims, 200 + it)
            s.set(arrays)
            st.update(it)
            for k, x in enumerate(stats_ref.moments(*arrays)):
                vmax[k] = max(vmax[k], float(np.max(np.abs(x))))
        one = st.means()
        P = int(np.prod([d for i, d in enumerate(dims) if i != dir_keep - 1]))
        rows = []
        for k, name in enumerate(stats_ref.MEAN_NAMES):
            key = "d%d_%s" % (dir_keep, name)
            two = parts[0][key] if dir_keep == 2 else np.concatenate([parts[0][key], parts[1][key]])
            if dir_keep == 2:
                assert np.array_equal(parts[0][key], parts[1][key])  # every rank holds the global answer
            assert two.shape == one[name].shape
            rows.append((key, float(np.max(np.abs(two - one[name]))), (n + 4 + P) * eps * vmax[k]))
        check_rows(rows)
