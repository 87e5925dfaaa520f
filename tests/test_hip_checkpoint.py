"""Checkpoints on the device (csrc/checkpoint.hip, x3d2_amd/checkpoint.py): the pack / sums / unpack kernels against
get_field_data and tests/checkpoint_ref.py, and exact resume of every driver and case.  Every comparison is of bits or
integers: there are no tolerances."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import checkpoint_ref as ref
from test_hip_snapshot import same_bits
from test_hip_stats import PER, WALL, make_backend

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [((17, 6, 5), PER),     # odd rows: the scalar tail, dense rows off the 16-byte grid
          ((64, 5, 3), PER),     # pitch a multiple of 64
          ((33, 33, 4), WALL),   # walls in y, more than one workgroup per block
          ((257, 3, 2), PER)]    # a row longer than one pass of a wave, odd
NBLOCKS = (1, 3, 13, 64)


# ---------------------------------------------------------------- helpers (also used by the worker processes)
def real_dtype():
    from x3d2_amd import _lib
    return np.dtype(_lib.NP_REAL)


def random_blocks(b, n, seed):
    """n blocks filled with random bits of finite numbers, padding included (so that a pack that reads a wrong element
    cannot find a zero there); returns the fields"""
    import torch
    from x3d2_amd.common import DIR_X, VERT
    fields = [b.allocator.get_block(DIR_X, VERT) for _ in range(n)]
    g = torch.Generator(device="cpu").manual_seed(seed)
    for f in fields:
        f.data.copy_(torch.randn(f.data.numel(), generator=g, dtype=torch.float64).to(f.data.dtype))
    return fields


def kernel_case(dims, ybc, nblock):
    """the checks of section 1 for one shape and block count; returns the number of comparisons made"""
    import torch
    from x3d2_amd.common import DIR_X, VERT
    b = make_backend(dims, ybc)
    real = real_dtype()
    fields = random_blocks(b, nblock, 100 + nblock)
    planted = {}
    if nblock >= 3:  # NaN / Inf in two blocks
        planted = {0: [(1, 2, 3, np.nan), (0, 0, 0, np.inf)], nblock - 1: [(dims[2] - 1, dims[1] - 1, dims[0] - 1, -np.inf)]}
        for k, pts in planted.items():
            a = b.get_field_data(fields[k])
            for z, y, x, v in pts:
                a[z, y, x] = v
            b.set_field_data(fields[k], a)
    want = [b.get_field_data(f) for f in fields]
    n = int(np.prod(dims))
    data, off, total = b.checkpoint_layout(nblock, n)
    buf = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=b.device)
    n0 = b.sync_count()
    assert b.checkpoint_pack(fields, dims, buf) == total and b.sync_count() == n0
    raw = buf.cpu().numpy()
    got = raw[:data].view(real).reshape(nblock, dims[2], dims[1], dims[0])
    checks = 0
    for k in range(nblock):
        assert same_bits(got[k], want[k]), (dims, nblock, k)
        checks += 1
    assert np.all(raw[data:off] == 0xA5) and np.all(raw[total:] == 0xA5), "bytes outside data and table were written"
    table = raw[off:total].view(np.uint64).reshape(nblock, 3)
    assert np.array_equal(table, ref.table(want)), (dims, nblock)
    assert [int(v) for v in table[:, 2]] == [len(planted.get(k, ())) for k in range(nblock)]
    # the sums of the packed buffer alone
    buf[off:total] = 0x5A
    b.checkpoint_sums(buf, nblock, n)
    assert np.array_equal(b.checkpoint_table(buf, nblock, n), table)
    # unpack into blocks full of a sentinel: interior = the source bits, every other element +0.0
    outs = [b.allocator.get_block(DIR_X, VERT) for _ in range(nblock)]
    for f in outs:
        f.data.fill_(-7.5)
    b.checkpoint_unpack(outs, dims, buf)
    nxp, nyp, nzp = b.padded_dims
    for k, f in enumerate(outs):
        whole = f.data.cpu().numpy().reshape(nzp, nyp, nxp)
        assert same_bits(np.ascontiguousarray(whole[:dims[2], :dims[1], :dims[0]]), want[k]), (dims, nblock, k)
        rest = whole.copy().view(np.uint32 if real.itemsize == 4 else np.uint64)
        rest[:dims[2], :dims[1], :dims[0]] = 0
        assert not np.any(rest), "an element outside the interior is not +0.0"
        checks += 2
    return checks


# ---------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("nblock", NBLOCKS)
@pytest.mark.parametrize("dims,ybc", SHAPES)
def test_pack_sums_unpack(dims, ybc, nblock):
    assert kernel_case(dims, ybc, nblock) == 3 * nblock


def test_cell_dims_leave_rows_and_planes_zero():
    """dims smaller than the block's vertex extent (the cell extent of a walled direction): the rows beyond are zeroed"""
    import torch
    from x3d2_amd.common import DIR_X, VERT
    b = make_backend((33, 33, 4), WALL)
    fields = random_blocks(b, 2, 3)
    dims = (33, 32, 4)
    n = int(np.prod(dims))
    data, off, total = b.checkpoint_layout(2, n)
    buf = torch.zeros(total, dtype=torch.uint8, device=b.device)
    b.checkpoint_pack(fields, dims, buf)
    want = [b.get_field_data(f)[:, :32, :] for f in fields]
    raw = buf.cpu().numpy()
    assert np.array_equal(raw[off:total].view(np.uint64).reshape(2, 3), ref.table(want))
    b.checkpoint_unpack(fields, dims, buf)
    nxp, nyp, nzp = b.padded_dims
    for f, a in zip(fields, want):
        whole = f.data.cpu().numpy().reshape(nzp, nyp, nxp)
        assert same_bits(np.ascontiguousarray(whole[:, :32, :33]), np.ascontiguousarray(a))
        assert not np.any(whole[:, 32:, :]) and not np.any(whole[:, :, 33:])


def test_65_blocks_are_an_error_and_nothing_is_launched():
    import torch
    from x3d2_amd.common import X3dError
    dims = (17, 6, 5)
    b = make_backend(dims, PER)
    f = random_blocks(b, 1, 1)
    _, _, total = b.checkpoint_layout(65, int(np.prod(dims)))
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=b.device)
    with pytest.raises(X3dError, match="64"):
        b.checkpoint_pack(f * 65, dims, buf)
    import ctypes
    tab = (ctypes.c_void_p * 65)(*[f[0].ptr] * 65)
    from x3d2_amd import _lib
    rc = b.lib.x3d_checkpoint_pack(b.h, tab, 65, _lib.ints(*dims), buf.data_ptr(),
                                   ctypes.cast(buf.data_ptr() + total - 65 * 24, ctypes.POINTER(ctypes.c_ulonglong)))
    assert rc != 0 and b"64" in b.lib.x3d_last_error()
    assert bool(torch.all(buf == 0xA5))


# ---------------------------------------------------------------- 2. exact resume
def make_case(kind, **kw):
    from x3d2_amd import make_channel, make_cylinder, make_tgv
    if kind == "tgv":
        case = make_tgv(32, **kw)
        if case.solver.species:
            from mp_gpu_worker import set_species
            set_species(case)
    elif kind == "channel":
        case = make_channel((32, 33, 16), inlet_noise=(0.125, 0.25, 0.5), seed=1234, **kw)
    else:
        case = make_cylinder((33, 16, 8), centre=(5.0, 6.0), radius=1.3, **kw)
    case.solver.n_output = 1  # a monitoring row per step
    return case


def fields_of(case):
    s = case.solver
    return [s.backend.get_field_data(f) for f in [s.u, s.v, s.w] + list(s.species)]


def run_pair(kind, tmp_path, stats_cfg=None, n_output=1, **kw):
    """run A: 6 steps with checkpoint_freq = 3; run B: a fresh case restored from checkpoint_000003, run to step 6"""
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    from x3d2_amd.stats import Stats
    prefix = str(tmp_path / "checkpoint")
    cases = []
    for restart in (False, True):
        case = make_case(kind, **kw)
        case.solver.n_output = n_output
        if stats_cfg is not None:
            case.stats = Stats(case.solver, stats_cfg)
        if restart:
            assert restore(case, prefix + "_000003.npz") == 3 and case.solver.current_iter == 3
        else:
            case.checkpoints = Checkpoints(case.solver, CheckpointConfig(checkpoint_freq=3, checkpoint_prefix=prefix), case)
        case.run(n_iters=6)
        cases.append(case)
    assert cases[0].checkpoints.files == [prefix + "_000003.npz", prefix + "_000006.npz"]
    return cases


def assert_same_run(a, c, n_output=1):
    for k, (x, y) in enumerate(zip(fields_of(a), fields_of(c))):
        assert same_bits(x, y), "variable %d differs after the resume" % k
    if n_output == 1:
        assert len(a.monitoring.rows) == 7 and len(c.monitoring.rows) == 4
        assert a.monitoring.rows[3:] == c.monitoring.rows  # step 3 (written again at the restart) and steps 4 - 6


CONFIGS = [("tgv", dict(time_intg="RK3", fused=True)), ("tgv", dict(time_intg="RK3", fused=False)),
           ("tgv", dict(time_intg="AB3", fused=True)), ("tgv", dict(time_intg="AB3", fused=False)),
           ("tgv", dict(time_intg="AB4", fused=True)), ("tgv", dict(time_intg="AB4", fused=False)),
           ("tgv", dict(time_intg="AB3", fused=False, lazy=True)),
           ("tgv", dict(time_intg="AB3", fused=True, n_species=1, pr_species=[0.7])),
           ("channel", dict(fused=True)), ("cylinder", dict(time_intg="AB3", fused=True))]


@pytest.mark.parametrize("kind,kw", CONFIGS, ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v.values()))
def test_exact_resume(kind, kw, tmp_path):
    a, c = run_pair(kind, tmp_path, **kw)
    assert_same_run(a, c)
    if kind == "cylinder":
        assert len(a.outflow_rows) == 7 and a.outflow_rows[3:] == c.outflow_rows
    if kind == "channel":
        assert a.noise_draws == c.noise_draws > 0


def test_exact_resume_across_deferred_corrections(tmp_path):
    """no output step: the fused driver leaves the velocity correction pending from step to step, except where the
    checkpoint is due"""
    a, c = run_pair("tgv", tmp_path, n_output=0, time_intg="RK3", fused=True)
    assert_same_run(a, c, n_output=0)


@pytest.mark.parametrize("kind,kw", [("tgv", dict(time_intg="AB3", fused=True)), ("cylinder", dict(time_intg="AB3", fused=True))],
                         ids=["tgv-AB3", "cylinder"])
def test_control_u_v_w_alone_do_not_resume(kind, kw, tmp_path):
    """restore only u, v, w and current_iter through set_field_data: the run differs from the uninterrupted one, so the
    history and gdt in the checkpoint matter"""
    from x3d2_amd.checkpoint import read_checkpoint
    a, c = run_pair(kind, tmp_path, **kw)
    z = read_checkpoint(str(tmp_path / "checkpoint_000003.npz"))
    d = make_case(kind, **kw)
    s = d.solver
    for f, n in zip((s.u, s.v, s.w), "uvw"):
        s.backend.set_field_data(f, z[n])
    s.current_iter = 3
    d.run(n_iters=6)
    assert not all(same_bits(x, y) for x, y in zip(fields_of(a), fields_of(d)))


def test_restart_needs_more_iterations(tmp_path):
    from x3d2_amd.checkpoint import CheckpointConfig, restart_from_checkpoint
    from x3d2_amd.common import X3dError
    a, c = run_pair("tgv", tmp_path, time_intg="RK3", fused=True)
    d = make_case("tgv", time_intg="RK3", fused=True)
    cfg = CheckpointConfig(restart_from_checkpoint=True, restart_file=str(tmp_path / "checkpoint_000006.npz"))
    assert restart_from_checkpoint(d, cfg) == 6
    with pytest.raises(X3dError, match="Restart requires n_iters greater than the restart iteration"):
        d.run(n_iters=6)


# ---------------------------------------------------------------- 3. statistics
@pytest.mark.parametrize("profile_dir", [None, 2])
def test_statistics_resume(profile_dir, tmp_path):
    from x3d2_amd.stats import StatsConfig
    cfg = StatsConfig(initstat=1, istatfreq=1, profile_dir=profile_dir)
    a, c = run_pair("channel", tmp_path, stats_cfg=cfg, fused=True)
    assert_same_run(a, c)
    assert a.stats.sample_count == c.stats.sample_count == 6
    ma, mc = a.stats.means(), c.stats.means()
    assert sorted(ma) == sorted(mc) and len(ma) == 9
    for k in ma:
        assert same_bits(ma[k], mc[k]), k


# ---------------------------------------------------------------- 4. no host wait, 5. the guard, 6. detection
def test_write_does_not_wait_for_the_host(tmp_path):
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints
    case = make_case("tgv", time_intg="AB3", fused=True)
    s, b = case.solver, case.solver.backend
    ck = Checkpoints(s, CheckpointConfig(checkpoint_freq=1, checkpoint_prefix=str(tmp_path / "ck")), case)
    assert ck.ring.allocated == 0
    for it, expect in ((1, 0), (2, 1)):  # the second checkpoint without a poll in between waits for the first
        case.step(it)
        s.current_iter = it
        n0 = b.sync_count()
        assert ck.write(it)
        assert b.sync_count() - n0 == expect, it
    assert ck.files == [str(tmp_path / "ck_000001.npz")]
    assert ck.finalise() == [str(tmp_path / "ck_000002.npz")]


def test_a_nan_is_written_aside_and_the_good_checkpoint_survives(tmp_path):
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, read_checkpoint
    case = make_case("tgv", time_intg="RK3", fused=True)
    s, b = case.solver, case.solver.backend
    ck = Checkpoints(s, CheckpointConfig(checkpoint_freq=1, checkpoint_prefix=str(tmp_path / "ck"), keep_checkpoint=False), case)
    case.step(1)
    assert ck.write(1) and ck.finalise() == [str(tmp_path / "ck_000001.npz")]
    w = b.get_field_data(s.w)
    w[3, 4, 5] = np.nan
    b.set_field_data(s.w, w)  # (planted, the solver is not run on it)
    assert ck.write(2) and ck.finalise() == [str(tmp_path / "ck_000002.nonfinite.npz")]
    assert sorted(os.listdir(tmp_path)) == ["ck_000001.npz", "ck_000002.nonfinite.npz"]
    assert [int(v) for v in read_checkpoint(ck.files[-1])["checksums"][:, 2]] == [0, 0, 1]


def test_a_flipped_bit_is_found_before_the_solver_is_touched(tmp_path):
    from x3d2_amd.checkpoint import read_checkpoint, restore
    from x3d2_amd.common import X3dError
    a, c = run_pair("tgv", tmp_path, time_intg="AB3", fused=True)
    path = str(tmp_path / "checkpoint_000003.npz")
    z = read_checkpoint(path)
    u = z["u"].copy()
    u.view(np.uint32 if u.dtype.itemsize == 4 else np.uint64)[5, 6, 7] ^= 1 << 9
    z["u"] = u
    np.savez(path, **z)
    d = make_case("tgv", time_intg="AB3", fused=True)
    before = fields_of(d)
    with pytest.raises(X3dError, match="`u`"):
        restore(d, path)
    assert d.solver.current_iter == 0 and d.solver.time_integrator.istep == 1 and not d.restarted
    for x, y in zip(before, fields_of(d)):
        assert same_bits(x, y)


# ---------------------------------------------------------------- 7. two ranks, 8. the FP32 flavour
def _two_ranks(mode, prefix, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(HERE, "mp_checkpoint_worker.py"), mode, prefix]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_two_ranks_sharing_the_gpu(tmp_path):
    """TGV 32^3 on [1, 2, 1], RK3 fused: per-rank files; the resumed two-rank run has the bits of the uninterrupted one;
    a rank's file does not restore on one rank"""
    from x3d2_amd.checkpoint import restore
    from x3d2_amd.common import X3dError
    prefix = str(tmp_path / "mp")
    _two_ranks("run", prefix, 29547)
    for r in (0, 1):
        assert os.path.exists("%s_000003.r%d.npz" % (prefix, r)) and os.path.exists("%s_000006.r%d.npz" % (prefix, r))
    assert not os.path.exists(prefix + "_000003.npz")
    _two_ranks("resume", prefix, 29548)
    for r in (0, 1):
        with np.load("%s.final.run.%d.npz" % (prefix, r)) as x, np.load("%s.final.resume.%d.npz" % (prefix, r)) as y:
            for n in "uvw":
                assert same_bits(x[n], y[n]), (r, n)
    one = make_case("tgv", time_intg="RK3", fused=True)
    with pytest.raises(X3dError, match="dims|nproc_dir"):
        restore(one, prefix + "_000003.r0.npz")


def test_checkpoints_in_the_fp32_flavour(tmp_path):
    """the kernels at (17, 6, 5) and (64, 5, 3) and one AB3 resume on 4-byte reals (libx3d2_hip_sp.so), in a process of
    its own"""
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "checkpoint_sp_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("CKPTRESULT ")][-1][11:])
    assert res == {"real_bytes": 4, "kernel_checks": 2 * sum(3 * n for n in NBLOCKS), "resume": True}
