"""Device-side budget moments (csrc/budget.hip, x3d2_amd/budgets.py) against the longdouble numpy restatement of
tests/budgets_ref.py.

Bound, per moment after n samples (not tuned to the kernel):   |err| <= (n + 4 + P) 2^-52 max|term|
with P the points per plane and max|term| the largest sampled product.  A plane sum of P terms in double, in ANY order,
is off by at most (P - 1) eps max|term| P to first order, i.e. its mean by (P - 1) eps max|term|; the scaling by 1 / P adds
one rounding; the recurrence mean += (x - mean) / k commits at most eps (|mean| + 2 |x - mean| / k) per update, which gives
((n + 1) / 2 + 2) eps max|term| after n updates -- n + 4 doubles that, as tests/test_hip_stats.py does.  The terms
themselves are exact: the fields are float32-representable and every factor is widened to double first (a product of two
is exact; the one further product or sum of a term rounds once, counted by the + 4).  It is the FP64 eps in BOTH flavours
of the library.  One dropped or doubled point moves a mean by |term| / P, orders of magnitude more."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import budgets_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2
EPS = 2.0 ** -52
P_SCALE = 200.0  # 1 / dt of the channel example
# (dims, y boundary, dir_keep): the smallest shapes at which each branch of the kernel can go wrong
SHAPES = [((35, 9, 6), PER, 2), ((35, 9, 6), PER, 3),       # odd tail; fewer rows than parts
          ((520, 5, 4), PER, 2), ((520, 5, 4), PER, 3),     # second trip of the 512-point lane loop
          ((64, 6, 5), PER, 2), ((64, 6, 5), PER, 3),       # padded pitch
          ((8, 33, 130), WALL, 2),                          # several rows per part: 4096 / 33 -> 125 parts < 130 rows
          ((8, 130, 33), PER, 3)]                           # the same, along z
IDS = ["%dx%dx%d-keep%d" % (d + (k,)) for d, _, k in SHAPES]


# ---------------------------------------------------------------- helpers (also used by the worker processes)
class Fields:
    """thirteen VERT blocks: u, v, w, p and the nine gradients"""

    def __init__(self, backend):
        from x3d2_amd.common import DIR_X, VERT
        self.backend, self.mesh = backend, backend.mesh
        blocks = [backend.allocator.get_block(DIR_X, VERT) for _ in range(13)]
        self.u, self.v, self.w, self.p = blocks[:4]
        self.grads = blocks[4:]

    def set(self, arrays):
        for f, a in zip([self.u, self.v, self.w, self.p] + self.grads, arrays):
            self.backend.set_field_data(f, a)


def make_backend(dims, ybc=PER, lazy=False, nproc_dir=(1, 1, 1), rank=0, comm=None):
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    mesh = Mesh(tuple(dims), nproc_dir, (1.0, 1.0, 1.0), PER, ybc, PER, nrank=rank)
    return HipBackend(mesh, lazy=lazy, comm=comm)


def sample_arrays(dims, seed):
    """thirteen standard_normal fields [nz, ny, nx] (u, v, w, p, nine gradients), exactly representable in both flavours;
    u is offset by 1 and v scaled by 0.125, so that the central moments are small differences of the raw ones"""
    rng = np.random.default_rng(seed)
    shape = (dims[2], dims[1], dims[0])
    a = [rng.standard_normal(shape, dtype=np.float32) for _ in range(13)]
    a[0] = a[0] + np.float32(1.0)
    a[1] = a[1] * np.float32(0.125)
    return [x.astype(np.float64) for x in a]


@functools.lru_cache(maxsize=None)
def reference(dims, dir_keep, n, seed=5):
    """(the running means [41, n_keep] in longdouble after n samples, max|term| per moment); computed once per shape"""
    d = dir_keep - 1
    samples, vmax = [], np.zeros(41)
    for it in range(1, n + 1):
        a = sample_arrays(dims, seed * 1000 + it)
        samples.append(budgets_ref.moments41(a[0], a[1], a[2], a[3], a[4:], d, P_SCALE))
        vmax = np.maximum(vmax, [float(np.max(np.abs(t))) for t in
                                 budgets_ref.terms41(a[0], a[1], a[2], a[3], a[4:], d, P_SCALE)])
    ref, vmax = budgets_ref.running_means(samples), vmax
    ref.setflags(write=False)
    vmax.setflags(write=False)
    return ref, vmax


def plane_points(dims, dir_keep):
    return int(np.prod([n for i, n in enumerate(dims) if i != dir_keep - 1]))


def new_sums(b, nk):
    import torch
    return torch.zeros(41 * nk, dtype=torch.float64, device=b.device)


def parity_case(dims, ybc, dir_keep, n=3, seed=5, with_p=True, lazy=False):
    """n samples through x3d_budget_profile_sums + _accumulate; every sample's sums are formed twice and must agree bit
    for bit.  Returns ([(moment, err, bound)], the running profile [41, n_keep], the last sample's sums [41, n_keep])."""
    import torch
    from x3d2_amd.budgets import MOMENT_NAMES
    b = make_backend(dims, ybc, lazy=lazy)
    s = Fields(b)
    nk, P = dims[dir_keep - 1], plane_points(dims, dir_keep)
    prof, sums, again = new_sums(b, nk), new_sums(b, nk), new_sums(b, nk)
    for it in range(1, n + 1):
        s.set(sample_arrays(dims, seed * 1000 + it))
        p = s.p if with_p else None
        b.budget_profile_sums(s.u, s.v, s.w, p, s.grads, dir_keep, P_SCALE, sums)
        b.budget_profile_sums(s.u, s.v, s.w, p, s.grads, dir_keep, P_SCALE, again)
        assert torch.equal(sums, again), "the budget reduction is not deterministic"
        b.budget_profile_accumulate(prof, sums, 1.0 / P, 1.0 / it)
    got = prof.view(41, nk).cpu().numpy()
    ref, vmax = reference(tuple(dims), dir_keep, n, seed)
    rows = [(name, float(np.max(np.abs(got[k].astype(np.longdouble) - ref[k]))), (n + 4 + P) * EPS * vmax[k])
            for k, name in enumerate(MOMENT_NAMES)]
    return rows, got, sums.view(41, nk).cpu().numpy()


def check_rows(rows):
    for r in rows:
        print("budgets check:", *r)
    bad = [r for r in rows if not r[-2] <= r[-1]]
    assert not bad, bad


def no_pressure_case(dims, ybc, dir_keep):
    """the sums with p = NULL next to the sums with p: returns (pressure moments all exactly 0, the other 30 bit-equal)"""
    _, _, with_p = parity_case(dims, ybc, dir_keep, n=1)
    _, _, without = parity_case(dims, ybc, dir_keep, n=1, with_p=False)
    pm = list(budgets_ref.PRESSURE_MOMENTS)
    rest = [m for m in range(41) if m not in pm]
    zero = not np.any(without[pm]) and not np.any(np.signbit(without[pm]))
    return bool(zero), without[rest].tobytes() == with_p[rest].tobytes() and bool(np.all(np.any(with_p[pm] != 0, axis=1)))


# ---------------------------------------------------------------- 1., 2. parity and determinism
@pytest.mark.parametrize("dims,ybc,dir_keep", SHAPES, ids=IDS)
def test_all_41_moments_against_longdouble_plane_means(dims, ybc, dir_keep):
    rows, _, _ = parity_case(dims, ybc, dir_keep)
    assert len(rows) == 41 and all(r[2] > 0.0 for r in rows)
    check_rows(rows)


def test_the_same_fields_give_the_same_bits_from_two_backends():
    """twice within a backend is part of every parity case; here two backends (two partial buffers) as well"""
    dims, ybc, dir_keep = SHAPES[6]
    _, _, a = parity_case(dims, ybc, dir_keep, n=1)
    _, _, c = parity_case(dims, ybc, dir_keep, n=1)
    assert a.tobytes() == c.tobytes() and np.all(np.any(a != 0, axis=1))


# ---------------------------------------------------------------- 3. p = NULL
@pytest.mark.parametrize("dims,ybc,dir_keep", SHAPES, ids=IDS)
def test_without_pressure_its_moments_are_zero_and_the_rest_keeps_its_bits(dims, ybc, dir_keep):
    zero, same = no_pressure_case(dims, ybc, dir_keep)
    assert zero, "moments 3, 10-13, 35-40 must be exactly 0 without p"
    assert same, "the other 30 moments must not depend on whether p is given"


# ---------------------------------------------------------------- 4. against the statistics' profile sums
@pytest.mark.parametrize("dims,ybc,dir_keep", [SHAPES[0], SHAPES[6], SHAPES[7]], ids=[IDS[0], IDS[6], IDS[7]])
def test_first_and_second_moments_agree_with_the_statistics_profiles(dims, ybc, dir_keep):
    import torch
    from x3d2_amd import _lib
    b = make_backend(dims, ybc)
    s = Fields(b)
    s.set(sample_arrays(dims, 5001))
    nk, P = dims[dir_keep - 1], plane_points(dims, dir_keep)
    sums = new_sums(b, nk)
    b.budget_profile_sums(s.u, s.v, s.w, s.p, s.grads, dir_keep, P_SCALE, sums)
    st = torch.zeros(9 * nk, dtype=_lib.torch_real(), device=b.device)
    b.stats_profile_sums(s.u, s.v, s.w, dir_keep, st)
    got = sums.view(41, nk).cpu().numpy() / P
    want = st.view(9, nk).cpu().numpy().astype(np.float64) / P
    _, vmax = reference(tuple(dims), dir_keep, 3)
    eps_real = float(np.finfo(np.dtype(_lib.NP_REAL)).eps)
    rows = []
    for k9, k41 in enumerate([0, 1, 2] + list(range(4, 10))):
        rows.append((k41, float(np.max(np.abs(got[k41] - want[k9]))), (1 + 4 + P) * (EPS + eps_real) * vmax[k41]))
    check_rows(rows)


# ---------------------------------------------------------------- 5. errors
def test_bad_calls_set_the_error_and_launch_nothing():
    import ctypes
    import torch
    from x3d2_amd import _lib
    from x3d2_amd.common import CELL, VERT, X3dError
    dims = (32, 20, 24)
    b = make_backend(dims, WALL)
    s = Fields(b)
    s.set(sample_arrays(dims, 1))
    SENT = -7.5
    sums = torch.full((41 * 24,), SENT, dtype=torch.float64, device=b.device)
    prof = torch.full((41 * 24,), SENT, dtype=torch.float64, device=b.device)
    VP = ctypes.c_void_p

    def fields(**over):
        v = dict(u=s.u.ptr, v=s.v.ptr, w=s.w.ptr, p=s.p.ptr, grads=[g.ptr for g in s.grads])
        v.update(over)
        return _lib.BudgetFields(v["u"], v["v"], v["w"], v["p"], (VP * 9)(*v["grads"]))

    def call(f, d=_lib.ints(*dims), keep=2, out=sums.data_ptr()):
        return b.lib.x3d_budget_profile_sums(b.h, None if f is None else ctypes.byref(f), d, keep, P_SCALE, out)

    def untouched():
        b.sync()
        return bool(torch.all(sums == SENT)) and bool(torch.all(prof == SENT))

    g8 = [g.ptr for g in s.grads]
    g8[7] = None
    for f, kw, msg in [(None, {}, b"null"), (fields(u=None), {}, b"null"), (fields(v=None), {}, b"null"),
                       (fields(w=None), {}, b"null"), (fields(grads=g8), {}, b"gradient block 7 is null"),
                       (fields(), dict(d=None), b"null"), (fields(), dict(out=None), b"null"),
                       (fields(), dict(keep=1), b"not built"), (fields(), dict(keep=0), b"dir_keep"),
                       (fields(), dict(keep=4), b"dir_keep"),
                       (fields(), dict(d=_lib.ints(64, 20, 24)), b"outside the block"),
                       (fields(), dict(d=_lib.ints(32, 0, 24)), b"outside the block")]:
        assert call(f, **kw) != 0 and msg in b.lib.x3d_last_error(), msg
    acc = b.lib.x3d_budget_profile_accumulate
    for args, msg in [((None, sums.data_ptr(), 41 * 24), b"null"), ((prof.data_ptr(), None, 41 * 24), b"null"),
                      ((prof.data_ptr(), prof.data_ptr(), 41 * 24), b"same buffer"),
                      ((prof.data_ptr(), sums.data_ptr(), 0), b"positive"),
                      ((prof.data_ptr(), sums.data_ptr(), -3), b"positive")]:
        assert acc(b.h, args[0], args[1], args[2], 1.0, 1.0) != 0 and msg in b.lib.x3d_last_error(), msg
    assert acc(None, prof.data_ptr(), sums.data_ptr(), 4, 1.0, 1.0) != 0
    assert untouched()
    # the Python layer: a non-VERT input, a bad direction, a buffer of the wrong kind
    s.v.set_data_loc(CELL)
    with pytest.raises(X3dError, match="VERT"):
        b.budget_profile_sums(s.u, s.v, s.w, s.p, s.grads, 2, 1.0, sums)
    s.v.set_data_loc(VERT)
    with pytest.raises(X3dError, match="not built"):
        b.budget_profile_sums(s.u, s.v, s.w, s.p, s.grads, 1, 1.0, sums)
    with pytest.raises(X3dError, match="nine"):
        b.budget_profile_sums(s.u, s.v, s.w, s.p, s.grads[:8], 2, 1.0, sums)
    with pytest.raises(X3dError, match="float64"):
        b.budget_profile_sums(s.u, s.v, s.w, s.p, s.grads, 2, 1.0, sums[:40])
    assert untouched()
    # and the good call still works afterwards
    assert call(fields()) == 0
    b.sync()
    assert not bool(torch.any(sums[:41 * 20] == SENT))


# ---------------------------------------------------------------- 6. deferred execution
def test_sums_behind_queued_blas1_calls_equal_the_eager_result():
    dims, ybc, dir_keep = SHAPES[0]
    out = {}
    for lazy in (False, True):
        b = make_backend(dims, ybc, lazy=lazy)
        s = Fields(b)
        s.set(sample_arrays(dims, 5001))
        sums = new_sums(b, dims[dir_keep - 1])
        b.vecadd(0.5, s.v, 1.0, s.u)   # recorded, not run, while the deferred layer is on
        b.vecmult(s.w, s.u)
        b.veccopy(s.grads[4], s.w)
        b.field_scale(s.p, 1.25)
        b.budget_profile_sums(s.u, s.v, s.w, s.p, s.grads, dir_keep, P_SCALE, sums)
        if lazy:
            assert b.lazy_stats()["recorded"] >= 4
        out[lazy] = sums.cpu().numpy()
    assert out[True].tobytes() == out[False].tobytes() and np.any(out[False] != 0)


# ---------------------------------------------------------------- 7. the driver
def _host_sample(s, pressure):
    """u, v, w, the nine gradients and the vertex pressure of the solver's current state, on the host"""
    from x3d2_amd.common import DIR_X, VERT
    b, al = s.backend, s.backend.allocator
    taken = s.velocity_gradients()
    vel = [b.get_field_data(f).astype(np.float64) for f in (s.u, s.v, s.w)]
    grads = [b.get_field_data(g).astype(np.float64) for g in taken]
    p = None
    if pressure:
        taken += [al.get_block(DIR_X, VERT), al.get_block(DIR_X, VERT)]
        p = b.get_field_data(s.pressure_vert(*taken[-2:])).astype(np.float64)
    for f in taken:
        al.release_block(f)
    return vel, p, grads


@pytest.mark.parametrize("kw", [dict(fused=True), dict(fused=False),
                                dict(fused=True, inlet_noise=(0.125, 0.25, 0.5), seed=1234)],
                         ids=["fused", "op-granular", "fused-noise"])
def test_channel_run_samples_the_fields_and_the_pressure_of_every_step(kw):
    """the fused and the op-granular driver on the plain channel (fields of y alone), and the fused one with wall noise
    (fields that vary in x and z)"""
    from x3d2_amd import make_channel
    from x3d2_amd.budgets import Budgets, BudgetsConfig, MOMENT_NAMES
    dims, n = (24, 33, 16), 3
    case = make_channel(dims, **kw)
    s = case.solver
    assert not s.keep_pressure
    case.budgets = Budgets(s, BudgetsConfig(initbud=1, ibudfreq=1, pressure=True))
    assert s.keep_pressure
    samples, vmax = [], np.zeros(41)
    for it in range(1, n + 1):
        case.run(n_iters=it)
        assert s.pressure_wanted and s.pressure is not None and case.budgets.sample_count == it
        vel, p, grads = _host_sample(s, True)
        samples.append(budgets_ref.moments41(vel[0], vel[1], vel[2], p, grads, 1, 1.0 / s.dt))
        vmax = np.maximum(vmax, [float(np.max(np.abs(t))) for t in
                                 budgets_ref.terms41(vel[0], vel[1], vel[2], p, grads, 1, 1.0 / s.dt)])
    ref = budgets_ref.running_means(samples)
    got = case.budgets.moments()
    P = dims[0] * dims[2]
    rows = [(name, float(np.max(np.abs(got[name].astype(np.longdouble) - ref[k]))), (n + 4 + P) * EPS * vmax[k])
            for k, name in enumerate(MOMENT_NAMES)]
    assert got["umean"].shape == (33,) and float(np.max(np.abs(got["dudymean"]))) > 0.0
    if "seed" in kw:
        assert all(float(np.max(np.abs(got[name]))) > 0.0 for name in MOMENT_NAMES)
    check_rows(rows)
    terms = case.budgets.budgets()
    assert np.all(np.isfinite(terms["residual_uu"])) and terms["residual_uu"].shape == (33,)
    assert np.all(np.isfinite(terms["p_rms"]))


def test_tgv_run_without_pressure_leaves_the_run_alone():
    from x3d2_amd import make_tgv
    from x3d2_amd.budgets import Budgets, BudgetsConfig, MOMENT_NAMES
    n = 3
    case = make_tgv(32, fused=True)
    s = case.solver
    case.budgets = Budgets(s, BudgetsConfig(initbud=1, ibudfreq=1, pressure=False, profile_dir=3))
    samples, vmax = [], np.zeros(41)
    for it in range(1, n + 1):
        case.run(n_iters=it)
        assert not s.keep_pressure and case.budgets.sample_count == it
        vel, _, grads = _host_sample(s, False)
        samples.append(budgets_ref.moments41(vel[0], vel[1], vel[2], None, grads, 2))
        vmax = np.maximum(vmax, [float(np.max(np.abs(t))) for t in budgets_ref.terms41(vel[0], vel[1], vel[2], None, grads, 2)])
    ref = budgets_ref.running_means(samples)
    got = case.budgets.moments()
    rows = [(name, float(np.max(np.abs(got[name].astype(np.longdouble) - ref[k]))), (n + 4 + 32 * 32) * EPS * vmax[k])
            for k, name in enumerate(MOMENT_NAMES)]
    check_rows(rows)
    for k in budgets_ref.PRESSURE_MOMENTS:
        assert not np.any(got[MOMENT_NAMES[k]])
    terms = case.budgets.budgets()
    assert np.all(np.isfinite(terms["residual_uu"])) and "pressure_strain_uu" not in terms and "p_rms" not in terms
    plain = make_tgv(32, fused=True)
    assert plain.budgets is None
    plain.run(n_iters=n)
    for f, g in zip((s.u, s.v, s.w), (plain.solver.u, plain.solver.v, plain.solver.w)):
        assert s.backend.get_field_data(f).tobytes() == plain.solver.backend.get_field_data(g).tobytes()


# ---------------------------------------------------------------- 8. restart
def test_restart_continues_the_means_bit_for_bit(tmp_path):
    from x3d2_amd import make_channel
    from x3d2_amd.budgets import Budgets, BudgetsConfig, MOMENT_NAMES, load_budgets
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    from x3d2_amd.common import X3dError
    prefix = str(tmp_path / "checkpoint")

    def make(cfg):
        case = make_channel((24, 33, 16), fused=True)
        if cfg is not None:
            case.budgets = Budgets(case.solver, cfg)
        return case

    cfg = BudgetsConfig(initbud=1, ibudfreq=1, ibudout=4, prefix=str(tmp_path / "budgets"), pressure=True)
    whole = make(cfg)
    whole.checkpoints = Checkpoints(whole.solver, CheckpointConfig(checkpoint_freq=2, checkpoint_prefix=prefix), whole)
    whole.run(n_iters=4)
    resumed = make(cfg)
    assert restore(resumed, prefix + "_000002.npz") == 2 and resumed.budgets.sample_count == 2
    resumed.run(n_iters=4)
    a, c = whole.budgets.moments(), resumed.budgets.moments()
    assert whole.budgets.sample_count == resumed.budgets.sample_count == 4
    for name in MOMENT_NAMES:
        assert a[name].tobytes() == c[name].tobytes(), name
        assert np.any(a[name] != 0), name
    # the file of step 4, written by both runs
    assert whole.budgets.files == resumed.budgets.files == [str(tmp_path / "budgets_000004.npz")]
    back = load_budgets(cfg.prefix, 4)
    assert back["sample_count"] == 4 and back["profile_dir"] == 2 and back["pressure"] is True
    assert back["coord"].shape == (33,) and back["moments"]["uvmean"].tobytes() == a["uvmean"].tobytes()
    assert back["budgets"]["production_uu"].tobytes() == whole.budgets.budgets()["production_uu"].tobytes()
    # refusals: a checkpoint without budgets, another direction, another pressure setting
    bare = make(None)
    bare.checkpoints = Checkpoints(bare.solver, CheckpointConfig(checkpoint_freq=1, checkpoint_prefix=prefix + "_bare"), bare)
    bare.run(n_iters=1)
    with pytest.raises(X3dError, match="holds none"):
        restore(make(cfg), prefix + "_bare_000001.npz")
    with pytest.raises(X3dError, match="profile_dir"):
        restore(make(BudgetsConfig(initbud=1, profile_dir=3)), prefix + "_000002.npz")
    with pytest.raises(X3dError, match="pressure"):
        restore(make(BudgetsConfig(initbud=1, pressure=False)), prefix + "_000002.npz")
    assert restore(make(None), prefix + "_000002.npz") == 2  # (a run that samples none ignores the stored profiles)


# ---------------------------------------------------------------- 9. FP32, 10. two ranks
def _run(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_parity_determinism_and_no_pressure_in_the_fp32_flavour():
    """the same cases on 4-byte reals (libx3d2_hip_sp.so), in a process of its own; the factors are widened first and every
    accumulator is FP64, so the bound is the same FP64 one"""
    out = _run(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "budgets_sp_worker.py")],
               env={"X3D_SINGLE_PREC": "1"})
    res = json.loads([l for l in out.splitlines() if l.startswith("BUDGETSRESULT ")][-1][14:])
    assert res["dtype"] == "float32" and len(res["cases"]) == len(SHAPES) + 1
    for case in res["cases"]:
        assert len(case["rows"]) == 41
        check_rows([tuple(r) for r in case["rows"]])
        assert case["zero"] and case["same"], case["id"]


@pytest.mark.parametrize("layout,port", [((1, 2, 1), 29547), ((1, 1, 2), 29548)])
def test_two_ranks_hold_the_global_profile_of_the_one_rank_reference(layout, port, tmp_path):
    """two processes share the GPU and exchange through gloo (tests/mp_budgets_worker.py), y slabs and z slabs, profiles
    along y: both ranks hold the same global profile, within the bound of the one-rank numpy reference"""
    from x3d2_amd.budgets import MOMENT_NAMES
    dims, n, dir_keep = (16, 34, 32), 3, 2
    out = str(tmp_path / "mp")
    env = dict(MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    _run(["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
          "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(HERE, "mp_budgets_worker.py"),
          ",".join(map(str, dims)), ",".join(map(str, layout)), str(n), out], env=env)
    parts = [np.load(out + ".%d.npz" % k)["prof"] for k in range(2)]
    assert parts[0].shape == (41, dims[1]) and parts[0].tobytes() == parts[1].tobytes()
    ref, vmax = reference(dims, dir_keep, n, 7)
    P = plane_points(dims, dir_keep)
    check_rows([(name, float(np.max(np.abs(parts[0][k].astype(np.longdouble) - ref[k]))), (n + 4 + P) * EPS * vmax[k])
                for k, name in enumerate(MOMENT_NAMES)])
