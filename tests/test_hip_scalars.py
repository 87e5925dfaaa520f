"""Active scalars on the device (csrc/scalars.hip, x3d2_amd/scalars.py, case.RayleighBenardCase) against the numpy restatement
tests/scalars_ref.py (pinned on the host by tests/test_scalars_host.py).

Bounds, counted and not tuned to the kernels (eps = 2^-52; in the FP32 flavour 2^-23 |want| for the one rounding of the output
is added: every factor is widened to double before any product there too):
  coupling      (ns + 3) eps (|d| + sum |terms|) per point: ns products and ns additions of the buoyancy sum each round once
                relative to partial sums that sum |terms| bounds, the product with up_i, the addition to d (or the three-term
                scalar product G . u and its subtraction) three more.
  plane sums    (n_plane + 2) eps sum |terms| per entry: a sum of n_plane terms in double in ANY order is off by at most
                (n_plane - 1) eps sum |terms| to first order, the product that forms a term and the final rounding add two.
  min / max     exact.
  steps         the tolerance tests/test_hip_poisson_010.py applies to the channel's step against the oracle:
                max |got - ref| < 1e-10 max(max |ref|, 1) per field (FP32: 2e-5, README "FP32").
  two ranks     the tolerance of tests/test_hip_channel_multirank.py: 1e-11 max(max |ref|, 1) against the one-rank run.
Every block is filled with 1e30 before its data are set: a kernel that reads the row padding fails by thirty orders of
magnitude, one that writes it is caught by the comparison of the whole block."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import scalars_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2
EPS = 2.0 ** -52
BETA = 0.259065151
# (dims, x bc, y bc, stretched y)
MESHES = {"box": ((20, 12, 16), PER, PER, False),        # the 20 x 12 x 16 box: full 16-byte vectors, no tail
          "channel": ((24, 33, 16), PER, WALL, True),    # the channel mesh: 528 rows, Dirichlet y, stretched
          "tail": ((18, 9, 5), PER, PER, False),         # 18 = 4 * 4 + 2 (FP32) and 9 rows of an odd count: the scalar tail
          "cylinder": ((33, 16, 8), WALL, PER, False),   # the cylinder's mesh: x faces, an odd row length
          "corner": ((17, 9, 6), WALL, WALL, False)}     # walls in x and y: the shared edges


# ---------------------------------------------------------------- helpers (also used by the worker processes)
def single():
    from x3d2_amd import _lib
    return _lib.SINGLE


def out_eps():
    """the rounding of an output to the library's real kind"""
    return 2.0 ** -23 if single() else 0.0


def step_tol():
    return 2e-5 if single() else 1e-10


def make_backend(name, nproc_dir=(1, 1, 1), rank=0, comm=None):
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    dims, xbc, ybc, stretched = MESHES[name]
    st = ("uniform", "top-bottom" if stretched else "uniform", "uniform")
    mesh = Mesh(tuple(dims), nproc_dir, (4.0, 2.0, 2.0), xbc, ybc, PER, st, (1.0, BETA, 1.0), nrank=rank)
    return HipBackend(mesh, comm=comm)


def normal_fields(dims, n, seed):
    """n standard_normal float32-representable fields [nz, ny, nx]"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(n)]


def poisoned_blocks(b, arrays):
    from x3d2_amd.common import DIR_X, VERT
    out = []
    for a in arrays:
        f = b.allocator.get_block(DIR_X, VERT)
        f.fill(1e30)
        b.set_field_data(f, a)
        out.append(f)
    return out


def whole(f):
    import torch
    torch.cuda.synchronize()
    return f.data.cpu().numpy().copy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def inside_mask(b, dims, like):
    nxp, nyp, nzp = (int(v) for v in b.padded_dims)
    inside = np.zeros(like.shape, dtype=bool)
    inside[:nxp * nyp * nzp].reshape(nzp, nyp, nxp)[:dims[2], :dims[1], :dims[0]] = True
    return inside


def coefficients(ns, with_g):
    """ri (one passive species among three; nine: all active, more than one group), ref non-zero, G on every other species
    (nine: on all of them, two groups of imposed-gradient terms)"""
    ri = [0.7 - 0.45 * s for s in range(ns)]
    if ns == 3:
        ri[1] = 0.0
    ref = [0.25 + 0.5 * s for s in range(ns)]
    grad = None
    if with_g:
        grad = [(0.3 + 0.1 * s, -0.2, 0.05 * (s + 1)) if s % 2 == 0 or ns == 9 else (0.0, 0.0, 0.0) for s in range(ns)]
    return ri, ref, grad


UPS = [(1.5, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -2.0), (0.6, 0.8, 0.0)]


# ---------------------------------------------------------------- 1. the coupling kernel
def check_couple(name):
    """every (ns, up, G) on one mesh; returns the worst error / bound"""
    dims = MESHES[name][0]
    b = make_backend(name)
    worst = 0.0
    for ns in (1, 3, 9):
        arrays = normal_fields(dims, 6 + 2 * ns, 100 + ns)
        blocks = poisoned_blocks(b, arrays)
        d, vel, dphi, phi = blocks[0:3], blocks[3:6], blocks[6:6 + ns], blocks[6 + ns:]
        # (what the device holds: the float32-representable inputs are exact in both flavours)
        a_d, a_vel, a_dphi, a_phi = arrays[0:3], arrays[3:6], arrays[6:6 + ns], arrays[6 + ns:]
        inside = inside_mask(b, dims, whole(blocks[0]))
        for up in UPS:
            for with_g in (False, True):
                for f, a in zip(blocks, arrays):
                    f.fill(1e30)
                    b.set_field_data(f, a)
                before = [whole(f) for f in blocks]
                ri, ref, grad = coefficients(ns, with_g)
                b.scalars_couple(d, dphi, vel, phi, up, ri, ref, grad)
                after = [whole(f) for f in blocks]
                want_d, want_p, mag_d, mag_p = R.couple(a_d, a_dphi, a_vel, a_phi, up, ri, ref, grad)
                what = "%s ns=%d up=%s G=%s" % (name, ns, up, with_g)
                for k in range(len(blocks)):  # inputs and all padding keep their bits
                    if k in (3, 4, 5) or k >= 6 + ns:
                        assert same_bits(before[k], after[k]), "%s: input %d changed" % (what, k)
                    else:
                        assert same_bits(before[k][~inside], after[k][~inside]), "%s: padding of %d changed" % (what, k)
                for i in range(3):
                    if up[i] == 0.0:
                        assert same_bits(before[i], after[i]), "%s: d[%d] touched though up[%d] = 0" % (what, i, i)
                    got = b.get_field_data(d[i]).astype(np.longdouble)
                    bound = (ns + 3) * EPS * mag_d[i] + out_eps() * np.abs(want_d[i])
                    worst = max(worst, float(np.max(np.abs(got - want_d[i]) / bound)))
                    assert np.all(np.abs(got - want_d[i]) <= bound), "%s: d[%d]" % (what, i)
                    if up[i] != 0.0:
                        assert not same_bits(before[i], after[i])
                for s in range(ns):
                    if grad is None or not any(grad[s]):
                        assert same_bits(before[6 + s], after[6 + s]), "%s: dphi[%d] touched though G = 0" % (what, s)
                    got = b.get_field_data(dphi[s]).astype(np.longdouble)
                    bound = (ns + 3) * EPS * mag_p[s] + out_eps() * np.abs(want_p[s])
                    worst = max(worst, float(np.max(np.abs(got - want_p[s]) / bound)))
                    assert np.all(np.abs(got - want_p[s]) <= bound), "%s: dphi[%d]" % (what, s)
        for f in blocks:
            b.allocator.release_block(f)
    return worst


@pytest.mark.parametrize("name", ["box", "channel", "tail"])
def test_coupling_kernel(name):
    worst = check_couple(name)
    print("coupling kernel on %s: worst error / bound %.3f" % (name, worst))
    assert 0.0 < worst <= 1.0


# ---------------------------------------------------------------- 2. the face stamp
FACE_CASES = [("channel", [{"y": (1.0, 0.0)}, None, {"y": (-2.5, 0.75)}]),
              ("cylinder", [{"x": (3.0, None)}, {"x": (None, -1.0)}]),
              ("corner", [{"x": (1.0, 2.0), "y": (3.0, 4.0)}, {"y": (None, 5.0), "x": (6.0, None)}] + [{"y": (7.0, 8.0)}] * 8)]


@pytest.mark.parametrize("name,walls", FACE_CASES, ids=[c[0] for c in FACE_CASES])
def test_face_stamp(name, walls):
    from x3d2_amd.scalars import ScalarsConfig
    dims = MESHES[name][0]
    b = make_backend(name)
    ns = len(walls)
    arrays = normal_fields(dims, ns, 7)
    blocks = poisoned_blocks(b, arrays)
    before = [whole(f) for f in blocks]
    spec = [ScalarsConfig._wall_of(w) for w in walls]
    mask = [sum(1 << (2 * d + side) for d in range(3) for side in range(2) if w[d][side] is not None) for w in spec]
    value = [[0.0 if w[d][side] is None else w[d][side] for d in range(3) for side in range(2)] for w in spec]
    b.scalars_apply_bc(blocks, mask, value, 63)
    inside = inside_mask(b, dims, before[0])
    for s in range(ns):
        want = R.stamp(arrays[s].copy(), spec[s])
        got = b.get_field_data(blocks[s])
        assert np.array_equal(got, want.astype(got.dtype)), "species %d" % s  # faces exact, interior bits kept
        after = whole(blocks[s])
        assert same_bits(before[s][~inside], after[~inside]), "padding of species %d" % s
        if mask[s] == 0:
            assert same_bits(before[s], after)
    # a face this rank does not own is not stamped
    for f, a in zip(blocks, arrays):
        f.fill(1e30)
        b.set_field_data(f, a)
    own = 0b010101  # the low faces only
    b.scalars_apply_bc(blocks, mask, value, own)
    for s in range(ns):
        low = [(w[0], None) for w in spec[s]]
        want = R.stamp(arrays[s].copy(), low)
        got = b.get_field_data(blocks[s])
        assert np.array_equal(got, want.astype(got.dtype)), "species %d, low faces only" % s


# ---------------------------------------------------------------- 3. profile sums
def check_profile_sums(name, ns, dir_keep):
    import torch
    from x3d2_amd import _lib
    from x3d2_amd.common import VERT
    dims = MESHES[name][0]
    b = make_backend(name)
    arrays = normal_fields(dims, 3 + ns, 40 + ns)
    blocks = poisoned_blocks(b, arrays)
    before = [whole(f) for f in blocks]
    nk = dims[dir_keep - 1]
    z = lambda n: torch.full((n,), 7.0, dtype=_lib.torch_real(), device=b.device)
    sums, mm = z(ns * 5 * nk), z(2 * ns)
    b.scalars_profile_sums(blocks[0], blocks[1], blocks[2], blocks[3:], dir_keep, sums, mm)
    got = sums.cpu().numpy().astype(np.float64).reshape(ns, 5, nk)
    gmm = mm.cpu().numpy().astype(np.float64).reshape(ns, 2)
    sums2, mm2 = z(ns * 5 * nk), z(2 * ns)
    b.scalars_profile_sums(blocks[0], blocks[1], blocks[2], blocks[3:], dir_keep, sums2, mm2)
    assert same_bits(sums.cpu().numpy(), sums2.cpu().numpy()) and same_bits(mm.cpu().numpy(), mm2.cpu().numpy())
    assert all(same_bits(x, whole(f)) for x, f in zip(before, blocks))
    worst = 0.0
    for s in range(ns):
        want, mags, n_plane = R.plane_sums(arrays[0], arrays[1], arrays[2], arrays[3 + s], dir_keep)
        bound = (n_plane + 2) * EPS * mags + out_eps() * np.abs(want)
        worst = max(worst, float(np.max(np.abs(got[s] - want) / bound)))
        assert np.all(np.abs(got[s] - want) <= bound), (name, ns, dir_keep, s)
        assert gmm[s, 0] == arrays[3 + s].min() and gmm[s, 1] == arrays[3 + s].max()
    return worst


@pytest.mark.parametrize("name,ns,dir_keep", [("channel", 1, 2), ("channel", 3, 3), ("tail", 1, 3), ("tail", 9, 2), ("box", 2, 2)])
def test_profile_sums(name, ns, dir_keep):
    worst = check_profile_sums(name, ns, dir_keep)
    print("profile sums on %s ns=%d dir=%d: worst error / bound %.3f" % (name, ns, dir_keep, worst))
    assert 0.0 < worst <= 1.0


def test_running_mean_follows_the_recurrence():
    """three samples of different fields through Scalars.update: mean_k = mean_{k-1} + (sample_k - mean_{k-1}) / k on the
    plane means, within 4 roundings of the real kind per sample (the kernel may contract the update into one fma)"""
    from x3d2_amd import make_tgv
    from x3d2_amd.common import VERT
    from x3d2_amd.scalars import Scalars, ScalarsConfig
    dims = (20, 12, 16)
    case = make_tgv(dims, L=(2.0 * np.pi, np.pi, 3.0), poisson="CG", n_species=2)
    s = case.solver
    for f in s.species:
        f.set_data_loc(VERT)
        f.fill(0.0)
    sca = s.scalars = Scalars(s, ScalarsConfig(profile_dir=2, initstat=2, istatfreq=2))
    assert not sca.coupled and not sca.reads_state(1) and sca.reads_state(2) and not sca.reads_state(3)
    mean = np.zeros((2, 5, dims[1]))
    scale = 0.0
    for k, it in enumerate((2, 4, 6), 1):
        arrays = normal_fields(dims, 5, 300 + it)
        for f, a in zip([s.u, s.v, s.w] + list(s.species), arrays):
            s.backend.set_field_data(f, a)
        assert not sca.update(it - 1) and sca.update(it)
        for i in range(2):
            want, _, n_plane = R.plane_sums(arrays[0], arrays[1], arrays[2], arrays[3 + i], 2)
            mean[i] += (want / n_plane - mean[i]) / k
        scale = max(scale, float(np.max(np.abs(mean))))
    p = sca.profiles()
    assert p["count"] == 3
    real_eps = 2.0 ** -23 if single() else EPS
    for m, nm in enumerate(("phi", "phiphi", "uphi", "vphi", "wphi")):
        assert p[nm].shape == (2, dims[1])
        assert np.max(np.abs(p[nm] - mean[:, m])) <= 3 * (4 + dims[0] * dims[2] * EPS / real_eps) * real_eps * scale, nm


# ---------------------------------------------------------------- 4. steps of the Rayleigh-Benard case
RB_DIMS, RB_L = (24, 33, 16), (4.0, 1.0, 4.0)
RB_KW = dict(Ra=1e5, Pr=0.71, dt=2e-3, noise=1e-3, seed=20)


def make_rb(stretching="uniform", time_intg="RK3", fused=True, **kw):
    from x3d2_amd import make_rayleigh_benard
    args = dict(RB_KW, stretching=stretching, beta=BETA, time_intg=time_intg, fused=fused)
    args.update(kw)
    return make_rayleigh_benard(RB_DIMS, RB_L, **args)


@functools.lru_cache(maxsize=None)
def rb_reference(stretching, time_intg, nsteps, noise=RB_KW["noise"]):
    """the restatement's fields after every step and its monitor after every step (computed once, never changed)"""
    r = R.RayleighBenardRef(RB_DIMS, RB_L, stretching=stretching, beta=BETA, time_intg=time_intg,
                            **dict(RB_KW, noise=noise))
    fields, mon = [r.fields()], [r.monitor()]
    for _ in range(nsteps):
        r.step()
        fields.append(r.fields())
        mon.append(r.monitor())
    return fields, mon


def fields_of(case):
    s = case.solver
    s.flush_grad()
    return [s.backend.get_field_data(f).astype(np.float64) for f in [s.u, s.v, s.w] + list(s.species)]


def assert_step(got, ref, what):
    worst = 0.0
    for x, y, nm in zip(got, ref, ("u", "v", "w", "phi")):
        err = float(np.max(np.abs(x - y))) / max(float(np.max(np.abs(y))), 1.0)
        worst = max(worst, err)
        assert err < step_tol(), "%s: %s off by %.3e" % (what, nm, err)
    return worst


def check_steps(stretching, time_intg, fused):
    ref, _ = rb_reference(stretching, time_intg, 2)
    case = make_rb(stretching, time_intg, fused)
    assert case.scalars is case.solver.scalars and case.scalars.coupled
    assert_step(fields_of(case), ref[0], "initial state")
    worst = 0.0
    for it in (1, 2):
        case.step(it)
        got = fields_of(case)
        worst = max(worst, assert_step(got, ref[it], "step %d (%s, %s, fused=%s)" % (it, stretching, time_intg, fused)))
        assert np.all(got[3][:, 0, :] == 1.0) and np.all(got[3][:, -1, :] == 0.0)  # the wall rows of phi, exactly
        assert np.all(got[1][:, 0, :] == 0.0) and np.all(got[1][:, -1, :] == 0.0)
    return worst


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op"])
@pytest.mark.parametrize("time_intg", ["RK3", "AB3"])
@pytest.mark.parametrize("stretching", ["top-bottom", "uniform"])
def test_two_steps_against_the_composed_restatement(stretching, time_intg, fused):
    worst = check_steps(stretching, time_intg, fused)
    print("two steps %s %s fused=%s: worst field error %.3e" % (stretching, time_intg, fused, worst))


SERIES = ("nu_lo", "nu_hi", "nu_vol", "phi_min", "phi_max")


def test_monitor_series_of_ten_steps():
    """monitor() after each of ten fused RK3 steps against the restatement's: bound 8 x the project's FP64 parity figure
    1e-12 x the scale of the series (its largest absolute value; the Nusselt numbers are near 1, of a state near conduction)"""
    ref, mon = rb_reference("top-bottom", "RK3", 10)
    case = make_rb("top-bottom", "RK3", True)
    rows = [case.scalars.monitor()]
    for it in range(1, 11):
        case.step(it)
        rows.append(case.scalars.monitor())
    assert_step(fields_of(case), ref[10], "step 10")
    for key in SERIES:
        got = np.array([float(np.ravel(r[key])[0]) for r in rows])
        want = np.array([float(m[key]) for m in mon])
        scale = max(float(np.max(np.abs(want))), 1.0)
        gap = float(np.max(np.abs(got - want)))
        print("monitor series %-8s scale %.3e  worst gap %.3e  (bound %.1e)" % (key, scale, gap, 8e-12 * scale))
        assert gap <= 8e-12 * scale, key
    assert rows[0]["phi"].shape == (1, RB_DIMS[1]) and rows[0]["vphi"].shape == (1, RB_DIMS[1])


# ---------------------------------------------------------------- 5. the conduction state
def test_conduction_state():
    ref, _ = rb_reference("top-bottom", "RK3", 3, noise=0.0)
    case = make_rb("top-bottom", "RK3", True, noise=0.0)
    m = case.scalars.monitor()
    for key in ("nu_lo", "nu_hi", "nu_vol"):
        assert abs(float(m[key][0]) - 1.0) <= 1e-12, (key, m[key])
    assert m["phi_min"][0] == 0.0 and m["phi_max"][0] == 1.0
    for it in (1, 2, 3):
        case.step(it)
    got = fields_of(case)
    assert_step(got, ref[3], "conduction state, step 3")
    print("conduction state after 3 steps: max|u| %.3e (restatement %.3e)"
          % (max(float(np.max(np.abs(a))) for a in got[:3]), max(float(np.max(np.abs(a))) for a in ref[3][:3])))


# ---------------------------------------------------------------- 6. nothing changes when nothing is asked
def run_tgv(attach):
    from mp_gpu_worker import set_species
    from x3d2_amd import make_tgv
    from x3d2_amd.scalars import Scalars, ScalarsConfig
    case = make_tgv(32, fused=True, n_species=1, pr_species=[0.7])
    s = case.solver
    set_species(case)
    if attach:
        s.scalars = Scalars(s, ScalarsConfig(ri=[0.0]))
        assert not s.scalars.coupled
    calls = {"deferred": 0, "stored": 0}
    transeq = s.transeq

    def spy(deriv, curr, defer=False):
        calls["deferred" if defer else "stored"] += 1
        return transeq(deriv, curr, defer=True) if defer else transeq(deriv, curr)

    s.transeq = spy
    for it in (1, 2):
        case.step(it, more=(it == 1))
    s.flush_grad()
    fields = [s.backend.get_field_data(f) for f in [s.u, s.v, s.w] + list(s.species)]
    return fields, calls, s.n_epi3, getattr(s.time_integrator, "n_stage_in_transeq", 0)


def test_an_uncoupled_scalars_object_changes_no_bit():
    plain, calls0, epi0, stage0 = run_tgv(False)
    attached, calls1, epi1, stage1 = run_tgv(True)
    for x, y, nm in zip(plain, attached, ("u", "v", "w", "phi")):
        assert same_bits(x, y), nm
    assert calls0 == calls1 == {"deferred": 6, "stored": 0}  # the deferred branch, as before
    assert (epi0, stage0) == (epi1, stage1)


def test_a_coupled_scalars_object_gives_up_the_deferred_branch_and_acts():
    from mp_gpu_worker import set_species
    from x3d2_amd import make_tgv
    from x3d2_amd.scalars import Scalars, ScalarsConfig
    plain, _, _, _ = run_tgv(False)
    case = make_tgv(32, fused=True, n_species=1, pr_species=[0.7])
    s = case.solver
    set_species(case)
    s.scalars = Scalars(s, ScalarsConfig(ri=[0.5], up=(0, 0, 1)))
    for it in (1, 2):
        case.step(it, more=(it == 1))
    s.flush_grad()
    w = s.backend.get_field_data(s.w)
    assert float(np.max(np.abs(w - plain[2]))) > 1e-6  # the TGV's w starts at zero: buoyancy along z is what moves it


# ---------------------------------------------------------------- 7. exact resume
def run_resume_pair(tmp_path):
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    prefix = str(tmp_path / "checkpoint")
    cases = []
    for restart in (False, True):
        case = make_rb("top-bottom", "RK3", True, initstat=1, istatfreq=1)
        if restart:
            assert restore(case, prefix + "_000003.npz") == 3
        else:
            case.checkpoints = Checkpoints(case.solver, CheckpointConfig(checkpoint_freq=3, checkpoint_prefix=prefix), case)
        case.run(n_iters=6)
        cases.append(case)
    return cases, prefix


def test_exact_resume(tmp_path):
    from x3d2_amd.checkpoint import read_checkpoint, restore
    from x3d2_amd.common import X3dError
    (a, c), prefix = run_resume_pair(tmp_path)
    for x, y, nm in zip(fields_of(a), fields_of(c), ("u", "v", "w", "phi")):
        assert same_bits(x, y), nm
    pa, pc = a.scalars.profiles(), c.scalars.profiles()
    assert pa["count"] == pc["count"] == 6
    for k in ("phi", "phiphi", "uphi", "vphi", "wphi"):
        assert same_bits(pa[k], pc[k]) and np.any(pa[k] != 0.0), k
    assert int(read_checkpoint(prefix + "_000003.npz")["case_seed"]) == RB_KW["seed"]
    # a checkpoint without the scalar profiles is refused by a run that keeps them -- before any field is written
    z = read_checkpoint(prefix + "_000003.npz")
    bare = str(tmp_path / "bare.npz")
    np.savez(bare, **{k: v for k, v in z.items() if not k.startswith("scalars_")})
    d = make_rb("top-bottom", "RK3", True, initstat=1, istatfreq=1)
    before = fields_of(d)
    with pytest.raises(X3dError, match="scalar profiles"):
        restore(d, bare)
    assert all(same_bits(x, y) for x, y in zip(before, fields_of(d))) and d.solver.current_iter == 0


# ---------------------------------------------------------------- 8. two ranks
MP_DIMS = (24, 33, 96)


def test_two_z_slabs_equal_the_one_rank_run(tmp_path):
    """two processes share the GPU and exchange through gloo (tests/mp_scalars_worker.py): two Rayleigh-Benard steps and
    three profile samples on z slabs against the one-rank run, at test_hip_channel_multirank's 1e-11.  24 x 33 x 96, not
    24 x 33 x 16: that test's own note applies -- a rank needs 48 planes and more for the truncation of the distributed
    tridiagonal solve along z to fall below round-off; with 8 planes per rank one and two ranks differ by far more than any
    parity tolerance, whatever the scalars do."""
    out = str(tmp_path / "mp")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", "29547", os.path.join(HERE, "mp_scalars_worker.py"),
           ",".join(map(str, MP_DIMS)), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    parts = [dict(np.load(out + ".%d.npz" % k)) for k in range(2)]
    one = rb_two_steps_with_profiles(MP_DIMS)
    for nm in ("u", "v", "w", "phi"):
        two = np.concatenate([parts[0][nm], parts[1][nm]], axis=0)
        ref = one[nm]
        err = float(np.max(np.abs(two - ref))) / max(float(np.max(np.abs(ref))), 1.0)
        print("two ranks against one, %s: %.3e" % (nm, err))
        assert err < 1e-11, nm
    n_plane = MP_DIMS[0] * MP_DIMS[2]
    for nm in ("p_phi", "p_phiphi", "p_uphi", "p_vphi", "p_wphi"):
        assert np.array_equal(parts[0][nm], parts[1][nm])  # every rank holds the global answer
        # the profile bound on the mean of n_plane terms, with sum |terms| / n_plane <= max |term| taken from the one-rank means
        scale = max(float(np.max(np.abs(one[nm]))), float(np.max(np.abs(one["p_phiphi"]))))
        assert np.max(np.abs(parts[0][nm] - one[nm])) <= (n_plane + 2) * EPS * scale + 1e-11 * scale, nm
    for nm in ("phi_min", "phi_max"):
        assert np.array_equal(parts[0][nm], parts[1][nm])
        assert abs(float(parts[0][nm][0]) - float(one[nm][0])) <= 1e-11


def rb_two_steps_with_profiles(dims, **kw):
    """two steps, a profile sample after each and one monitor at the end: what the worker's ranks and the one-rank run do"""
    from x3d2_amd import make_rayleigh_benard
    case = make_rayleigh_benard(dims, RB_L, stretching="top-bottom", beta=BETA, fused=True, initstat=1, **dict(RB_KW, **kw))
    for it in (1, 2):
        case.step(it)
        case.scalars.update(it)
    out = dict(zip(("u", "v", "w", "phi"), fields_of(case)))
    for k, v in case.scalars.profiles().items():
        out["p_" + k] = np.asarray(v)
    m = case.scalars.monitor()
    out["phi_min"], out["phi_max"] = m["phi_min"], m["phi_max"]
    return out


# ---------------------------------------------------------------- 9. FP32
def test_fp32_flavour():
    """tests 1 and 4 (stretched) on 4-byte fields (libx3d2_hip_sp.so), in a process of its own; the worker asserts with the
    FP32 bounds of the module docstring"""
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "scalars_sp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("SCALARSRESULT ")][-1]
    print(line)
    assert "float32" in line


# ---------------------------------------------------------------- 10. refusals
def test_every_refusal_raises_and_changes_nothing():
    import ctypes
    import torch
    from x3d2_amd import _lib
    from x3d2_amd.common import VERT, X3dError
    VP = ctypes.c_void_p
    name = "channel"
    dims = MESHES[name][0]
    b = make_backend(name)
    arrays = normal_fields(dims, 10, 5)
    blocks = poisoned_blocks(b, arrays)
    d, vel, dphi, phi = blocks[0:3], blocks[3:6], blocks[6:8], blocks[8:10]
    before = [whole(f) for f in blocks]
    untouched = lambda: all(same_bits(x, whole(f)) for x, f in zip(before, blocks))
    nan, inf = float("nan"), float("inf")
    ok = dict(up=(0, 1, 0), ri=[1.0, 0.5], ref=[0.0, 0.0], grad=[(0.1, 0, 0), (0, 0, 0.2)])
    bad = [dict(ok, up=(0, nan, 0)), dict(ok, ri=[1.0, inf]), dict(ok, ref=[nan, 0.0]), dict(ok, grad=[(0.1, 0, 0), (0, inf, 0)])]
    for kw in bad:
        with pytest.raises(X3dError, match="not finite"):
            b.scalars_couple(d, dphi, vel, phi, **kw)
    with pytest.raises(X3dError, match="is input"):  # an output that is an input
        b.scalars_couple([d[0], phi[0], d[2]], dphi, vel, phi, **ok)
    with pytest.raises(X3dError, match="same block"):
        b.scalars_couple([d[0], d[0], d[2]], dphi, vel, phi, **ok)
    with pytest.raises(X3dError, match="is input"):
        b.scalars_couple(d, [vel[1], dphi[1]], vel, phi, **ok)
    with pytest.raises(X3dError):  # ns < 1
        b.scalars_couple(d, [], vel, [], (0, 1, 0), [], [])
    with pytest.raises(X3dError):  # entries per species
        b.scalars_couple(d, dphi, vel, phi, (0, 1, 0), [1.0], [0.0, 0.0])
    assert untouched()
    # at the C ABI: null, dims outside the block
    dbl = ctypes.c_double
    prm = _lib.ScalarsParams(2, (dbl * 3)(0, 1, 0), (dbl * 2)(1.0, 0.5), (dbl * 2)(0.0, 0.0), None)
    pp = lambda fs: (VP * len(fs))(*[f.ptr for f in fs])
    lib, ints = b.lib, _lib.ints
    assert lib.x3d_scalars_couple(b.h, pp(d), pp(dphi), pp(vel), pp(phi), ints(*dims), None) != 0
    assert lib.x3d_scalars_couple(None, pp(d), pp(dphi), pp(vel), pp(phi), ints(*dims), ctypes.byref(prm)) != 0
    nulls = (VP * 2)(phi[0].ptr, None)
    assert lib.x3d_scalars_couple(b.h, pp(d), pp(dphi), pp(vel), nulls, ints(*dims), ctypes.byref(prm)) != 0
    assert b"null" in lib.x3d_last_error()
    assert lib.x3d_scalars_couple(b.h, pp(d), pp(dphi), pp(vel), pp(phi), ints(4096, 33, 16), ctypes.byref(prm)) != 0
    assert b"outside the block" in lib.x3d_last_error()
    assert lib.x3d_scalars_couple(b.h, pp(d), pp(dphi), pp(vel), pp(phi), ints(24, 0, 16), ctypes.byref(prm)) != 0
    prm0 = _lib.ScalarsParams(0, (dbl * 3)(0, 1, 0), (dbl * 2)(1.0, 0.5), (dbl * 2)(0.0, 0.0), None)
    assert lib.x3d_scalars_couple(b.h, pp(d), pp(dphi), pp(vel), pp(phi), ints(*dims), ctypes.byref(prm0)) != 0
    assert b"ns must be at least 1" in lib.x3d_last_error()
    assert untouched()
    # the stamp
    vals = (dbl * 12)(*([1.0] * 12))
    with pytest.raises(X3dError, match="not finite"):
        b.scalars_apply_bc(phi, [4, 0], [[0, 0, nan, 0, 0, 0], [0] * 6], 63)
    with pytest.raises(X3dError, match="same block"):
        b.scalars_apply_bc([phi[0], phi[0]], [4, 8], [[0.0] * 6] * 2, 63)
    assert lib.x3d_scalars_apply_bc(b.h, pp(phi), 2, ints(*dims), ints(4, 64), vals, 63) != 0
    assert lib.x3d_scalars_apply_bc(b.h, pp(phi), 2, ints(24, 33, 17), ints(4, 8), vals, 63) != 0
    assert lib.x3d_scalars_apply_bc(b.h, pp(phi), 0, ints(*dims), ints(4, 8), vals, 63) != 0
    assert lib.x3d_scalars_apply_bc(b.h, pp(phi), 2, ints(*dims), ints(4, 8), vals, 64) != 0
    assert lib.x3d_scalars_apply_bc(b.h, pp(phi), 2, ints(*dims), None, vals, 63) != 0
    assert untouched()
    # the sums
    sums = torch.full((2 * 5 * 33,), 3.0, dtype=_lib.torch_real(), device=b.device)
    mm = torch.full((4,), 3.0, dtype=_lib.torch_real(), device=b.device)
    with pytest.raises(X3dError, match="dir_keep"):
        b.scalars_profile_sums(vel[0], vel[1], vel[2], phi, 1, sums, mm)
    with pytest.raises(X3dError):
        b.scalars_profile_sums(vel[0], vel[1], vel[2], phi, 2, sums[:10], mm)
    rc = lib.x3d_scalars_profile_sums(b.h, vel[0].ptr, vel[1].ptr, vel[2].ptr, pp(phi), 2, ints(*dims), 1, sums.data_ptr(), mm.data_ptr())
    assert rc != 0 and b"not built" in lib.x3d_last_error()
    rc = lib.x3d_scalars_profile_sums(b.h, vel[0].ptr, vel[1].ptr, vel[2].ptr, pp(phi), 2, ints(64, 33, 16), 2, sums.data_ptr(), mm.data_ptr())
    assert rc != 0 and b"outside the block" in lib.x3d_last_error()
    rc = lib.x3d_scalars_profile_sums(b.h, vel[0].ptr, None, vel[2].ptr, pp(phi), 2, ints(*dims), 2, sums.data_ptr(), mm.data_ptr())
    assert rc != 0
    assert untouched() and bool(torch.all(sums == 3.0)) and bool(torch.all(mm == 3.0))
    # the Python object: refusals of the configuration leave the solver's fields alone
    from x3d2_amd import make_channel
    from x3d2_amd.scalars import Scalars, ScalarsConfig
    case = make_channel((24, 33, 16), n_species=1)
    s = case.solver
    s.species[0].set_data_loc(VERT)
    s.species[0].fill(0.25)
    fields0 = fields_of(case)
    for cfg in (dict(ri=[1.0, 2.0]), dict(wall=[{"x": (1.0, 0.0)}]), dict(wall=[{"z": (1.0, None)}]),
                dict(init=[np.zeros((2, 2, 2))]), dict(init=[lambda x, y, z: np.inf * y])):
        with pytest.raises(X3dError):
            Scalars(s, ScalarsConfig(**cfg))
    assert s.scalars is None and all(same_bits(x, y) for x, y in zip(fields0, fields_of(case)))
