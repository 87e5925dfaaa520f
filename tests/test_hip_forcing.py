"""Band forcing on the device (csrc/forcing.hip, x3d2_amd/forcing.py, case.HITCase) against the numpy restatement
tests/forcing_ref.py (pinned on the host by tests/test_forcing_host.py).

Bounds:
  coefficients  U of the mode box against rfftn, 1e-12 relative to the largest: a coefficient is a sum of N <= 138240 FP64 terms
                of size <= 5 in a fixed order, whose rounding stays below N eps max|term| / max|U| ~ 1e-13 even if every
                rounding had the same sign (max|U| ~ 3 sqrt(N)).
  row           E_band, D, the coefficient and the power, 1e-12 relative.
  blocks        the derivative blocks after add() against before + f of the restatement, 1e-12 max|f|; in the FP32 flavour
                2 * 2^-24 max|d_after|: the arithmetic is FP64 there too (the restatement runs in FP64 on the same float32 inputs),
                one rounding at the store.
  power         the mean of f . u, formed by numpy from the library's own output, equals P to 1e-12.
  steps         1e-10 max(max|ref|, 1) per field, the step tolerance of tests/test_hip_scalars.py (FP32: 2e-5).
  two ranks     1e-11 max(max|ref|, 1) against the one-rank run, as tests/test_hip_scalars.py.
Every block is filled with 1e30 before its data are set: a kernel that reads the row padding fails by thirty orders of
magnitude, one that writes it is caught by the comparison of the whole block.  Inputs are default_rng normal, float32-
representable (exact in both flavours); E_band of unit white noise is near 1.5 x (modes of the band) / N: the restatement gives
0.025, 0.0077, 0.0074 and 0.00083 on the four shapes, far from the guard."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import forcing_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TWOPI = 2.0 * np.pi
SHAPES = {"20x12x18": ((20, 12, 18), (TWOPI, TWOPI, TWOPI)),    # pitch 32, rows with a tail
          "33x10x9": ((33, 10, 9), (TWOPI, np.pi, 4.0)),        # odd extents, M = (2, 1, 1)
          "64x16x16": ((64, 16, 16), (TWOPI, TWOPI, TWOPI)),    # the extra 16 of the pitch
          "16x96x90": ((16, 96, 90), (TWOPI, TWOPI, TWOPI)),    # 8640 lines: several workgroups per plane with a short last one
          "20x20x20": ((20, 20, 20), (TWOPI, TWOPI, TWOPI))}
DEFAULT = dict(scheme="power", power=0.1, coeff=0.0, k_lo=0.0, k_hi=2.5, solenoidal=True)


# ---------------------------------------------------------------- helpers (also used by the worker processes)
def single():
    from x3d2_amd import _lib
    return _lib.SINGLE


def step_tol():
    return 2e-5 if single() else 1e-10


def normal_fields(dims, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(n)]


def make_solver(name, **kw):
    from x3d2_amd import make_tgv
    dims, L = SHAPES[name]
    return make_tgv(dims, L=L, poisson="CG", **kw).solver


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


def rel(got, want):
    return abs(got - want) / abs(want)


# ---------------------------------------------------------------- 1. projection, coefficients and synthesis
def check_kernels(name, **cfg_kw):
    """one add() on poisoned blocks against the restatement; returns the worst figures"""
    from x3d2_amd.forcing import Forcing, ForcingConfig
    kw = dict(DEFAULT, **cfg_kw)
    dims, L = SHAPES[name]
    s = make_solver(name)
    b = s.backend
    arrays = normal_fields(dims, 6, 11)
    blocks = poisoned_blocks(b, arrays)
    d, vel = blocks[:3], blocks[3:]
    frc = Forcing(s, ForcingConfig(**kw))
    assert frc.M == R.mode_box(L, kw["k_hi"])
    before = [whole(f) for f in blocks]
    inside = inside_mask(b, dims, before[0])
    frc.add(d[0], d[1], d[2], vel[0], vel[1], vel[2])
    after = [whole(f) for f in blocks]
    state = [t.cpu().numpy().copy() for t in (frc.uhat, frc.fhat, frc._row)]
    ref = R.forcing(arrays[3:], L, **kw)
    fig = {"e_band": ref["e_band"]}
    # the coefficients
    uhat, fhat = frc.coefficients_host()
    for what, got, want in (("U", uhat, ref["U"]), ("F", fhat, ref["F"])):
        want = np.stack([R.box_of(x, dims, frc.M) for x in want])
        err = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
        fig[what] = err
        print("%s %s: %s off by %.3e (relative to the largest)" % (name, cfg_kw, what, err))
        assert err <= 1e-12, what
    # the row
    row = frc.row()
    for key in ("e_band", "d", "coeff", "power"):
        err = rel(row[key], ref[key])
        fig["row_" + key] = err
        print("%s %s: row %s %.17g against %.17g" % (name, cfg_kw, key, row[key], ref[key]))
        assert err <= 1e-12, key
    # the blocks: inputs and all padding keep their bits, the interior is before + f
    fmax = max(float(np.max(np.abs(f))) for f in ref["f"])
    for k in range(6):
        if k >= 3:
            assert same_bits(before[k], after[k]), "input %d changed" % k
        else:
            assert same_bits(before[k][~inside], after[k][~inside]), "padding of block %d changed" % k
            assert not same_bits(before[k], after[k])
    worst = 0.0
    for c in range(3):
        got = b.get_field_data(d[c]).astype(np.float64)
        want = arrays[c] + ref["f"][c]
        bound = 2.0 * 2.0 ** -24 * float(np.max(np.abs(want))) if single() else 1e-12 * fmax
        err = float(np.max(np.abs(got - want)))
        worst = max(worst, err / bound)
        print("%s %s: block %d off by %.3e (bound %.3e, max|f| %.3e)" % (name, cfg_kw, c, err, bound, fmax))
        assert err <= bound, c
    fig["blocks"] = worst
    if not single() and kw["scheme"] == "power":
        # the injected power from the library's own output, on zeroed derivative blocks (f is then the output itself)
        for f in d:
            f.fill(1e30)
            b.set_field_data(f, np.zeros_like(arrays[0]))
        frc.add(d[0], d[1], d[2], vel[0], vel[1], vel[2])
        fu = float(np.mean(sum(b.get_field_data(f).astype(np.float64) * u for f, u in zip(d, arrays[3:]))))
        fig["power"] = rel(fu, kw["power"])
        print("%s %s: <f.u> = %.17g" % (name, cfg_kw, fu))
        assert fig["power"] <= 1e-12
    # two calls on the same inputs give the same bits
    for f, a in zip(d, arrays[:3]):
        f.fill(1e30)
        b.set_field_data(f, a)
    frc.add(d[0], d[1], d[2], vel[0], vel[1], vel[2])
    assert all(same_bits(x, whole(f)) for x, f in zip(after, blocks))
    assert all(same_bits(x, t.cpu().numpy()) for x, t in zip(state, (frc.uhat, frc.fhat, frc._row)))
    for f in blocks:
        b.allocator.release_block(f)
    return fig


@pytest.mark.parametrize("name", ["20x12x18", "33x10x9", "64x16x16", "16x96x90"])
def test_projection_and_synthesis(name):
    fig = check_kernels(name)
    assert fig["e_band"] > 5e-4  # (far from the guard)


@pytest.mark.parametrize("scheme,solenoidal,k_lo,k_hi", [("power", False, 0.0, 2.5), ("linear", True, 0.0, 2.5),
                                                         ("linear", False, 1.2, 2.5), ("power", True, 0.0, 4.5),
                                                         ("linear", False, 2.0, 4.5)])
def test_schemes_and_the_wider_mode_box(scheme, solenoidal, k_lo, k_hi):
    check_kernels("20x20x20", scheme=scheme, solenoidal=solenoidal, k_lo=k_lo, k_hi=k_hi, coeff=0.3)


def test_guard_on_a_zero_velocity():
    from x3d2_amd.forcing import Forcing, ForcingConfig
    name = "20x12x18"
    dims, _ = SHAPES[name]
    s = make_solver(name)
    b = s.backend
    arrays = normal_fields(dims, 3, 5) + [np.zeros((dims[2], dims[1], dims[0]))] * 3
    blocks = poisoned_blocks(b, arrays)
    before = [whole(f) for f in blocks]
    for scheme in ("power", "linear"):
        frc = Forcing(s, ForcingConfig(scheme=scheme, power=0.1, coeff=0.3))
        frc._row.fill_(7.0)
        frc.add(*blocks)
        assert all(same_bits(x, whole(f)) for x, f in zip(before, blocks)), scheme
        assert frc.row() == {"e_band": 0.0, "d": 0.0, "coeff": 0.0, "power": 0.0}, scheme
        assert not frc.fhat.cpu().numpy().any()


# ---------------------------------------------------------------- 2. steps of the case
HIT_DIMS, HIT_L = (20, 12, 18), (TWOPI, TWOPI, TWOPI)
HIT_KW = dict(Re=400.0, dt=2e-3, k0=2.0, ke0=0.5, seed=4)
FORCING_KW = dict(scheme="power", power=0.1, k_lo=0.0, k_hi=2.5, solenoidal=True)


def make_case(time_intg="RK3", fused=True, forcing=True, dims=HIT_DIMS, **kw):
    from x3d2_amd import make_hit
    from x3d2_amd.forcing import ForcingConfig
    args = dict(HIT_KW, time_intg=time_intg, fused=fused, forcing=ForcingConfig(**FORCING_KW) if forcing else None)
    args.update(kw)
    return make_hit(dims, L=HIT_L, **args)


@functools.lru_cache(maxsize=None)
def hit_reference(time_intg, nsteps, dims=HIT_DIMS):
    """the restatement's fields, kinetic energy and forcing rows after every step (computed once, never changed)"""
    kw = dict(HIT_KW)
    r = R.HitRef(dims, HIT_L, time_intg=time_intg, forcing_kw=FORCING_KW, **kw)
    fields, ke = [r.fields()], [r.kinetic_energy()]
    for _ in range(nsteps):
        r.step()
        fields.append(r.fields())
        ke.append(r.kinetic_energy())
    return fields, ke, list(r.rows)


def fields_of(case):
    s = case.solver
    s.flush_grad()
    return [s.backend.get_field_data(f).astype(np.float64) for f in (s.u, s.v, s.w)]


def assert_step(got, ref, what, tol=None):
    tol = step_tol() if tol is None else tol
    worst = 0.0
    for x, y, nm in zip(got, ref, "uvw"):
        err = float(np.max(np.abs(x - y))) / max(float(np.max(np.abs(y))), 1.0)
        worst = max(worst, err)
        assert err < tol, "%s: %s off by %.3e" % (what, nm, err)
    return worst


def check_steps(time_intg, fused):
    ref, _, _ = hit_reference(time_intg, 2)
    case = make_case(time_intg, fused)
    assert case.solver.forcing is not None
    assert_step(fields_of(case), ref[0], "initial state")
    worst = 0.0
    for it in (1, 2):
        case.step(it)
        worst = max(worst, assert_step(fields_of(case), ref[it], "step %d (%s, fused=%s)" % (it, time_intg, fused)))
    return worst


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op"])
@pytest.mark.parametrize("time_intg", ["RK3", "AB3"])
def test_two_forced_steps_against_the_composed_restatement(time_intg, fused):
    worst = check_steps(time_intg, fused)
    print("two forced steps %s fused=%s: worst field error %.3e" % (time_intg, fused, worst))


def spied_steps(case, nsteps=2):
    s = case.solver
    calls = {"deferred": 0, "stored": 0}
    transeq = s.transeq

    def spy(deriv, curr, defer=False):
        calls["deferred" if defer else "stored"] += 1
        return transeq(deriv, curr, defer=True) if defer else transeq(deriv, curr)

    s.transeq = spy
    for it in range(1, nsteps + 1):
        case.step(it, more=(it < nsteps))
    s.flush_grad()
    return [s.backend.get_field_data(f) for f in (s.u, s.v, s.w)], calls


def test_without_forcing_the_case_is_the_tgv_drivers_path_bit_for_bit():
    from x3d2_amd import make_tgv
    plain = make_case(forcing=False)
    assert plain.solver.forcing is None
    start = [plain.solver.backend.get_field_data(f) for f in (plain.solver.u, plain.solver.v, plain.solver.w)]
    got, calls = spied_steps(plain)
    tgv = make_tgv(HIT_DIMS, L=HIT_L, Re=HIT_KW["Re"], dt=HIT_KW["dt"], fused=True)
    for f, a in zip((tgv.solver.u, tgv.solver.v, tgv.solver.w), start):
        tgv.solver.backend.set_field_data(f, a)
    want, calls_tgv = spied_steps(tgv)
    for x, y, nm in zip(got, want, "uvw"):
        assert same_bits(x, y), nm
    assert calls == calls_tgv == {"deferred": 6, "stored": 0}  # the deferred branch, as before
    forced, calls_f = spied_steps(make_case(forcing=True))
    assert calls_f == {"deferred": 0, "stored": 6}  # the explicit branch
    assert max(float(np.max(np.abs(x - y))) for x, y in zip(forced, got)) > 1e-6


def test_deferred_execution_equals_eager():
    """the same two forced steps with the deferred-execution layer on, against the call-by-call run: 1e-12 x scale, the bound
    tests/test_hip_lazy_programs.py holds a deferred sequence to"""
    out = {}
    for lazy in (False, True):
        case = make_case("RK3", fused=False, lazy=lazy)
        for it in (1, 2):
            case.step(it)
        out[lazy] = fields_of(case)
    for x, y, nm in zip(out[True], out[False], "uvw"):
        err = float(np.max(np.abs(x - y))) / max(float(np.max(np.abs(y))), 1.0)
        print("deferred against eager, %s: %.3e" % (nm, err))
        assert err <= 1e-12, nm
    ref, _, _ = hit_reference("RK3", 2)
    assert_step(out[True], ref[2], "deferred, step 2")


def test_ten_forced_steps_hold_the_power():
    dims = (32, 32, 32)
    _, ke_ref, rows_ref = hit_reference("RK3", 10, dims)
    case = make_case("RK3", True, dims=dims)
    mon = case.monitoring
    ke = [mon.kinetic_energy()]
    for it in range(1, 11):
        case.step(it)
        row = case.solver.forcing.row()
        assert rel(row["power"], 0.1) <= 1e-12, (it, row)
        ref = rows_ref[3 * it - 1]  # (the last sub-step's)
        assert rel(row["e_band"], ref["e_band"]) <= 1e-10 and rel(row["coeff"], ref["coeff"]) <= 1e-10, (it, row, ref)
        ke.append(mon.kinetic_energy())
    gap = float(np.max(np.abs(np.array(ke) - np.array(ke_ref))))
    print("kinetic energy of ten forced steps: %s, worst gap %.3e" % (["%.6f" % k for k in ke], gap))
    assert gap <= 1e-10


def test_exact_resume(tmp_path):
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, read_checkpoint, restore
    prefix = str(tmp_path / "checkpoint")
    cases = []
    for restart in (False, True):
        case = make_case("RK3", True)
        if restart:
            assert restore(case, prefix + "_000003.npz") == 3
        else:
            case.checkpoints = Checkpoints(case.solver, CheckpointConfig(checkpoint_freq=3, checkpoint_prefix=prefix), case)
        case.run(n_iters=5)
        cases.append(case)
    for x, y, nm in zip(fields_of(cases[0]), fields_of(cases[1]), "uvw"):
        assert same_bits(x, y), nm
    z = read_checkpoint(prefix + "_000003.npz")
    assert int(z["case_seed"]) == HIT_KW["seed"] and float(z["case_k0"]) == HIT_KW["k0"] and float(z["case_ke0"]) == HIT_KW["ke0"]
    assert not any("forcing" in k for k in z)  # the term has no state


# ---------------------------------------------------------------- 3. two ranks
MP_DIMS = (16, 16, 96)


def mp_run(dims, **kw):
    """what the worker's ranks and the one-rank run do: the projection of the initial field (this rank's block alone), then two
    forced steps"""
    import torch
    case = make_case("RK3", True, dims=dims, **kw)
    s = case.solver
    frc = s.forcing
    local = torch.zeros_like(frc.uhat)
    frc.project(s.u, s.v, s.w, uhat=local, reduce=False)
    out = {"uhat": local.cpu().numpy().copy()}
    for it in (1, 2):
        case.step(it)
    out.update(zip("uvw", fields_of(case)))
    return out


def test_two_z_slabs_equal_the_one_rank_run(tmp_path):
    """two processes share the GPU and exchange through gloo (tests/mp_forcing_worker.py).  96 planes: the note of
    tests/test_hip_scalars.py on the distributed solve along z applies"""
    out = str(tmp_path / "mp")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", "29561", os.path.join(HERE, "mp_forcing_worker.py"),
           ",".join(map(str, MP_DIMS)), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    parts = [dict(np.load(out + ".%d.npz" % k)) for k in range(2)]
    one = mp_run(MP_DIMS)
    for nm in "uvw":
        two = np.concatenate([parts[0][nm], parts[1][nm]], axis=0)
        err = float(np.max(np.abs(two - one[nm]))) / max(float(np.max(np.abs(one[nm]))), 1.0)
        print("two ranks against one, %s: %.3e" % (nm, err))
        assert err < 1e-11, nm
    summed = parts[0]["uhat"] + parts[1]["uhat"]
    err = float(np.max(np.abs(summed - one["uhat"]))) / float(np.max(np.abs(one["uhat"])))
    print("the two ranks' coefficients summed against one rank's: %.3e" % err)
    assert err <= 1e-12 and np.any(parts[0]["uhat"] != parts[1]["uhat"])


def test_a_cut_x_is_refused():
    from x3d2_amd.common import X3dError
    with pytest.raises(X3dError, match="never cut"):
        make_case(nproc_dir=(2, 1, 1))


# ---------------------------------------------------------------- 4. FP32
def test_fp32_flavour():
    """the kernel cases and the two forced steps on 4-byte fields (libx3d2_hip_sp.so), in a process of its own; the worker
    asserts with the FP32 bounds of the module docstring"""
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "forcing_sp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("FORCINGRESULT ")][-1]
    print(line)
    assert "float32" in line


# ---------------------------------------------------------------- 5. refusals
def test_every_refusal_raises_and_changes_nothing():
    from x3d2_amd.common import CELL, VERT, X3dError
    from x3d2_amd.forcing import Forcing, ForcingConfig
    name = "20x12x18"
    dims, _ = SHAPES[name]
    s = make_solver(name)
    b = s.backend
    arrays = normal_fields(dims, 6, 9)
    blocks = poisoned_blocks(b, arrays)
    d, vel = blocks[:3], blocks[3:]
    frc = Forcing(s, ForcingConfig())
    frc.add(*blocks)
    for f, a in zip(blocks, arrays):
        f.fill(1e30)
        b.set_field_data(f, a)
    before = [whole(f) for f in blocks]
    state = [t.cpu().numpy().copy() for t in (frc.uhat, frc.fhat, frc._row)]
    untouched = lambda: (all(same_bits(x, whole(f)) for x, f in zip(before, blocks))
                         and all(same_bits(x, t.cpu().numpy()) for x, t in zip(state, (frc.uhat, frc.fhat, frc._row))))
    lib, h = b.lib, b.h
    prm = lambda p: ctypes.byref(p)
    P = frc.prm
    part, cap = frc.part.data_ptr(), frc.part.numel()
    uh, fh, row = frc.uhat.data_ptr(), frc.fhat.data_ptr(), frc._row.data_ptr()

    def project(p=P, u=vel[0].ptr, v=vel[1].ptr, w=vel[2].ptr, part=part, cap=cap, uh=uh, h=h):
        return lib.x3d_forcing_project(h, prm(p) if p is not None else None, u, v, w, part, cap, uh)

    def coeffs(p=P, uh=uh, scheme=0, value=0.1, sol=1, d_min=1e-300, fh=fh, row=row):
        return lib.x3d_forcing_coeffs(h, prm(p) if p is not None else None, uh, scheme, value, sol, d_min, fh, row)

    def synth(p=P, a=d[0].ptr, bb=d[1].ptr, c=d[2].ptr, fh=fh, row=row):
        return lib.x3d_forcing_synth(h, prm(p) if p is not None else None, a, bb, c, fh, row)

    def changed(**kw):
        q = type(P).from_buffer_copy(P)  # (a copy of the structure: the tables stay the object's)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    I3 = lambda *v: (ctypes.c_int * 3)(*v)
    bad_params = [(changed(periodic=I3(1, 0, 1)), b"not periodic"), (changed(M=I3(9, 2, 2)), b"at most 8"),
                  (changed(M=I3(2, 6, 2)), b"Nyquist"), (changed(nband=0), b"empty"),
                  (changed(nlocal=I3(10, 12, 18)), b"never cut"), (changed(tw_y=None), b"null table"),
                  (changed(nlocal=I3(20, 12, 19)), b"rows")]
    for q, msg in bad_params:
        for call in (project, coeffs, synth):
            assert call(p=q) != 0 and msg in lib.x3d_last_error(), (msg, lib.x3d_last_error())
    assert project(p=None) != 0 and coeffs(p=None) != 0 and synth(p=None) != 0
    assert project(h=None) != 0
    assert project(u=None) != 0 and b"null" in lib.x3d_last_error()
    assert project(part=None) != 0 and project(uh=None) != 0
    assert project(v=vel[0].ptr) != 0 and b"same block" in lib.x3d_last_error()
    assert project(cap=cap - 1) != 0 and b"buffer holds" in lib.x3d_last_error()
    assert coeffs(uh=None) != 0 and coeffs(fh=None) != 0 and coeffs(row=None) != 0
    assert coeffs(fh=uh) != 0 and b"same array" in lib.x3d_last_error()
    assert coeffs(scheme=2) != 0 and b"unknown scheme" in lib.x3d_last_error()
    assert coeffs(value=float("nan")) != 0 and coeffs(d_min=-1.0) != 0 and coeffs(d_min=float("inf")) != 0
    assert synth(a=None) != 0 and synth(fh=None) != 0 and synth(row=None) != 0
    assert synth(bb=d[0].ptr) != 0 and b"same block" in lib.x3d_last_error()
    assert untouched()
    # the Python object: refusals leave the solver without a forcing and allocate nothing
    for kw in (dict(k_hi=9.5), dict(k_hi=6.0), dict(k_lo=1.1, k_hi=1.3)):
        with pytest.raises(X3dError):
            Forcing(s, ForcingConfig(**kw))
    d[0].set_data_loc(CELL)
    with pytest.raises(X3dError, match="VERT"):
        frc.add(*blocks)
    d[0].set_data_loc(VERT)
    assert untouched() and s.forcing is None
    from x3d2_amd import make_channel
    with pytest.raises(X3dError, match="not periodic"):
        Forcing(make_channel((24, 33, 16), poisson="CG").solver, ForcingConfig())
