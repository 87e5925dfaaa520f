"""The FP32 flavour of the library -- libx3d2_hip_sp.so, every kernel, table, scalar and transform on 4-byte reals
(make SP=1 = -DX3D_SINGLE_PREC; the reference's -DSINGLE_PREC, /root/reference/src/common.f90:6-12, whose CUDA backend
plans single-precision cuFFT transforms then, src/backend/cuda/poisson_fft.f90:427-458) -- against the reference's FP64
vectors and the FP64 library.  Tolerances are FP32's: 1e-5 relative for operators on O(1) fields (second derivatives
amplify the inputs' rounding by 1 / dx^2: 2e-4 there), 1e-5 on the enstrophy trace.  Each case runs tests/sp_worker.py in a
process of its own (the real kind is chosen when x3d2_amd is imported).

The Poisson solvers, path by path, on broadband right-hand sides (tests/poisson_sp_worker.py): each path's error against the
FP64 reference is held to fp32_ref.BOUND = 8 x the FP32 yardstick of its case (tests/fp32_ref.py: the oracle's solve as a
correctly rounded FP32 pipeline; tests/test_fp32_ref_host.py caps it and shows that the bound can fail), L2 against L2 and max
norm against max norm.  The channel case and two-rank runs (tests/channel_sp_worker.py, test_hip_parity._run_ranks) at the
step tolerances of this file: fields 2e-5 max(|ref|, 1), enstrophy 1e-5, max |div u| at FP32 round-off / the smallest spacing.

The compact operators, kernel family by kernel family and switch by switch (tests/ops_sp_worker.py), likewise: each result's
error against the oracle in FP64 is held to fp32_ref.BOUND x the yardstick of its own check (tests/fp32_ops_ref.py: the dense
operators as a correctly rounded FP32 pipeline; tests/test_fp32_ops_ref_host.py caps it and shows that the bound rejects a
1e-5 defect which the 2e-5 / 5e-4 of the fixture tests above accept)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _worker(*args, timeout=900, script="sp_worker.py", env=None):
    r = subprocess.run([sys.executable, os.path.join(HERE, script)] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout, env=dict(os.environ, X3D_SINGLE_PREC="1", **(env or {})))
    print(r.stdout[-6000:])  # (the workers print every figure before anything is asserted on it)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("SPRESULT ")][-1][9:])


@pytest.mark.parametrize("fixture", ["p000_rk3", "c010_rk3", "n111_rk2"])
def test_single_precision_operators_against_reference_vectors(fixture):
    """all 24 tds_solve operators (8 per direction: every closure, n_rhs = n_tds + 1, stretched y), transeq, divergence,
    gradient, curl and the enstrophy reduction of the periodic / Dirichlet + stretched / Neumann fixtures"""
    res = _worker("operators", fixture)[fixture]
    loose = {k: v for k, v in res["all"].items() if "der2nd" in k or k.startswith("transeq")}
    tight = {k: v for k, v in res["all"].items() if k not in loose}
    assert max(tight.values()) < 2e-5, (max(tight, key=tight.get), max(tight.values()))
    assert max(loose.values()) < 5e-4, (max(loose, key=loose.get), max(loose.values()))


def test_single_precision_tgv_trace():
    """TGV 64^3, RK3, FFT Poisson solve, 20 steps, fused driver and the reference's call sequence through the deferred
    layer: the enstrophy of the FP64 trace fixture to 1e-5, the projected field's divergence at FP32 round-off"""
    res = _worker("trace")
    for driver in ("fused", "lazy"):
        assert max(res[driver]["enstrophy_rel"]) < 1e-5, (driver, res[driver])
        assert max(res[driver]["div_max"][1:]) < 5e-5, (driver, res[driver])


def test_single_precision_step_at_the_bench_size(tmp_path):
    """one fused step at 512^3 -- the size-specialised kernels of the bench (three-in-one scan and tile kernels, on-chip solves,
    the z-first Poisson solve with the transforms on the z pairs' tiles) on 4-byte reals -- against the FP64 library"""
    from x3d2_amd import make_tgv
    ref = make_tgv(512, fused=True)
    ref.step(1)
    s = ref.solver
    want = [s.backend.get_field_data(f) for f in (s.u, s.v, s.w)]
    ens = ref.postprocess(1, 1e-3)[1]
    del ref, s
    out = tmp_path / "sp512.npz"
    res = _worker("step512", out, timeout=1200)
    assert res["dtype"] == "float32" and res["n_zfirst"] == 3
    got = np.load(out)
    for w, k in zip(want, "uvw"):
        assert np.max(np.abs(got[k].astype(np.float64) - w)) < 2e-5 * max(np.max(np.abs(w)), 1.0), k
    assert abs(res["enstrophy"] - ens) < 1e-5 * ens
    assert res["div_max"] < 1e-3  # (max |div u| of an FP32 projection at dx = 2 pi / 512: round-off / dx)


def test_fp32_through_the_boundary_the_reference_built_with_single_prec_on_the_fp32_library(tmp_path):
    """round 6: the Fortran side of the boundary in single precision.  oracle/_ref/shim/sp/xcompact_hip = the reference's own
    solver.f90 / cases / monitoring compiled with -DSINGLE_PREC (src/common.f90:6-12: dp = kind(0.0e0), MPI_REAL) + this
    repo's shim compiled with the same flag (m_x3d2_hip_capi.f90: x3d_creal = c_float) + libx3d2_hip_sp.so.  TGV 64^3,
    RK3, FFT Poisson, 20 steps: the enstrophy series of the FP64 fixture to 1e-5 relative (the tolerance of the FP32
    flavour's own trace test), the projection's divergence at FP32 round-off.  (Either shim checks x3d_real_bytes() against
    the kind it was compiled for before its first call and stops on the other flavour of the library.)"""
    import os
    import subprocess
    from util import read_trace_fixture
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "shim", "sp", "xcompact_hip")
    if not os.path.exists(exe) or not os.path.exists(os.path.join(root, "x3d2_amd", "libx3d2_hip_sp.so")):
        pytest.skip("FP32 shim binary not built (needs the reference tree at build time)")
    r = subprocess.run([exe, os.path.join(root, "fortran", "tgv64.x3d")], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = np.loadtxt(tmp_path / "monitoring.csv", delimiter=",", comments="#")
    fx = read_trace_fixture()
    assert rows.shape[0] >= 3
    assert np.all(np.abs(rows[:3, 1] - fx[:, 1]) < 1e-5 * fx[:, 1]), (rows[:3, 1], fx[:, 1])
    assert rows[:, 2].max() < 1e-4  # max |div u| after the projection, FP32


# ---------------------------------------------------------------- Poisson paths on broadband right-hand sides
ULP32 = 2.0 ** -23
PATH_ENVS = {"default": {}, "split": {"X3D_Y010_FORM": "split"}, "staged": {"X3D_Y010_FORM": "staged"},
             "no_y010": {"X3D_NO_Y010": "1"}, "no_fft512": {"X3D_NO_FFT512": "1"}, "no_rwt": {"X3D_NO_RWT": "1"},
             "slab": {"X3D_FORCE_PENCIL_FFT": "slab"}, "pencil3": {"X3D_FORCE_PENCIL_FFT": "1", "X3D_PENCIL_PARTS": "3"}}
_CLEAR = ("X3D_Y010_FORM", "X3D_NO_Y010", "X3D_NO_FFT512", "X3D_NO_RWT", "X3D_FORCE_PENCIL_FFT", "X3D_PENCIL_PARTS",
          "X3D_NO_ZFIRST", "X3D_NO_ZFIRST010", "X3D_NO_R2C512", "X3D_SLAB_PARTS")


def _poisson_worker(*args, env=None, timeout=900):
    """tests/poisson_sp_worker.py with exactly the switches of `env` set"""
    base = {k: v for k, v in os.environ.items() if k not in _CLEAR}
    r = subprocess.run([sys.executable, os.path.join(HERE, "poisson_sp_worker.py")] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=timeout, env=dict(base, X3D_SINGLE_PREC="1", **(env or {})))
    print(r.stdout[-8000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("SPRESULT ")][-1][9:])


@pytest.fixture(scope="module")
def poisson_paths(tmp_path_factory):
    """every environment's worker, run once each when first asked for: name -> (results by case, saved solutions)"""
    d = tmp_path_factory.mktemp("sp_poisson")
    done = {}

    def get(name):
        if name not in done:
            path = d / (name + ".npz")
            done[name] = (_poisson_worker("paths", name, path, env=PATH_ENVS[name]), dict(np.load(path)))
        return done[name]

    return get


def _accept(res, what):
    """both errors within fp32_ref.BOUND x the yardstick of the same case, norm by norm; the yardstick itself capped"""
    import fp32_ref
    for tag, r in res.items():
        assert r["finite"], (what, tag)
        assert r["yard_max"] <= fp32_ref.CAP, (what, tag, r["yard_max"])
        assert r["ratio_l2"] <= fp32_ref.BOUND and r["ratio_max"] <= fp32_ref.BOUND, (what, tag, r["ratio_l2"], r["ratio_max"])


def test_fp32_poisson_paths_default_environment(poisson_paths):
    """000 general (rocFFT 3-D plans), 000 with the own strided 512-point passes and the fused z pass, 010 uniform and the
    three stretchings at 32 cells (3-D transforms + the post-processing kernels and pentadiagonal solves) and at 256 cells
    (the y-last form, csrc/y010.hip), 100 and 110: the solver class, the case and the kind of pentadiagonal system as the
    FP64 twins assert them; the paths that leave no such trace differ in bits from their switched-off forms
    (test_fp32_poisson_010_forms_at_256_cells, test_fp32_poisson_512_point_passes)"""
    import fp32_ref
    res, _ = poisson_paths("default")
    assert sorted(res) == sorted(t for t in fp32_ref.CASES if not t.startswith(("000.24x512", "000.512x512x8")))
    _accept(res, "default")
    for tag, r in res.items():
        case, _, _, stretching, _, _ = fp32_ref.CASES[tag]
        assert r["case"] == case and not r["zfirst_ok"], (tag, r)
        assert r["type"] == {"000": "HipPoissonFFT", "010": "HipPoissonFFT", "100": "HipPoissonFFT100", "110": "HipPoissonFFT110"}[case]
        assert r["stretched_y"] == (stretching != "uniform"), (tag, r)
        if r["stretched_y"]:
            assert r["stretched_y_sym"] == (stretching != "bottom"), (tag, r)


def test_fp32_poisson_010_forms_at_256_cells(poisson_paths):
    """the y-last form of the 010 solve in its default, "split" and "staged" forms (odd / even systems: top-bottom; the
    full system: bottom) and the 3-D-transform form (X3D_NO_Y010=1), each within the bound; that the y-last kernels ran
    in FP32 is shown as the FP64 twin shows it: every y-last solution differs in bits from the 3-D form's of the same
    right-hand side, and the staged form's from the split form's"""
    off, off_sol = poisson_paths("no_y010")
    _accept(off, "no_y010")
    assert len(off) == 3 and all(r["stretched_y"] for r in off.values())
    sols = {}
    for name in ("default", "split", "staged"):
        res, sols[name] = poisson_paths(name)
        res = {t: r for t, r in res.items() if t.startswith("010.32x257x16.")}
        assert len(res) == (3 if name == "default" else 2)
        _accept(res, name)
        for tag, r in res.items():
            assert r["type"] == "HipPoissonFFT" and r["stretched_y_sym"] == (not tag.endswith(".bottom"))
            assert np.max(np.abs(sols[name][tag] - off_sol[tag])) > 0.0, (name, tag)  # (identical bits: the switched-off form ran twice)
    # X3D_Y010_FORM was honoured: the staged form (which falls back to the split one where its kernel declines) gives other
    # bits than the split form
    for tag in ("010.32x257x16.top-bottom", "010.32x257x16.bottom"):
        assert np.max(np.abs(sols["staged"][tag] - sols["split"][tag])) > 0.0, tag


def test_fp32_poisson_512_point_passes(poisson_paths):
    """ny = nz = 512: the solver's own strided 512-point y pass and the fused z pass (forward, division, backward in one
    kernel, csrc/fft512.hip), against the rocFFT-only path (X3D_NO_FFT512=1) and the tile branch of the fused pass
    (X3D_NO_RWT=1): each within the bound, and -- these paths leave no counter -- the solutions of the own passes differ in
    bits from the rocFFT-only form's.  (The tile branch does the operations of the default branch in the same order on
    another layout of the tile, k_fft512<2>: no difference in bits is to be expected of it, and none is asserted either way;
    it is held to the bound, which a wrong layout would miss by orders of magnitude.  A known gap: nothing here shows that
    X3D_NO_RWT was honoured at all.)"""
    tag = "000.20x512x512"
    sols = {}
    for name in ("default", "no_fft512", "no_rwt"):
        res, sol = poisson_paths(name)
        _accept({tag: res[tag]}, name)
        assert res[tag]["type"] == "HipPoissonFFT" and res[tag]["case"] == "000"
        sols[name] = sol[tag]
    assert np.max(np.abs(sols["default"] - sols["no_fft512"])) > 0.0
    assert np.max(np.abs(sols["no_rwt"] - sols["no_fft512"])) > 0.0


def test_fp32_slab_poisson_solver(poisson_paths):
    """csrc/sfft.hip on one rank (X3D_FORCE_PENCIL_FFT=slab): nx = 512 (k_r2c512 as the x pass), nz = 512 (the fused z
    stage on the received array), and neither"""
    res, _ = poisson_paths("slab")
    assert sorted(res) == ["000.24x512x40", "000.24x512x512", "000.512x512x8"]
    _accept(res, "slab")
    assert all(r["type"] == "HipSlabPoissonFFT" for r in res.values()), res


def test_fp32_pencil_poisson_solver_in_three_groups(poisson_paths):
    """csrc/pfft.hip on one rank with the z planes in 3 groups (X3D_FORCE_PENCIL_FFT=1, X3D_PENCIL_PARTS=3)"""
    res, _ = poisson_paths("pencil3")
    assert list(res) == ["000.34x40x24"]
    _accept(res, "pencil3")
    assert res["000.34x40x24"]["type"] == "HipPencilPoissonFFT" and res["000.34x40x24"]["parts"] == 3


def _stored_yardstick(tag):
    import fp32_ref
    with open(os.path.join(HERE, "golden", "fp32_yardsticks_full_size.json")) as fh:
        y = json.load(fh)[tag]
    assert tuple(y["dims"]) == fp32_ref.FULL_SIZE[tag][1] and y["max"] <= fp32_ref.CAP
    return y["l2"], y["max"]


def _full_size(paths, ref, yard, what):
    """the saved FP32 solutions against the FP64 library's, at the bound; -> the ratios"""
    import fp32_ref
    out = {}
    for name, path in paths.items():
        got = np.load(path)
        assert got.dtype == np.float32 and np.all(np.isfinite(got))
        err = fp32_ref.errors(got, ref)
        out[name] = (err[0] / yard[0], err[1] / yard[1])
        # (the raw figures, in the form of poisson_sp_worker.py's lines: profiles/fp32_poisson_paths.jsonl)
        print("FP32PATH " + json.dumps({"environment": "yslab" if name == "yslab" else "default", "case": what, "path": name,
                                        "l2": err[0], "yard_l2": yard[0], "ratio_l2": out[name][0], "max": err[1],
                                        "yard_max": yard[1], "ratio_max": out[name][1], "reference": "FP64 library"}))
        del got
    for name, (r2, rm) in out.items():
        assert r2 <= fp32_ref.BOUND and rm <= fp32_ref.BOUND, (what, name, r2, rm)
    return out


def test_fp32_poisson_000_at_512_cubed(tmp_path):
    """the paths that engage only at 512^3: solve_zfirst (csrc/zfirst.hip), the x-first poisson_000 with k_r2c512 as its x
    pass, and -- in a second worker -- the y-slab solver (X3D_FORCE_PENCIL_FFT=yslab, csrc/sfftz.hip) on the same right-hand
    side.  Reference: the FP64 library's solve of the same float32 values (held to the oracle at this size by
    test_hip_parity.py); yardstick: the stored one of this shape"""
    import fp32_ref
    tag = "000.512x512x512"
    yard = _stored_yardstick(tag)
    s = fp32_ref.product_solver(tag)
    assert not __import__("x3d2_amd")._lib.SINGLE
    ref = fp32_ref.hip_poisson_solve(s, fp32_ref.rhs_of(tag).astype(np.float64))
    assert ref.dtype == np.float64
    del s
    paths = {k: tmp_path / (k + ".npy") for k in ("zfirst", "xfirst", "yslab")}
    ev = _poisson_worker("full512", paths["zfirst"], paths["xfirst"], timeout=1200)
    assert ev["type"] == "HipPoissonFFT" and ev["zfirst_ok"], ev
    ev = _poisson_worker("full512", paths["yslab"], env={"X3D_FORCE_PENCIL_FFT": "yslab"}, timeout=1200)
    assert ev["type"] == "HipSlabPoissonFFTZ", ev
    _full_size(paths, ref, yard, tag)
    z, x = np.load(paths["zfirst"]), np.load(paths["xfirst"])
    assert np.max(np.abs(z - x)) > 0.0  # (different routes)


def test_fp32_poisson_010_at_the_channel_bench_size(tmp_path):
    """1024 x 257 x 512, top-bottom: solve_interleaved (rocFFT x and z, the y pass of csrc/y010.hip on the half-x spectrum)
    and solve_interleaved_zfirst (own z transform, complex 1024-point x transform, the y pass on the half-z spectrum)
    against the FP64 library's solve_interleaved of the same float32 values; yardstick: the stored one of this shape"""
    import fp32_ref
    tag = "010.1024x257x512.top-bottom"
    yard = _stored_yardstick(tag)
    s = fp32_ref.product_solver(tag)
    ref = fp32_ref.hip_poisson_solve(s, fp32_ref.rhs_of(tag).astype(np.float64), "solve_interleaved")
    del s
    paths = {k: tmp_path / (k + ".npy") for k in ("xfirst", "zfirst")}
    ev = _poisson_worker("chan010", paths["xfirst"], paths["zfirst"], timeout=1200)
    assert ev["type"] == "HipPoissonFFT" and ev["zfirst_ok"] and ev["stretched_y_sym"], ev
    _full_size(paths, ref, yard, tag)
    z, x = np.load(paths["zfirst"]), np.load(paths["xfirst"])
    assert np.max(np.abs(z - x)) > 0.0  # (different routes)


# ---------------------------------------------------------------- the channel case and decomposed directions
def _div_bound(min_spacing, vmax=1.0):
    """max |div u| after an FP32 projection: round-off of the velocity over the smallest spacing -- 100 ulp, the multiple
    that the 512^3 test's 1e-3 at dx = 2 pi / 512 amounts to"""
    return 100.0 * ULP32 * max(vmax, 1.0) / min_spacing


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("stretching,beta", [("top-bottom", 0.259065151), ("uniform", 1.0)])
def test_fp32_channel_steps_vs_oracle(stretching, beta, fused):
    """make_channel in the FP32 library: two steps at 24 x 33 x 16 (define_BC, transeq, forcings, RK3, apply_BC, the
    pressure correction with the 010 Poisson solve), fused and op-granular, against the oracle.
    The bulk-velocity integral of define_BC is part of what this holds: its per-row partial sums are added in double in
    either flavour (csrc/backend.hip, run_reduce and k_finish_shift).  Added one after the other on 4-byte reals, the 528
    partials left u shifted wall to wall by 2.2e-6 (37 ulp of its maximum) and the uniform case's enstrophy off by
    1.06e-5; the oracle's step with only that sum restated in float32 shows the same figures (2.0e-6, 1.17e-5), with the
    partials added in double 2.9e-9 and 1.7e-8."""
    res = _worker("small", stretching, beta, int(fused), script="channel_sp_worker.py")
    assert max(res["err"].values()) < 2e-5, res
    assert res["enstrophy_rel"] < 1e-5, res
    assert res["div_max"] < _div_bound(res["min_spacing"], res["vmax"]), res


def test_fp32_channel_step_at_the_bench_pencil_lengths():
    """1024-point x pencils and 257 stretched wall-normal vertices in FP32: K3w (csrc/xwide.hip) with the rotation forcing
    fused, K3g (csrc/ygen.hip), the 010 solve, one fused step against the oracle's signatures (asserted in the worker:
    assert_signature at 2e-5 of max(absmax, 1)); the three-in-one launches and the fused rotation happened"""
    res = _worker("bench", script="channel_sp_worker.py")
    assert res["three_in_one"] >= 6 and res["n_rot_fused"] == 3 and res["n_interleaved"] == 0, res
    assert max(res["sample_err"].values()) < 2e-5 and res["enstrophy_rel"] < 1e-5, res
    assert res["div_max"] < _div_bound(res["min_spacing"]), res


def test_fp32_channel_step_with_wall_noise(tmp_path):
    """x3d_wall_noise draws the same 53-bit integers in both flavours and converts them to the library's real kind
    (csrc/backend.hip: (real_t)(mix64(..) >> 11) * 2^-53), so for one seed the FP32 wall planes are the FP64 ones rounded: the
    wall planes to 2 ulp of the amplitude, and one fused channel step with the noise on within the step tolerances of the FP64
    library's.
    Random wall values are not compatible with a divergence-free interior (their net flux through the walls is not zero), so
    the projection leaves max |div u| = 2.7e-3 in FP64 as well -- the oracle's step with these wall planes gives 2.73e-3, and
    2.75e-3 with its Poisson solve done as tests/fp32_ref.py's FP32 pipeline.  What FP32 may add to it is round-off: max |div u|
    is held to the FP64 library's of the same step within round-off over the smallest spacing."""
    import fp32_ref
    ref, want, walls = fp32_ref.noise_step()  # (the lines the worker runs in the FP32 library)
    assert want[0].dtype == np.float64
    _, ens, dmax, _ = ref.postprocess(1, 0.005)
    out = tmp_path / "noise.npz"
    res = _worker("noise", out, script="channel_sp_worker.py")
    got = np.load(out)
    for c, (w, amp) in enumerate(zip(walls, fp32_ref.NOISE["inlet_noise"])):
        assert np.abs(w).max() > 0.5 * amp
        assert np.max(np.abs(got["wall%d" % c].astype(np.float64) - w)) <= 2 * ULP32 * amp, c
    for w, k in zip(want, "uvw"):
        assert np.all(np.isfinite(got[k]))
        assert np.max(np.abs(got[k].astype(np.float64) - w)) < 2e-5 * max(np.max(np.abs(w)), 1.0), k
    assert abs(res["enstrophy"] - ens) < 1e-5 * ens
    print("fields %s enstrophy %.3e max |div u|: FP32 %.4e, FP64 %.4e" % (
        ["%.2e" % (np.max(np.abs(got[k].astype(np.float64) - w)) / max(np.max(np.abs(w)), 1.0)) for w, k in zip(want, "uvw")],
        abs(res["enstrophy"] - ens) / ens, res["div_max"], dmax))
    assert abs(res["div_max"] - dmax) < _div_bound(res["min_spacing"], max(np.max(np.abs(w)) for w in want)), (res, dmax)


@pytest.mark.parametrize("nproc_dir,fused,dims", [((1, 1, 2), False, (48, 96, 96)), ((1, 2, 1), True, (48, 96, 96)),
                                                  ((1, 1, 2), True, (32, 512, 512))])
def test_fp32_two_ranks_match_the_single_rank_fp64_run(nproc_dir, fused, dims, tmp_path, monkeypatch):
    """decomposed directions in FP32 (halo exchange, reduced systems, strip corrections, the slab / pencil Poisson solvers):
    two steps of the decomposed TGV on two ranks of the FP32 library against the single-rank FP64 run; 512 rows per rank:
    the single-pass HALO kernels took the decomposed direction"""
    from test_hip_parity import _run_ranks
    from x3d2_amd import _lib, make_tgv
    assert not _lib.SINGLE
    ref = make_tgv(dims, fused=fused)
    ref.solver.n_output = 2
    rrows = ref.run(n_iters=2)
    want = [ref.solver.backend.get_field_data(f) for f in (ref.solver.u, ref.solver.v, ref.solver.w)]
    del ref
    monkeypatch.setenv("X3D_SINGLE_PREC", "1")
    g, rows = _run_ranks(nproc_dir, dims, 2, fused, "FFT", tmp_path)
    for k in range(2):  # (the ranks ran the FP32 library: _run_ranks gathers into float64 arrays)
        assert np.load(str(tmp_path / ("mp.%d.npz" % k)))["u"].dtype == np.float32
    if dims[1] == 512:
        assert g["halo_launches"] > 0
    for name, w in zip("uvw", want):
        assert np.max(np.abs(g[name] - w)) < 2e-5 * max(np.max(np.abs(w)), 1.0), name
    assert abs(rows[-1][1] - rrows[-1][1]) < 1e-5 * abs(rrows[-1][1])
    assert rows[-1][2] < _div_bound(2 * np.pi / max(dims)), rows[-1]


# ---------------------------------------------------------------- the compact operators, kernel family by kernel family
OPS_ENVS = {"default": {}, "no_npw2": {"X3D_NO_NPW2": "1"}, "no_circ": {"X3D_NO_CIRC": "1"}, "no_xcirc": {"X3D_NO_XCIRC": "1"},
            "no_uniform": {"X3D_NO_UNIFORM": "1"}, "no_direct": {"X3D_NO_DIRECT": "1"}, "no_q5": {"X3D_NO_Q5": "1"},
            "reserve127": {"X3D_COMM_RESERVE_CUS": "127"}}
_OPS_CLEAR = ("X3D_NO_CIRC", "X3D_NO_XCIRC", "X3D_NO_NPW2", "X3D_NO_UNIFORM", "X3D_NO_Q5", "X3D_NO_DIRECT", "X3D_NO_HALO_CIRC",
              "X3D_NO_XSCAN", "X3D_XDIR_GENERIC", "X3D_XSCAN_P1", "X3D_NO_XWIDE", "X3D_NO_XWIDE_UPD", "X3D_NO_YTILE", "X3D_NO_ZTILE",
              "X3D_NO_YGEN", "X3D_NO_TILE3", "X3D_NO_TDS_PAIR", "X3D_NO_TDS_LINCOMB", "X3D_NO_ONCHIP2", "X3D_NO_VIA_X", "X3D_PAD_X",
              "X3D_COMM_RESERVE_CUS")


def _ops_worker(name, tags, timeout=900):
    """tests/ops_sp_worker.py over a group of cases with exactly the switches of OPS_ENVS[name] set"""
    base = {k: v for k, v in os.environ.items() if k not in _OPS_CLEAR}
    r = subprocess.run([sys.executable, os.path.join(HERE, "ops_sp_worker.py"), name, ",".join(tags)],
                       capture_output=True, text=True, timeout=timeout, env=dict(base, X3D_SINGLE_PREC="1", **OPS_ENVS[name]))
    print(r.stdout[-200000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("SPRESULT ")][-1][9:])


@pytest.fixture(scope="module")
def ops_runs():
    """(environment, cases) -> results by case; a case runs once per environment, in one worker per call"""
    done = {}

    def get(name, tags):
        todo = [t for t in tags if (name, t) not in done]
        if todo:
            for t, r in _ops_worker(name, todo).items():
                done[name, t] = r
        return {t: done[name, t] for t in tags}

    return get


def _accept_ops(res, what):
    """every result of every case: finite, its yardstick under the cap, both errors within BOUND x the yardstick; -> the
    number of results"""
    import fp32_ops_ref as ops_ref
    n, bad = 0, []
    for tag, r in res.items():
        assert len(r["ops"]) == 31, (what, tag, sorted(r["ops"]))
        for name, e in r["ops"].items():
            n += 1
            assert e["finite"], (what, tag, name)
            assert e["yard_max"] <= ops_ref.CAP, (what, tag, name, e["yard_max"])
            if not (e["ratio_l2"] <= ops_ref.BOUND and e["ratio_max"] <= ops_ref.BOUND):
                bad.append((tag, name, round(e["ratio_l2"], 2), round(e["ratio_max"], 2)))
    assert not bad, (what, bad)
    return n


def _bits_differ(a, b):
    """the names of the results whose bits differ between two runs of one case"""
    return sorted(k for k in a["ops"] if a["ops"][k]["bits"] != b["ops"][k]["bits"])


def _ops_groups():
    import fp32_ops_ref as ops_ref
    return {"x": ops_ref.X_PERIODIC + [ops_ref.X_NEUMANN], "yz_periodic": ops_ref.NPW2 + ops_ref.NPW1 + [ops_ref.NON_TILE],
            "walls": ops_ref.WALLS, "counts": ops_ref.COUNTS}


@pytest.mark.parametrize("group", ["x", "yz_periodic", "walls"])
def test_fp32_operators_default_environment(ops_runs, group):
    """every case of fp32_ops_ref.CASES, in three workers: x pencils of 128 .. 1024 points (LDS-tiled, generic and FAST scan
    kernels, the 1024-row kernels, a Neumann pencil); periodic y / z pencils of 256 and 512 rows (tile kernels with two
    pencils per wave and, at nx = 48, with one; the non-tile route at nx = 40); wall-normal pencils (K3g on 257, 320, 321,
    384 and 500 rows, stretched and not, 130 Neumann rows).  Per case 31 results -- eight operators plain and accumulating,
    both pairs in both modes, the direction's transeq plain and accumulating, Solver.transeq -- each within
    fp32_ref.BOUND x the yardstick of its own check in both norms (tests/fp32_ops_ref.py)"""
    import fp32_ops_ref as ops_ref
    tags = _ops_groups()[group]
    res = ops_runs("default", tags)
    assert sorted(t for g in _ops_groups().values() for t in g) == sorted(ops_ref.CASES)
    _accept_ops(res, "default")
    if group == "x":
        for tag, r in res.items():
            assert r["extra"]["lincomb_bits_equal"], tag
            if tag in ops_ref.X_PERIODIC and ops_ref.CASES[tag][0][0] in (256, 512, 1024):
                assert r["extra"]["three_in_one"] == 1, (tag, r["extra"])  # the three-components-in-one kernels took transeq_x


def test_fp32_operators_at_counts_that_leave_a_tail(ops_runs):
    """the eleven count-edge cases (fp32_ops_ref.COUNTS; tests/test_hip_work_counts.py has what each count does to the
    launches, FP32 where it differs: two pencils per wave halve the tiles of y.128x256x66 to 264 and of z.64x66x512 to 132),
    31 results each within BOUND x the yardstick in both norms.  transeq_x in one launch at 4160 pencils of 256 points and at
    81 and 2070 pencils of 1024; not at 81 pencils of 512 (x3d_xscan_transeq3 declines an odd count)"""
    import fp32_ops_ref as ops_ref
    res = ops_runs("default", _ops_groups()["counts"])
    assert len(res) == 11 and _accept_ops(res, "default") == 11 * 31
    for tag in ops_ref.COUNTS_X:
        assert res[tag]["extra"]["lincomb_bits_equal"], tag
        assert res[tag]["extra"]["three_in_one"] == (0 if tag == "x.512x9x9.periodic.uniform" else 1), (tag, res[tag]["extra"])


def test_fp32_operators_with_cus_reserved_keep_their_bits(ops_runs):
    """X3D_COMM_RESERVE_CUS=127 on the tile and wall-normal cases of COUNTS: 129 workgroups at most (256 for the 8-pencil ygen
    form), so every persistent launch takes other trips -- z.64x66x512's 132 tiles, one trip by default, now two.  Accepted
    at the same bound, and no result changes bits against the default run: a pencil's arithmetic does not depend on the
    workgroup that takes it"""
    import fp32_ops_ref as ops_ref
    tags = ops_ref.COUNTS_TILE + ops_ref.COUNTS_WALLS
    res = ops_runs("reserve127", tags)
    _accept_ops(res, "reserve127")
    ref = ops_runs("default", tags)
    moved = {}
    for tag in tags:
        differ = _bits_differ(res[tag], ref[tag])
        line = json.dumps({"environment": "reserve127", "case": tag, "bits_differ": len(differ), "of": len(res[tag]["ops"]),
                           "kinds": sorted({k.split(".")[0] for k in differ})})
        print("FP32OPBITS " + line)
        if os.environ.get("X3D_FP32_OPS_PROFILE"):
            with open(os.environ["X3D_FP32_OPS_PROFILE"], "a") as fh:
                fh.write(line + "\n")
        if differ:
            moved[tag] = differ
    assert not moved, moved


@pytest.mark.parametrize("name,group", [("no_npw2", "NPW2"), ("no_circ", "CIRC"), ("no_xcirc", "XCIRC"), ("no_uniform", "UNIFORM"),
                                        ("no_direct", "DIRECT"), ("no_q5", "Q5")])
def test_fp32_operators_in_their_other_forms(ops_runs, name, group):
    """the forms a switch selects, on the cases it bears on, at the bound of the default run: one pencil per wave where two
    are the default (X3D_NO_NPW2); the lane-table form of the periodic uniform pencils in place of the circulant one
    (X3D_NO_CIRC; X3D_NO_XCIRC: of the three-in-one x kernel only); the general tables on a uniform grid (X3D_NO_UNIFORM); the
    distributed form of the wall-normal pencils in place of the Thomas recurrences (X3D_NO_DIRECT); 6 rows per lane on 320-row
    pencils in place of 5 (X3D_NO_Q5).
    That a switch was honoured: X3D_NO_CIRC and X3D_NO_DIRECT select another algorithm, so in every case at least one result
    differs in bits from the default run's.  The other switches re-tile or re-table the same arithmetic and may give the same
    bits: which results differ is printed, nothing is asserted on it."""
    import fp32_ops_ref as ops_ref
    tags = getattr(ops_ref, group)
    res = ops_runs(name, tags)
    _accept_ops(res, name)
    ref = ops_runs("default", tags)
    for tag in tags:
        differ = _bits_differ(res[tag], ref[tag])
        kinds = sorted({k.split(".")[0] for k in differ})
        line = json.dumps({"environment": name, "case": tag, "bits_differ": len(differ), "of": len(res[tag]["ops"]), "kinds": kinds})
        print("FP32OPBITS " + line)
        if os.environ.get("X3D_FP32_OPS_PROFILE"):  # (next to the workers' raw lines)
            with open(os.environ["X3D_FP32_OPS_PROFILE"], "a") as fh:
                fh.write(line + "\n")
        if name in ("no_circ", "no_direct"):
            assert differ, (name, tag)  # (identical bits throughout: the default form ran twice)
        if tag.startswith("x.") and "three_in_one" in res[tag]["extra"] and ops_ref.CASES[tag][0][0] in (256, 512, 1024):
            assert res[tag]["extra"]["three_in_one"] == 1, (name, tag)  # (none of these switches removes that launch)
