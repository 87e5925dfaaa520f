"""The persistent and capped-grid kernels at pencil and tile counts that leave a tail (fp32_ops_ref.COUNTS), in FP64 against
the oracle at test_hip_parity's TOL: the batteries of test_x_direction_scan_kernels_full_size_pencils and
test_yz_operators_on_512_row_pencils (tests/util.py) extended to the 31 results tests/ops_sp_worker.py takes.

What a launch does with a count, read from the launchers (W = workgroups wanted, cap = x3d_persistent_blocks: 256 minus the
CU reserve; a workgroup loops `for (t = blockIdx.x; t < W; t += gridDim.x)`; "a + b" = a full trips and a last trip of b):

  x.256x65x64    4160 pencils.  k_xscan_transeq2x3 (8 pencil PAIRS per workgroup): W = 2080 / 8 = 260: 1 + 4; reserve 127
                 (cap 129): 2 + 2.  The one-pencil operators (k_xscan_tds, W = 520, fixed caps 768 / 1024) and the lincomb
                 prologue take one trip.  k_reduce: 4160 rows on 2048 workgroups: 2 + 64.  BLAS-1: the 272 x 65 x 64 block
                 is 565760 16-byte pairs = 2210 workgroups of 256 lanes against 2048: 1 + 162.
  x.512x9x9      81 pencils, odd: x3d_xscan_transeq3 and the two-pencil k_xscan_transeq2 decline (np % 2); the one-pencil
                 k_xscan_transeq runs three times on W = 11, the last workgroup with 1 pencil of 8.
  x.1024x9x9     81 pencils: csrc/xwide.hip is one pencil per wave throughout and has no np % 2: x3d_xwide_transeq3 takes it
                 (the counter rises), W = 11, the last workgroup with 1 pencil.
  x.1024x46x45   2070 pencils: W = 259, the last workgroup with 6 pencils.  k_xwide_transeq3: 1 + 3 (reserve: 2 + 1);
                 k_xwide_tds: its table form has a fixed cap of 256 (1 + 3), its circulant form of 512 (one trip).
  y.128x256x66   ntx = 8, 528 tiles: k_ytile_transeq3 and k_ytile_tds_pair 2 + 16 (reserve: 4 + 12).  The plain operators
                 are k_tds_onchip2, one workgroup per 32 pencils without a loop.
  z.64x66x512    ntx = 4, 264 tiles along z: 1 + 8 (reserve: 2 + 6).
  y.48x512x87    nx % 32 != 0: ntx = 3, 261 tiles: 1 + 5 (reserve: 2 + 3); the plain operators take the generic route.
  y.64x257x65    csrc/ygen.hip.  k_ygen_pair (also the plain operators, mode 2): ntx = 4, 260 tiles: 1 + 4 (reserve: 2 + 2).
                 k_ygen_transeq3 in its 8-pencil form (Q = 5, nx % 32 == 0): ntx = 8, 520 tiles against 2 x 256: 1 + 8
                 (reserve: cap 2 x 129 = 258, less 258 % 16 -> 256: 2 + 8).
  y.32x257x9     the 8-pencil form: 36 tiles, blocks = 36 - 36 % 16 = 32: 1 + 4.  Workgroup b of a group of 16 starts at
                 tile 2 (b % 8) + b / 8, so the tiles 32 .. 35 go to the workgroups 0, 8, 1 and 9 -- two pairs (b, b + 8) take
                 a second trip together, the other 28 workgroups none; reserve: the same.  k_ygen_pair: 18 tiles, one trip.
  y.48x257x87    the 16-pencil form (nx % 32 = 16): ntx = 3, 261 tiles: 1 + 5 (reserve: 2 + 3), pairs the same.
  y.32x320x9     as y.32x257x9 on 5 rows per lane with all 64 lanes busy.

Every case runs twice in one process: without the reserve and with X3D_COMM_RESERVE_CUS=127 (read when HipBackend is made),
which splits every persistent launch into other trips.  A pencil's arithmetic does not depend on the workgroup that takes it:
all 31 results must keep their bits."""
import hashlib
import json
import os

import numpy as np
import pytest

import fp32_ops_ref as ops_ref
import util
from test_hip_parity import TOL

gpu = pytest.mark.gpu
RESERVE = 127
FALLBACKS = ("X3D_XDIR_GENERIC", "X3D_NO_XSCAN", "X3D_XSCAN_P1", "X3D_NO_TILE3", "X3D_NO_XWIDE")
# results whose bits may move under the reserve, with the cause in the code: {(tag, result name): cause}.  None is known
BIT_EXEMPT = {}


def _split(want, cap):
    """(full trips, workgroups of the short last trip) of `want` work items on min(want, cap) workgroups"""
    g = min(want, cap)
    return want // g, want % g


def test_the_counts_leave_a_tail():
    """the arithmetic of the module docstring, from the launchers' formulas: every COUNTS case has a persistent launch with
    more than one trip and a short last one (without the reserve, or -- FP32-sized z tiles -- with it), an odd count, or a
    last workgroup with fewer than 8 pencils"""
    C = {t: ops_ref.CASES[t][0] for t in ops_ref.COUNTS}
    caps = (256, 256 - RESERVE)

    def tail(want):
        return [_split(want, cap) for cap in caps]
    nx, ny, nz = C["x.256x65x64.periodic.uniform"]
    assert tail((ny * nz // 2 + 7) // 8) == [(1, 4), (2, 2)] and _split(ny * nz, 2048) == (2, 64)
    assert _split(-(-(272 * ny * nz // 2) // 256), 2048) == (1, 162)
    for t in ("x.512x9x9.periodic.uniform", "x.1024x9x9.periodic.uniform"):
        np_ = C[t][1] * C[t][2]
        assert np_ % 2 == 1 and (np_ + 7) // 8 == 11 and np_ - 8 * 10 == 1
    nx, ny, nz = C["x.1024x46x45.periodic.uniform"]
    assert tail((ny * nz + 7) // 8) == [(1, 3), (2, 1)] and ny * nz - 8 * 258 == 6
    nx, ny, nz = C["y.128x256x66.periodic.uniform"]
    assert tail(nx // 16 * nz) == [(2, 16), (4, 12)] and tail(nx // 32 * nz) == [(1, 8), (2, 6)]  # FP64; two pencils per wave
    nx, ny, nz = C["z.64x66x512.periodic.uniform"]
    assert tail(nx // 16 * ny) == [(1, 8), (2, 6)] and tail(nx // 32 * ny) == [(1, 0), (1, 3)]
    nx, ny, nz = C["y.48x512x87.periodic.uniform"]
    assert nx % 32 and tail(nx // 16 * nz) == [(1, 5), (2, 3)]
    nx, ny, nz = C["y.64x257x65.dirichlet.top-bottom"]
    assert tail(nx // 16 * nz) == [(1, 4), (2, 2)]

    def np8(ntiles, cap):  # x3d_ygen_transeq3, NP == 8
        blocks = min(ntiles, 2 * cap)
        blocks -= blocks % 16
        return ntiles // blocks, ntiles % blocks
    assert nx % 32 == 0 and [np8(nx // 8 * nz, c) for c in caps] == [(1, 8), (2, 8)]
    for t in ("y.32x257x9.dirichlet.top-bottom", "y.32x320x9.dirichlet.top-bottom"):
        nx, ny, nz = C[t]
        assert nx % 32 == 0 and ny <= 320 and [np8(nx // 8 * nz, c) for c in caps] == [(1, 4), (1, 4)]
    nx, ny, nz = C["y.48x257x87.dirichlet.top-bottom"]
    assert nx % 32 == 16 and tail(nx // 16 * nz) == [(1, 5), (2, 3)]


def _three_in_one(tag):
    """what the dispatch of transeq_x promises at this count: x3d_xscan_transeq3 declines an odd number of pencils,
    x3d_xwide_transeq3 (1024 points, one pencil per wave) does not look at it"""
    if any(os.environ.get(k) == "1" for k in FALLBACKS):
        return None
    return {"x.256x65x64.periodic.uniform": True, "x.512x9x9.periodic.uniform": False,
            "x.1024x9x9.periodic.uniform": True, "x.1024x46x45.periodic.uniform": True}[tag]


def _battery(tag):
    """-> ({result name: hash of its bits}, the largest relerr, the backend's reserve)"""
    dims, d, bc, stretching, beta, L, seed = ops_ref.CASES[tag]
    got, worst = {}, {}
    if d == 1:
        s = util.x_operator_battery(dims, L, seed, TOL, three_in_one=_three_in_one(tag), full=True, got=got, worst=worst)
    else:
        assert L == ops_ref._LYZ and beta in (1.0, 0.259065151)
        s = util.yz_operator_battery(dims, bc, stretching, TOL, d=d, seed=seed, full=True, got=got, worst=worst)
    assert len(got) == 31 and sorted(got) == sorted(_NAMES), sorted(got)
    return {k: hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest() for k, a in got.items()}, worst["relerr"], \
        s.backend.comm_reserve


_NAMES = (["tds." + op for op in util.OPNAMES] + ["acc." + op for op in util.OPNAMES]
          + [n for a, b in ops_ref.PAIRS for n in ("pair0.%s+%s" % (a, b), "pair1.%s.A" % a, "pair1.%s.B" % b)]
          + [k + c for k in ("transeq_dir.", "transeq_dir_acc.", "transeq.") for c in "uvw"])
_default = {}


def _record(tag, environment, worst):
    line = json.dumps({"precision": "fp64", "environment": environment, "case": tag, "results": 31,
                       "worst_relerr": float("%.4g" % worst), "tol": TOL})
    print("FP64OP " + line)
    if os.environ.get("X3D_FP32_OPS_PROFILE"):
        with open(os.environ["X3D_FP32_OPS_PROFILE"], "a") as fh:
            fh.write(line + "\n")


def _default_run(tag, monkeypatch):
    if tag not in _default:
        monkeypatch.delenv("X3D_COMM_RESERVE_CUS", raising=False)
        bits, worst, reserve = _battery(tag)
        assert reserve == 0
        _record(tag, "default", worst)
        _default[tag] = bits
    return _default[tag]


@gpu
@pytest.mark.parametrize("tag", ops_ref.COUNTS)
def test_operators_at_counts_that_leave_a_tail(tag, monkeypatch):
    """the 31 results of the case against the oracle at TOL, and what the dispatch promises: the three-in-one counter rises
    by one across transeq_x at 4160 pencils of 256 points, stays at 81 pencils of 512 (np % 2), rises at 81 and at 2070
    pencils of 1024 (x3d_xwide_transeq3 has no such condition); tds_lincomb gives the bits of lincomb + tds_apply"""
    _default_run(tag, monkeypatch)


@gpu
@pytest.mark.parametrize("tag", ops_ref.COUNTS)
def test_operators_with_cus_reserved_keep_their_bits(tag, monkeypatch):
    """the same battery with X3D_COMM_RESERVE_CUS=127: cap 129 (258 -> 256 workgroups for the 8-pencil ygen form), so every
    persistent launch of the case takes other trips (the module docstring has them).  Same TOL, same dispatch, and every one
    of the 31 results bit-identical to the run without the reserve"""
    ref = _default_run(tag, monkeypatch)
    monkeypatch.setenv("X3D_COMM_RESERVE_CUS", str(RESERVE))
    bits, worst, reserve = _battery(tag)
    assert reserve == RESERVE
    _record(tag, "reserve127", worst)
    moved = sorted(k for k in bits if bits[k] != ref[k] and (tag, k) not in BIT_EXEMPT)
    assert not moved, (tag, moved)


@gpu
def test_reserve_out_of_range_is_an_error():
    """0 .. 127 CUs may be reserved; 128 is refused with a message and leaves the reserve as it was"""
    from x3d2_amd import make_tgv
    b = make_tgv((16, 16, 16), poisson="CG").solver.backend
    assert b.lib.x3d_backend_set_comm_reserve(b.h, RESERVE) == 0
    for n in (128, -1):
        assert b.lib.x3d_backend_set_comm_reserve(b.h, n) != 0
        msg = b.lib.x3d_last_error().decode()
        assert "x3d_backend_set_comm_reserve" in msg and "127" in msg, msg
    assert b.lib.x3d_backend_set_comm_reserve(b.h, 0) == 0


@gpu
def test_blas1_and_reductions_past_their_grid_caps():
    """the block of x.256x65x64: 2210 workgroups' worth of 16-byte pairs on the 2048 of stream_grid -- the grid-stride loops
    of vecadd, vecmult, field_scale, field_shift and lincomb take a short second trip -- against numpy at the tolerances of
    test_blas1_reorder_faces; 4160 rows on k_reduce's 2048 workgroups (two full trips and 64 rows) against numpy's float64
    sums within 1e-12 x the sum of the terms' magnitudes, the maximum exactly"""
    from x3d2_amd.common import DIR_X, VERT
    tag = "x.256x65x64.periodic.uniform"
    dims, _, _, _, _, L, seed = ops_ref.CASES[tag]
    s = ops_ref.product_solver(tag)
    b, al = s.backend, s.backend.allocator
    rng = np.random.default_rng(seed)
    x, y, z = (rng.standard_normal(dims[::-1]) for _ in range(3))
    fx, fy, fz, fo = (al.get_block(DIR_X, VERT) for _ in range(4))
    for f, a in ((fx, x), (fy, y), (fz, z)):
        b.set_field_data(f, a)
    tol = dict(rtol=1e-15, atol=1e-15)
    # (each operation against numpy on the values the one before it left on the device)
    b.vecadd(0.3, fx, -1.7, fy)
    cur = b.get_field_data(fy)
    assert np.allclose(cur, 0.3 * x - 1.7 * y, **tol)
    b.vecmult(fy, fx)
    prev, cur = cur, b.get_field_data(fy)
    assert np.allclose(cur, prev * x, **tol)
    b.field_scale(fy, 2.0)
    prev, cur = cur, b.get_field_data(fy)
    assert np.array_equal(cur, 2.0 * prev)
    b.field_shift(fy, 0.5)
    prev, cur = cur, b.get_field_data(fy)
    assert np.allclose(cur, prev + 0.5, **tol)
    b.set_field_data(fy, y)
    b.lincomb(fo, fz, [0.3, -1.7, 0.01], [fx, fy, fz])
    assert np.allclose(b.get_field_data(fo), z + 0.3 * x - 1.7 * y + 0.01 * z, **tol)
    assert np.array_equal(b.get_field_data(fx), x) and np.array_equal(b.get_field_data(fz), z)
    # reductions
    assert abs(b.scalar_product(fx, fz) - np.sum(x * z)) <= 1e-12 * np.sum(np.abs(x * z))
    assert abs(b.field_volume_integral(fx) - np.sum(x)) <= 1e-12 * np.sum(np.abs(x))
    mx, mean = b.field_max_mean(fz)
    assert mx == np.max(np.abs(z))
    assert abs(mean - np.sum(np.abs(z)) / z.size) <= 1e-12 * np.sum(np.abs(z)) / z.size
