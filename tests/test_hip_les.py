"""Explicit LES on the device (csrc/les.hip, x3d2_amd/les.py) against the longdouble restatement tests/les_ref.py (pinned on
the host by tests/test_les_host.py) and the dense operators of tests/util.py.

Pointwise bound (counted, not tuned to the kernel), with u = 2^-53, n = |g|_F, cd = c2 D2 and the inputs float32-representable:
    |nu_t - ref| <= K 2^-52 cd n          |tau_ij - ref| <= K 2^-52 cd n^2          K = les_ref.K_BOUND[model]
  Common: D2 = a_x a_y a_z rounds twice, cd once (3u); S_ij = (g_ij + g_ji) / 2 once; S:S is six non-negative terms, each a
  square (1u) of a rounded value (2u), five additions and the doubling of the off-diagonal part: 9u relative.
  Smagorinsky: sqrt halves the 9u and adds at most 2u, the product 1u: 3 + 4.5 + 2 + 1 = 10.5u of nu_t <= cd sqrt(2) n, that
    is 7.5 2^-52 cd n.  tau_ij = 2 nu_t S_ij with |S_ij| <= n doubles it and adds S_ij's and the product's roundings on
    2 nu_t n <= 2.9 cd n^2 (2u): K = 2 x 7.5 + 3 = 18.
  WALE: G_ij is a three-term scalar product, off by at most 3u n^2; the trace third by 3u n^2; Sd_ii = G_ii - tr by
    3 + 3 + 2 = 8u n^2 (the off-diagonal ones by 4u n^2).  dd = Sd:Sd is off by sum 2 |Sd_ij| 8u n^2 + 7u dd <= (48 + 7) u n^2
    sqrt(dd), as sum |Sd_ij| <= 3 sqrt(dd) and sqrt(dd) <= n^2.  F = dd^(3/2) / D, D = ss^(5/2) + dd^(5/4), has dF/d(dd) <=
    3/2 sqrt(dd) / D, so dd's error moves F by 82.5u n (n dd / D).  With ss = e n^2 and the rotation part oo = (1 - e) n^2:
    (ss - oo)^2 / 6 <= dd <= n^4 / 4 (Nicoud and Ducros' identity Sd:Sd = (ss^2 + oo^2) / 6 + 2/3 ss oo + 2 IV with
    -ss oo / 2 <= IV <= 0), hence n dd / D <= min(6^(1/4) / sqrt|1 - 2e|, e^(-5/2) / 4) <= 3.1: 256u n.  ss's 9u moves F by at
    most 5/2 x 9u relative, the roots, products and the division of F, D and cd F add 14u relative, on F <= dd^(1/4) <=
    n / sqrt(2): 26u n.  Together 282u = 141 2^-52 cd n; tau as above: K = 2 x 141 + 3 = 285, rounded up to 288.
  tests/test_les_host.py shows that leaving one gradient out moves nu_t by more than a million times this bound.
Scalars: a sum of P terms in double, in ANY order, is off by at most (P - 1) 2^-52 max|term| P to first order (as
tests/test_hip_budgets.py argues for its means), plus the pointwise bound of every term: that of nu_t for slot 0, and
4 x that x n^2 for 2 nu_t S:S (S:S <= n^2; the factor's own 9u relative is below K's share).  The maxima are exact to the
pointwise bound of the term (slot 3: ih_x^2 + ih_y^2 + ih_z^2 rounds three times and the product once: + 4 2^-52 of the value).
Every block is filled with 1e30 before its data are set: a kernel that reads the row padding fails by thirty orders of
magnitude, one that writes it is caught by the comparison of the whole block."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import les_ref
import util

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2
EPS = 2.0 ** -52
MODELS = [("smagorinsky", 0.17 ** 2), ("wale", 0.5 ** 2)]
# (dims, y boundary, stretched y): the smallest shapes at which each branch of the kernel can go wrong
SHAPES = [((35, 9, 6), PER, False),    # an odd tail shorter than a 16-byte vector; 54 rows: one item per workgroup
          ((520, 5, 4), PER, False),   # 520 > 512 points: the lane loop's second trip (FP64), a second chunk per row
          ((64, 6, 5), PER, False),    # full 16-byte vectors only, pitch = nx: no padding at all
          ((256, 5, 4), PER, False),   # padded pitch: 272 != nx, the +16 pad of rows of 256 points and more
          ((8, 33, 7), WALL, True),    # Dirichlet, stretched y: the tables of the mesh, three different ones per index
          ((16, 40, 16), PER, False)]  # 640 rows: more items than workgroups, the prefetched second item of a workgroup
IDS = ["%dx%dx%d" % s[0] for s in SHAPES]
# the block that holds tau_ij after x3d_les_stress, written out (include/x3d2_hip.h): 11 12 13 / 12 22 23 / 13 23 33
TAU_AT = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 0): 1, (1, 1): 4, (1, 2): 5, (2, 0): 2, (2, 1): 5, (2, 2): 8}
NUT_AT = 3
OUT_BLOCKS = (0, 1, 2, 3, 4, 5, 8)
DER1ST_RHO = (1.0 - np.sqrt(1.0 - 4.0 / 9.0)) * 1.5  # decay per row of compact6 der1st's solve (alpha = 1 / 3): 0.382


# ---------------------------------------------------------------- helpers (also used by the worker processes)
def make_backend(dims, ybc=PER, stretched=False, nproc_dir=(1, 1, 1), rank=0, comm=None):
    from x3d2_amd import Mesh
    from x3d2_amd.backend import HipBackend
    st = ("uniform", "top-bottom" if stretched else "uniform", "uniform")
    mesh = Mesh(tuple(dims), nproc_dir, (4.0, 2.0, 2.0), PER, ybc, PER, st, (1.0, 0.259065151, 1.0), nrank=rank)
    return HipBackend(mesh, comm=comm)


def synthetic_gradients(dims, seed):
    """nine standard_normal float32-representable fields [nz, ny, nx]; plane k = 0 is all zero, plane k = 1 pure shear
    (only g_12 is left)"""
    rng = np.random.default_rng(seed)
    g = [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(9)]
    for m in range(9):
        g[m][0] = 0.0
        if m != 1:
            g[m][1] = 0.0
    return g


def tables_of(b, stretched, seed):
    """(a, ih) host tables: the mesh's own where it is stretched, else random ones (every index its own value)"""
    from x3d2_amd.diagnostics import spacing_tables
    from x3d2_amd.les import width_tables
    if stretched:
        return width_tables(b.mesh), spacing_tables(b.mesh)
    from x3d2_amd.common import VERT
    rng = np.random.default_rng(seed)
    dims = b.mesh.get_dims(VERT)
    return [rng.uniform(0.5, 2.0, int(n)) for n in dims], [rng.uniform(0.5, 2.0, int(n)) for n in dims]


def poisoned_blocks(b, arrays):
    from x3d2_amd.common import DIR_X, VERT
    out = []
    for a in arrays:
        f = b.allocator.get_block(DIR_X, VERT)
        f.fill(1e30)
        b.set_field_data(f, a)
        out.append(f)
    return out


def device_tables(b, tabs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(b.device) for t in tabs]


def whole(f):
    import torch
    torch.cuda.synchronize()
    return f.data.cpu().numpy().copy()


def run_kernel(dims, ybc, stretched, model, c2, seed=11):
    """one x3d_les_stress on synthetic gradients -> dict of what the tests assert on (device results as float64)"""
    import torch
    b = make_backend(dims, ybc, stretched)
    g = synthetic_gradients(dims, seed)
    a, ih = tables_of(b, stretched, seed + 1)
    da, dih = device_tables(b, a), device_tables(b, ih)
    blocks = poisoned_blocks(b, g)
    before = [whole(f) for f in blocks]
    row = torch.zeros(4, dtype=torch.float64, device=b.device)
    b.les_stress(blocks, model, c2, da, dih, row.data_ptr())
    after = [whole(f) for f in blocks]
    got = [b.get_field_data(f).astype(np.float64) for f in blocks]
    first = row.cpu().numpy().copy()
    for f, x in zip(blocks, g):  # the same input again, in the same blocks: the same bits
        f.fill(1e30)
        b.set_field_data(f, x)
    b.les_stress(blocks, model, c2, da, dih, row.data_ptr())
    again = [whole(f) for f in blocks]
    second = row.cpu().numpy().copy()
    nxp, nyp, nzp = (int(v) for v in b.padded_dims)
    inside = np.zeros(before[0].shape, dtype=bool)
    inside[:nxp * nyp * nzp].reshape(nzp, nyp, nxp)[:dims[2], :dims[1], :dims[0]] = True
    return dict(g=g, a=a, ih=ih, got=got, row=first, row2=second, before=before, after=after, again=again, inside=inside,
                padded=(nxp, nyp, nzp))


@functools.lru_cache(maxsize=None)
def kernel_case(idx, model):
    dims, ybc, stretched = SHAPES[idx]
    return run_kernel(dims, ybc, stretched, model, dict(MODELS)[model])


def pointwise_rows(r, model, c2, extra=None):
    """[(name, worst |err| / bound, 1.0)] of nu_t and the six stresses; extra(ref) -> an additional allowance (FP32)"""
    nt, tau, _ = les_ref.stress(r["g"], r["a"], model, c2)
    bn, bt = les_ref.bounds(r["g"], r["a"], model, c2)
    rows = []
    for name, blk, ref, bound in [("nut", NUT_AT, nt, bn)] + [("tau%d%d" % (i + 1, j + 1), TAU_AT[i, j], tau[i][j], bt)
                                                             for i in range(3) for j in range(i, 3)]:
        ref = np.asarray(ref, dtype=np.longdouble)
        allow = bound + (extra(ref) if extra is not None else 0.0)
        err = np.asarray(np.abs(r["got"][blk] - ref), dtype=np.float64)
        ok = err <= allow
        ratio = float(np.max(np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), 0.0)))
        rows.append((name, ratio if bool(np.all(ok)) else float("inf"), 1.0))
    return rows


def check_rows(rows):
    for r in rows:
        print("les check:", *r)
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, bad


# ---------------------------------------------------------------- 1. the kernel against the restatement
@pytest.mark.parametrize("model,c2", MODELS)
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_stress_against_the_restatement(idx, model, c2):
    dims = SHAPES[idx][0]
    r = kernel_case(idx, model)
    if dims == (256, 5, 4):
        assert r["padded"][0] == 272  # the padded pitch this shape is here for
    check_rows(pointwise_rows(r, model, c2))
    for blk in OUT_BLOCKS:
        assert not np.any(np.isnan(r["got"][blk]))
        assert not np.any(r["got"][blk][0]), "all-zero gradients: nu_t = tau = 0 exactly"
    if model == "wale":
        for blk in OUT_BLOCKS:
            assert not np.any(r["got"][blk][1]), "pure shear: g g = 0, WALE's nu_t = 0 exactly"
    else:
        assert np.all(r["got"][NUT_AT][1] > 0.0)
    assert np.max(r["got"][NUT_AT][2:]) > 0.0
    for m in (6, 7):
        assert r["after"][m].tobytes() == r["before"][m].tobytes(), "grads[%d] is left as it is" % m
    for m in OUT_BLOCKS:
        out = ~r["inside"]
        assert r["after"][m][out].tobytes() == r["before"][m][out].tobytes(), "row padding of block %d was written" % m


# ---------------------------------------------------------------- 2. the four scalars
def scalar_rows(r, model, c2, extra_rel=0.0):
    want = les_ref.scalars(r["g"], r["a"], r["ih"], model, c2)
    nt, _, ss = les_ref.stress(r["g"], r["a"], model, c2)
    bn, _ = les_ref.bounds(r["g"], r["a"], model, c2)
    n2 = np.asarray(les_ref.frobenius(r["g"]) ** 2, dtype=np.float64)
    P = nt.size
    terms = [np.asarray(nt, dtype=np.float64), np.asarray(2 * nt * ss, dtype=np.float64)]
    point = [bn, 4.0 * bn * n2]
    hx, hy, hz = r["ih"]
    q = hx[None, None, :] ** 2 + hy[None, :, None] ** 2 + hz[:, None, None] ** 2
    rows = []
    for k in (0, 1):
        bound = P * (P - 1) * EPS * float(terms[k].max()) + float(point[k].sum()) + extra_rel * float(want[k])
        rows.append(("sum%d" % k, float(abs(r["row"][k] - want[k])), bound))
    rows.append(("max2", float(abs(r["row"][2] - want[2])), float(bn.max()) + extra_rel * float(want[2])))
    rows.append(("max3", float(abs(r["row"][3] - want[3])), float((bn * q).max()) + (4 * EPS + extra_rel) * float(want[3])))
    return rows


@pytest.mark.parametrize("model,c2", MODELS)
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_scalars_against_longdouble_sums_and_twice_the_same_bits(idx, model, c2):
    r = kernel_case(idx, model)
    assert r["row"][0] > 0.0 and r["row"][1] > 0.0 and r["row"][3] > 0.0
    check_rows(scalar_rows(r, model, c2))
    assert r["row"].tobytes() == r["row2"].tobytes()
    for m in range(9):
        assert r["after"][m].tobytes() == r["again"][m].tobytes()


# ---------------------------------------------------------------- 3. plumbing, bit-exact
def small_case(kind, fused=True, time_intg="RK3", dims=None):
    """a TGV-like periodic box or the stretched Dirichlet channel with a smooth-plus-noise velocity"""
    from x3d2_amd import make_channel, make_tgv
    if kind == "box":
        dims = dims or (24, 20, 16)
        case = make_tgv(dims, fused=fused, time_intg=time_intg, poisson="CG")
    elif kind == "wall":  # uniform Dirichlet y
        dims = dims or (24, 20, 16)
        case = make_channel(dims, stretching="uniform", beta=1.0, fused=fused, time_intg=time_intg, poisson="CG")
    else:
        dims = dims or (24, 33, 16)
        case = make_channel(dims, fused=fused, time_intg=time_intg, poisson="CG")
    return case, dims  # (poisson="CG": the term needs no Poisson solver, none is built)


def set_noisy(case, dims):
    s = case.solver
    fields = util.noisy_tgv(dims, (0, 0, 0), dims)
    for f, a in zip((s.u, s.v, s.w), fields):
        s.backend.set_field_data(f, a)
    return fields


def seeded_blocks(b, dims, seed):
    rng = np.random.default_rng(seed)
    arrays = [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(3)]
    return poisoned_blocks(b, arrays)


@pytest.mark.parametrize("kind", ["channel", "box"])
@pytest.mark.parametrize("model", ["smagorinsky", "wale"])
def test_add_is_the_kernel_and_nine_accumulated_derivatives_bit_for_bit(kind, model):
    from x3d2_amd.common import DIR_X, DIR_Y, DIR_Z
    from x3d2_amd.les import Les, LesConfig
    case, dims = small_case(kind)
    s = case.solver
    b = s.backend
    set_noisy(case, dims)
    les = Les(s, LesConfig(model=model))
    grads = s.velocity_gradients()
    les.stress(grads)
    tau = [b.get_field_data(g) for g in grads]  # (downloaded, and handed back in blocks of their own)
    for g in grads:
        b.allocator.release_block(g)
    hand = seeded_blocks(b, dims, 5)
    tb = poisoned_blocks(b, tau)
    for i in range(3):
        for j, (dirps, d) in enumerate(((s.xdirps, DIR_X), (s.ydirps, DIR_Y), (s.zdirps, DIR_Z))):
            b.tds_apply(hand[i], tb[TAU_AT[i, j]], dirps.der1st, d, accumulate=True)
    want = [b.get_field_data(f) for f in hand]
    mine = seeded_blocks(b, dims, 5)
    free0 = len(b.allocator.free)
    les.add(*mine)
    assert len(b.allocator.free) >= free0  # the nine blocks went back to the pool
    for f, w in zip(mine, want):
        got = b.get_field_data(f)
        assert got.tobytes() == w.tobytes() and np.all(np.isfinite(got))
    m = les.monitor()
    assert m["nut_max"] >= m["nut_mean"] > 0.0 and m["eps_sgs"] > 0.0 and m["diffusion_number"] > 0.0


# ---------------------------------------------------------------- 4. the whole term against dense operators
@pytest.mark.parametrize("kind", ["box", "wall"])
@pytest.mark.parametrize("model,c2", MODELS)
def test_term_against_the_dense_restatement(kind, model, c2):
    """40^3, not smaller: util.dense_operator is a reference of the library's periodic (and decomposed) solves only where
    rho^n is negligible (its docstring; tests/test_hip_wide_stencils.py asks for rho^n < 1e-16), and der1st's rho is 0.382:
    n >= 39.  At 24 x 20 x 16 the periodic box misses the dense solve by 1.3e-7, 1.1e-7, 3.8e-7 (measured; rho^16 = 2e-7),
    which is the truncation of the reference's algorithm and says nothing about the term."""
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.les import Les, LesConfig
    case, dims = small_case(kind, dims=(40, 40, 40))
    assert all(DER1ST_RHO ** n < 1e-16 for n in dims)
    s = case.solver
    b, m = s.backend, s.mesh
    u, v, w = set_noisy(case, dims)
    cfg = LesConfig(model=model)
    assert cfg.c2 == c2
    les = Les(s, cfg)
    d = [b.allocator.get_block(DIR_X, VERT) for _ in range(3)]
    for f in d:
        f.fill(0.0)
    n0 = b.sync_count()
    les.add(*d)
    assert b.sync_count() == n0  # no call waited for the host
    got = [b.get_field_data(f) for f in d]
    deltas = [float(x) for x in m.d]
    ops = les_ref.dense_der1st(dims, deltas, [tuple(m.BCs_global[k]) for k in range(3)])
    tables = [np.full(n, h ** (2.0 / 3.0)) for n, h in zip(dims, deltas)]
    sgs, nt, ss = les_ref.dense_term(u, v, w, ops, tables, model, c2)
    errs = [util.relerr(g, r) for g, r in zip(got, sgs)]
    print("les check: term", kind, model, errs)
    assert max(errs) < 1e-12
    mon = les.monitor()
    n = float(np.prod(dims))
    assert abs(mon["eps_sgs"] - float(np.sum(2.0 * nt * ss)) / n) <= 1e-12 * mon["eps_sgs"]
    assert abs(mon["nut_max"] - float(nt.max())) <= 1e-12 * mon["nut_max"]
    if kind == "box":  # the energy identity of the conservative form, on the device term
        work = float(np.sum(u * got[0] + v * got[1] + w * got[2])) / n
        print("les check: energy identity", work, mon["eps_sgs"])
        assert abs(work + mon["eps_sgs"]) <= 1e-12 * mon["eps_sgs"]
        scale = sum(float(np.sum(np.abs(f))) for f in got)
        assert all(abs(float(np.sum(f))) <= 1e-12 * scale for f in got)


# ---------------------------------------------------------------- 5. steps
def perturbation(m):
    """tests/channel_sp_worker.py's smooth perturbation: all three components active"""
    X = 2 * np.pi * m.vert_coords[0][None, None, :] / m.L[0]
    Y = np.pi * m.vert_coords[1][None, :, None] / m.L[1]
    Z = 2 * np.pi * m.vert_coords[2][:, None, None] / m.L[2]
    return (0.05 * np.sin(X) * np.sin(Y) ** 2 * np.cos(Z), 0.04 * np.cos(X) * np.sin(Y) ** 2 * np.sin(Z),
            0.03 * np.sin(2 * X) * np.sin(Y) ** 2 * np.cos(Z))


def kinetic_energy(mesh, fields):
    """the volume mean of 1/2 |u|^2 from host fields [nz, ny, nx]: every vertex weighs h_x[i] h_y[j] h_z[k], the local
    spacings (1 / diagnostics.spacing_tables, the weights of the body loads).  On a uniform mesh this is
    Monitoring.kinetic_energy; on the channel's y, clustered at the walls, that unweighted vertex mean is NOT the kinetic
    energy: it counts the wall layers several times over."""
    from x3d2_amd.diagnostics import spacing_tables
    hx, hy, hz = (1.0 / np.asarray(t, dtype=np.float64) for t in spacing_tables(mesh))
    wgt = hx[None, None, :] * hy[None, :, None] * hz[:, None, None]
    return float(np.sum(wgt * 0.5 * sum(f * f for f in fields)) / np.sum(wgt))


def stepped(kind, time_intg, fused, cfg, nsteps=2):
    """(fields, kinetic energy, max |div u|, case) after nsteps steps; cfg = None: no model attached"""
    from x3d2_amd import make_channel, make_tgv
    from x3d2_amd.les import Les
    if kind == "tgv":
        case = make_tgv(32, fused=fused, time_intg=time_intg)
    else:
        case = make_channel((24, 33, 16), fused=fused, time_intg=time_intg)
        s = case.solver
        for f, p in zip((s.u, s.v, s.w), perturbation(s.mesh)):
            s.backend.set_field_data(f, s.backend.get_field_data(f) + p)
    s = case.solver
    assert s.les is None
    if cfg is not None:
        s.les = Les(s, cfg)
    for it in range(1, nsteps + 1):
        case.step(it)
    fields = [s.backend.get_field_data(f).astype(np.float64) for f in (s.u, s.v, s.w)]
    row = case.monitoring.write_step(nsteps * s.dt, s.u, s.v, s.w)
    print("les check: unweighted vertex mean of the energy", kind, time_intg, case.monitoring.kinetic_energy())
    return fields, kinetic_energy(s.mesh, fields), float(row[2]), case


def field_err(a, b):
    return max(util.relerr(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind,time_intg,model", [("tgv", "RK3", "smagorinsky"), ("tgv", "AB3", "wale"),
                                                   ("channel", "RK3", "wale"), ("channel", "AB3", "smagorinsky")])
def test_steps_with_the_model_attached(kind, time_intg, model):
    """The kinetic energy is the VOLUME mean (kinetic_energy above).  An earlier form of this test took
    Monitoring.kinetic_energy, the unweighted vertex mean, and found the WALE channel higher with the model by 3.2e-9
    (0.26491056410 against 0.26491056091; the three other cases lower).  That mean is not the energy on the channel's
    stretched y: its mean of u is 0.431 where the case holds the bulk velocity at 2/3 (the weighted mean is 0.657), the
    identity sum u_i sgs_i = - sum 2 nu_t S:S holds with the cell widths as weights and not without them, and WALE --
    zero in pure shear, nut_mean 5.2e-6 against nu = 2.4e-4 here -- leaves a signal that the wall layers' excess weight
    outweighs.  A second-order host estimate of the first sub-step gives, per unit time, - 1.9e-6 for the weighted energy
    (work of the term - 1.4e-6, work of the constant-mass-flux shift - 0.5e-6) and - 3e-8 of uncertain sign for the
    unweighted one (its work of the term + 8.9e-7 agrees with the device's + 8.2e-7)."""
    from x3d2_amd.les import LesConfig
    on, off = LesConfig(model=model), LesConfig(model=model, cs=0.0, cw=0.0)
    fused, ke_f, div_f, case = stepped(kind, time_intg, True, on)
    plain, ke_p, div_p, _ = stepped(kind, time_intg, True, None)
    opgran, ke_o, _, _ = stepped(kind, time_intg, False, on)
    zero, _, _, _ = stepped(kind, time_intg, True, off)
    mon = case.solver.les.monitor()
    print("les check: steps", kind, time_intg, model, "fused vs op-granular", field_err(fused, opgran), "c = 0 vs none",
          field_err(zero, plain), "ke", ke_f, ke_p, "div", div_f, div_p, mon)
    assert field_err(fused, opgran) < 1e-12  # the bound of tests/test_hip_ibm.py for fused against op-granular steps
    assert field_err(zero, plain) < 1e-12
    assert field_err(fused, plain) > 1e-9    # the model does something
    assert ke_f < ke_p and ke_o < ke_p
    # the projection leaves round-off of the velocity over the spacing whatever the right-hand side was: the same level,
    # with room for another realisation of the roundings
    assert div_f <= 4.0 * div_p + 1e-300
    assert mon["nut_max"] > 0.0 and 0.0 < mon["diffusion_number"] < 1.0


# ---------------------------------------------------------------- 6. two ranks
MP_DIMS = (48, 80, 80)  # 40 rows per rank in the direction that is cut: rho^40 < 1e-16, the two-rank solve is the one-rank one


def mp_run(layout, rank, comm):
    """(local term [3 arrays], monitor dict, offsets, local dims) of Les.add on this rank's part of the noisy field"""
    from x3d2_amd import make_tgv
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.les import Les, LesConfig
    case = make_tgv(MP_DIMS, nproc_dir=layout, rank=rank, comm=comm, poisson="CG")  # (no Poisson solver is needed)
    s = case.solver
    b = s.backend
    lo = [int(v) for v in b.mesh.n_offset]
    nl = [int(v) for v in b.mesh.get_dims(VERT)]
    for f, a in zip((s.u, s.v, s.w), util.noisy_tgv(MP_DIMS, lo, nl)):
        b.set_field_data(f, a)
    les = Les(s, LesConfig(model="wale"))
    d = [b.allocator.get_block(DIR_X, VERT) for _ in range(3)]
    for f in d:
        f.fill(0.0)
    les.add(*d)
    term_max = None
    if comm is None:  # the largest term of slot 1, for the summation bound: 2 nu_t S:S of the library's own gradients
        grads = s.velocity_gradients()
        g = [b.get_field_data(f).astype(np.float64) for f in grads]
        for f in grads:
            b.allocator.release_block(f)
        nt, _, ss = les_ref.stress(g, les.a_host, "wale", les.cfg.c2, dtype=np.float64)
        term_max = float(np.max(2.0 * nt * ss))
    return [b.get_field_data(f) for f in d], les.monitor(), lo, nl, term_max


@functools.lru_cache(maxsize=None)
def mp_one_rank():
    return mp_run((1, 1, 1), 0, None)


@pytest.mark.parametrize("layout,port", [((1, 1, 2), 29571), ((1, 2, 1), 29572)])
def test_two_ranks_give_the_one_rank_term_and_monitor(layout, port, tmp_path):
    """two processes share the GPU and exchange through gloo (tests/mp_les_worker.py).  The fields agree to 1e-12; the means
    agree to the summation bound of both runs, 2 (P - 1) 2^-52 max|term|, plus the 1e-12 relative the terms themselves may
    differ by (a decomposed derivative is not the bits of the one-rank one)"""
    one, mon1, _, _, term_max = mp_one_rank()
    out = str(tmp_path / "mp")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(HERE, "mp_les_worker.py"),
           ",".join(map(str, layout)), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    parts = [dict(np.load(out + ".%d.npz" % k)) for k in range(2)]
    got = [np.zeros_like(a) for a in one]
    for p in parts:
        lo, nl = p["lo"], p["nl"]
        for c in range(3):
            got[c][lo[2]:lo[2] + nl[2], lo[1]:lo[1] + nl[1], lo[0]:lo[0] + nl[0]] = p["d%d" % c]
    errs = [util.relerr(g, w) for g, w in zip(got, one)]
    print("les check: two ranks", layout, errs)
    assert max(errs) < 1e-12
    assert parts[0]["mon"].tobytes() == parts[1]["mon"].tobytes()  # every rank holds the global figures
    P = float(np.prod(MP_DIMS))
    keys = ("nut_mean", "eps_sgs", "nut_max", "diffusion_number")
    two = dict(zip(keys, parts[0]["mon"]))
    rows = [("nut_mean", abs(two["nut_mean"] - mon1["nut_mean"]), 2 * (P - 1) * EPS * mon1["nut_max"] + 1e-12 * mon1["nut_mean"]),
            ("eps_sgs", abs(two["eps_sgs"] - mon1["eps_sgs"]), 2 * (P - 1) * EPS * term_max + 1e-12 * mon1["eps_sgs"]),
            ("nut_max", abs(two["nut_max"] - mon1["nut_max"]), 1e-12 * mon1["nut_max"]),
            ("diffusion_number", abs(two["diffusion_number"] - mon1["diffusion_number"]), 1e-12 * mon1["diffusion_number"])]
    check_rows(rows)
    assert two["nut_max"] > 0.0


# ---------------------------------------------------------------- 7. restart
def test_restarted_run_with_the_model_gives_the_bits_of_the_uninterrupted_one(tmp_path):
    from x3d2_amd import make_tgv
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    from x3d2_amd.les import Les, LesConfig
    ck = str(tmp_path / "checkpoint")
    cfg = LesConfig(model="wale")
    case = make_tgv(32, fused=True)
    case.solver.les = Les(case.solver, cfg)
    case.checkpoints = Checkpoints(case.solver, CheckpointConfig(checkpoint_freq=2, checkpoint_prefix=ck), case)
    case.run(n_iters=4)
    again = make_tgv(32, fused=True)
    again.solver.les = Les(again.solver, cfg)  # (no state of its own: nothing of it is in the file)
    assert restore(again, ck + "_000002.npz") == 2 and again.restarted
    again.run(n_iters=4)
    sv, pv = case.solver, again.solver
    for f, g in zip((sv.u, sv.v, sv.w), (pv.u, pv.v, pv.w)):
        assert sv.backend.get_field_data(f).tobytes() == pv.backend.get_field_data(g).tobytes()
    assert sv.les.monitor() == pv.les.monitor()


# ---------------------------------------------------------------- 8. errors
def test_bad_calls_raise_launch_nothing_and_a_valid_call_still_works():
    import ctypes
    import torch
    from x3d2_amd import _lib, make_tgv
    from x3d2_amd.common import X3dError
    from x3d2_amd.les import Les, LesConfig
    dims = (35, 9, 6)
    b = make_backend(dims)
    g = synthetic_gradients(dims, 21)
    a, ih = tables_of(b, False, 22)
    da, dih = device_tables(b, a), device_tables(b, ih)
    blocks = poisoned_blocks(b, g)
    before = [whole(f) for f in blocks]
    row = torch.zeros(4, dtype=torch.float64, device=b.device)
    VP = ctypes.c_void_p

    def call(grads=None, dims_=dims, model=1, c2=0.25, tabs=None, row_=row, null=()):
        tabs = [t.data_ptr() for t in da + dih] if tabs is None else tabs
        prm = _lib.LesParams(model, c2, *tabs)
        gp = (VP * 9)(*(grads if grads is not None else [f.ptr for f in blocks]))
        args = [b.h, gp, _lib.ints(*dims_), ctypes.byref(prm), VP(row_.data_ptr())]
        for k in null:
            args[k] = None
        return b.lib.x3d_les_stress(*args), b.lib.x3d_last_error()

    for k in (0, 1, 2, 3, 4):  # the backend, the gradient table, dims, the parameters, the row
        rc, msg = call(null=(k,))
        assert rc != 0 and b"null" in msg
    rc, msg = call(grads=[f.ptr for f in blocks[:8]] + [None])
    assert rc != 0 and b"null" in msg
    rc, msg = call(grads=[f.ptr for f in blocks[:8]] + [blocks[0].ptr])
    assert rc != 0 and b"same block" in msg
    rc, msg = call(tabs=[da[0].data_ptr(), None] + [t.data_ptr() for t in da[2:] + dih])
    assert rc != 0 and b"null" in msg
    for bad in ((35, 0, 6), (-1, 9, 6)):
        rc, msg = call(dims_=bad)
        assert rc != 0 and b"positive" in msg
    rc, msg = call(dims_=(10 ** 6, 9, 6))
    assert rc != 0 and b"outside" in msg
    rc, msg = call(model=2)
    assert rc != 0 and b"unknown model" in msg
    for c2 in (-1e-3, float("nan")):
        rc, msg = call(c2=c2)
        assert rc != 0 and b"negative" in msg
    assert not np.any(row.cpu().numpy())  # nothing was launched: the row and the blocks are what they were
    for f, w in zip(blocks, before):
        assert whole(f).tobytes() == w.tobytes()
    with pytest.raises(X3dError, match="nine"):
        b.les_stress(blocks[:8], "wale", 0.25, da, dih, row.data_ptr())
    with pytest.raises(X3dError, match="unknown model"):
        b.les_stress(blocks, "dynamic", 0.25, da, dih, row.data_ptr())
    with pytest.raises(X3dError, match="negative"):
        b.les_stress(blocks, "wale", -0.25, da, dih, row.data_ptr())
    with pytest.raises(X3dError, match="table"):
        b.les_stress(blocks, "wale", 0.25, da, [t.float() for t in dih], row.data_ptr())
    for f, w in zip(blocks, before):
        assert whole(f).tobytes() == w.tobytes()
    with pytest.raises(X3dError, match="species"):
        Les(make_tgv(16, n_species=1).solver, LesConfig())
    rc, msg = call()  # and a valid call still works
    assert rc == 0
    got = row.cpu().numpy()
    want = les_ref.scalars(g, a, ih, "wale", 0.25)
    assert got[0] > 0.0 and abs(got[2] - float(want[2])) <= float(les_ref.bounds(g, a, "wale", 0.25)[0].max())
    assert b.lib.x3d_abi_version() == 1


# ---------------------------------------------------------------- 9. FP32
def _sp_worker(*args):
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "les_sp_worker.py")] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("LESRESULT ")][-1][10:])


def test_kernel_and_term_in_the_fp32_flavour():
    """check 1 with 2^-24 |ref| (one rounding of a double result) on top of the double bound, the scalars (still FP64),
    and check 4 at the 1e-5 relative of tests/sp_worker.py's operator checks, on 4-byte reals (libx3d2_hip_sp.so)"""
    res = _sp_worker("kernel")
    assert res["dtype"] == "float32" and res["row_dtype"] == "float64"
    assert len(res["rows"]) == 2 * len(SHAPES) * (7 + 4)
    check_rows([tuple(r) for r in res["rows"]])
    print("les check: fp32 term", res["term"])
    assert len(res["term"]) == 4 and max(res["term"].values()) < 1e-5


def test_one_fp32_channel_step_against_the_fp64_library(tmp_path):
    """one fused channel step with WALE attached in FP32 against the FP64 library's, at the FP32 step tolerance of
    tests/test_hip_single_prec.py: fields 2e-5 max(|ref|, 1)"""
    from x3d2_amd.les import LesConfig
    out = str(tmp_path / "sp.npz")
    _sp_worker("step", out)
    ref, _, _, _ = stepped("channel", "RK3", True, LesConfig(model="wale"), nsteps=1)
    got = np.load(out)
    for k, w in zip("uvw", ref):
        assert got[k].dtype == np.float32
        err = float(np.max(np.abs(got[k].astype(np.float64) - w)))
        print("les check: fp32 step", k, err, 2e-5 * max(float(np.max(np.abs(w))), 1.0))
        assert err < 2e-5 * max(float(np.max(np.abs(w))), 1.0)
