"""Eddy diffusivity of the explicit LES on the device (x3d_les_scalar_flux of csrc/les.hip, Les.add with species, x3d2_amd/les.py)
against the longdouble restatement tests/les_scalar_ref.py (pinned on the host by tests/test_les_scalar_host.py) and the dense
operators of tests/util.py.  Helpers and shapes are those of tests/test_hip_les.py.

Pointwise bound (counted, not tuned to the kernel), inputs float32-representable and 1 / Pr_t the double the host hands over:
    kappa = nu_t * (1 / Pr_t) rounds once, q_j = kappa * g_j once, the FP64 store is exact:  |q_j - ref| <= 2 2^-52 |kappa g_j|
Row: a sum of P terms in double, in ANY order, is off by at most (P - 1) 2^-52 P max|term| to first order (the argument of
tests/test_hip_les.py's docstring), plus every term's own error: kappa once, three squares, two additions (or fused
multiply-adds, which round less often) and the product: 6 2^-52 of the term, all terms being non-negative.
Every block is filled with 1e30 before its data are set: a kernel that reads the row padding fails by thirty orders of
magnitude, one that writes it is caught by the comparison of the whole block.

Velocity bits with and without species (check 4): the fused driver takes other kernels for a solver WITHOUT species (the
pressure-gradient correction deferred into the next transeq_x launch, Solver._finish_pressure_correction, and the stage in
the z launch, Solver.transeq_fused: both ask for nspecies == 0), so a fused run with one species and a fused run with none
do not share their bits whatever the model does.  The check is therefore made on the op-granular driver, whose velocity path
does not look at nspecies."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import les_ref
import les_scalar_ref
import test_hip_les as t
import util

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -52
PRT = (0.85, 0.4)
INV_PRT = (1.0 / 0.85, 1.0 / 0.4)
SHAPES, IDS = t.SHAPES, t.IDS


# ---------------------------------------------------------------- helpers (also used by the worker processes)
def synthetic_inputs(dims, ns, seed):
    """nu_t >= 0 with exact zeros (plane k = 0 and one point in eight) and 3 ns standard_normal gradients, all
    float32-representable, [nz, ny, nx]"""
    rng = np.random.default_rng(seed)
    shape = (dims[2], dims[1], dims[0])
    nut = np.abs(rng.standard_normal(shape, dtype=np.float32)).astype(np.float64)
    nut[rng.random(shape) < 0.125] = 0.0
    nut[0] = 0.0
    return nut, [rng.standard_normal(shape, dtype=np.float32).astype(np.float64) for _ in range(3 * ns)]


def run_flux(dims, ybc, stretched, ns, seed=31):
    """one x3d_les_scalar_flux on synthetic blocks, and the same again -> dict of what the tests assert on"""
    import torch
    b = t.make_backend(dims, ybc, stretched)
    nut, g = synthetic_inputs(dims, ns, seed)
    blocks = t.poisoned_blocks(b, [nut] + g)
    before = [t.whole(f) for f in blocks]
    row = torch.full((3,), -7.0, dtype=torch.float64, device=b.device)
    b.les_scalar_flux(blocks[0], blocks[1:], INV_PRT[:ns], row.data_ptr())
    after = [t.whole(f) for f in blocks]
    got = [b.get_field_data(f).astype(np.float64) for f in blocks]
    first = row.cpu().numpy().copy()
    for f, x in zip(blocks, [nut] + g):  # the same input again, in the same blocks: the same bits
        f.fill(1e30)
        b.set_field_data(f, x)
    b.les_scalar_flux(blocks[0], blocks[1:], INV_PRT[:ns], row.data_ptr())
    again = [t.whole(f) for f in blocks]
    second = row.cpu().numpy().copy()
    nxp, nyp, nzp = (int(v) for v in b.padded_dims)
    inside = np.zeros(before[0].shape, dtype=bool)
    inside[:nxp * nyp * nzp].reshape(nzp, nyp, nxp)[:dims[2], :dims[1], :dims[0]] = True
    return dict(nut=nut, g=g, ns=ns, got=got, row=first, row2=second, before=before, after=after, again=again, inside=inside)


@functools.lru_cache(maxsize=None)
def kernel_case(idx, ns):
    dims, ybc, stretched = SHAPES[idx]
    return run_flux(dims, ybc, stretched, ns)


def pointwise_rows(r, extra=None):
    """[(name, worst |err| / bound, 1.0)] of the 3 ns fluxes; extra(ref) -> an additional allowance (FP32)"""
    rows = []
    for s in range(r["ns"]):
        gs = r["g"][3 * s:3 * s + 3]
        ref = les_scalar_ref.flux(r["nut"], gs, INV_PRT[s])
        bound = les_scalar_ref.flux_bound(r["nut"], gs, INV_PRT[s])
        for j in range(3):
            allow = bound[j] + (extra(ref[j]) if extra is not None else 0.0)
            err = np.asarray(np.abs(r["got"][1 + 3 * s + j] - ref[j]), dtype=np.float64)
            ratio = float(np.max(np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), 0.0)))
            rows.append(("q%d%s" % (s, "xyz"[j]), ratio if bool(np.all(err <= allow)) else float("inf"), 1.0))
    return rows


def row_rows(r):
    rows = []
    for s in range(r["ns"]):
        gs = r["g"][3 * s:3 * s + 3]
        terms = np.asarray(les_scalar_ref.row_terms(r["nut"], gs, INV_PRT[s]), dtype=np.float64)
        want = les_scalar_ref.row(r["nut"], gs, INV_PRT[s])
        P = terms.size
        bound = P * (P - 1) * EPS * float(terms.max()) + 6 * EPS * float(terms.sum())
        rows.append(("row%d" % s, float(abs(r["row"][s] - want)), bound))
    return rows


# ---------------------------------------------------------------- 1. the kernel against the restatement
@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_flux_against_the_restatement(idx, ns):
    r = kernel_case(idx, ns)
    t.check_rows(pointwise_rows(r))
    for m in range(1, 1 + 3 * ns):
        assert not np.any(np.isnan(r["got"][m]))
        assert not np.any(r["got"][m][r["nut"] == 0.0]), "nu_t = 0: the flux is zero exactly"
        assert np.any(r["got"][m] != 0.0)
        out = ~r["inside"]
        assert r["after"][m][out].tobytes() == r["before"][m][out].tobytes(), "row padding of block %d was written" % m
    assert r["after"][0].tobytes() == r["before"][0].tobytes(), "nu_t is left as it is"


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_rows_against_fsum_and_twice_the_same_bits(idx, ns):
    r = kernel_case(idx, ns)
    assert r["row"].dtype == np.float64 and np.all(r["row"][:ns] > 0.0)
    assert np.all(r["row"][ns:] == -7.0), "only ns values of the row are written"
    t.check_rows(row_rows(r))
    assert r["row"].tobytes() == r["row2"].tobytes()
    for m in range(1 + 3 * ns):
        assert r["after"][m].tobytes() == r["again"][m].tobytes()


# ---------------------------------------------------------------- 2. plumbing, bit-exact
PR_SPECIES = [0.7, 1.0, 0.4]
PRT3 = [0.85, 0.4, 0.7]


def species_case(kind, ns, fused=True, time_intg="RK3", dims=None):
    """tests/test_hip_les.py's small_case with ns transported species"""
    from x3d2_amd import make_channel, make_tgv
    kw = dict(fused=fused, time_intg=time_intg, poisson="CG", n_species=ns, pr_species=PR_SPECIES[:ns])
    if kind == "box":
        dims = dims or (24, 20, 16)
        case = make_tgv(dims, **kw)
    elif kind == "wall":  # uniform Dirichlet y
        dims = dims or (24, 20, 16)
        case = make_channel(dims, stretching="uniform", beta=1.0, **kw)
    else:
        dims = dims or (24, 33, 16)
        case = make_channel(dims, **kw)
    return case, dims


def set_phi(case, dims):
    """species s <- les_scalar_ref.noisy_phi with its own noise, float32-representable; returns the host fields"""
    from x3d2_amd.common import VERT
    s = case.solver
    out = []
    for k, f in enumerate(s.species):
        a = (les_scalar_ref.noisy_phi(dims, salt=4 + k) * (1.0 + 0.5 * k)).astype(np.float32).astype(np.float64)
        f.set_data_loc(VERT)
        s.backend.set_field_data(f, a)
        out.append(a)
    return out


def seeded(b, dims, seed, n):
    rng = np.random.default_rng(seed)
    return t.poisoned_blocks(b, [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64)
                                 for _ in range(n)])


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("kind", ["channel", "box"])
def test_add_with_species_is_the_kernel_and_three_accumulated_derivatives_bit_for_bit(kind, ns):
    """three species: a group of two, then a group of one"""
    import torch
    from x3d2_amd.common import DIR_X, DIR_Y, DIR_Z
    from x3d2_amd.les import Les, LesConfig
    case, dims = species_case(kind, ns)
    s = case.solver
    b = s.backend
    t.set_noisy(case, dims)
    set_phi(case, dims)
    les = Les(s, LesConfig(model="wale", prt=PRT3[:ns]))
    assert les.serves_species and les.row_phi.dtype == torch.float64 and les.row_phi.numel() == ns and les.row_phi.is_cuda
    dirs = ((s.xdirps, DIR_X), (s.ydirps, DIR_Y), (s.zdirps, DIR_Z))
    grads = s.velocity_gradients()
    les.stress(grads)
    nut = b.get_field_data(grads[t.NUT_AT])  # (downloaded, and handed back in a block of its own)
    for g in grads:
        b.allocator.release_block(g)
    nb = t.poisoned_blocks(b, [nut])[0]
    hand = seeded(b, dims, 6, ns)
    want_row = []
    for s0 in range(0, ns, 2):
        n = min(2, ns - s0)
        gb = t.poisoned_blocks(b, [np.zeros((dims[2], dims[1], dims[0]))] * (3 * n))
        for q in range(n):
            for j, (dirps, d) in enumerate(dirs):
                b.tds_apply(gb[3 * q + j], s.species[s0 + q], dirps.der1st, d)
        row = torch.zeros(n, dtype=torch.float64, device=b.device)
        b.les_scalar_flux(nb, gb, [1.0 / p for p in PRT3[s0:s0 + n]], row.data_ptr())
        for q in range(n):
            for j, (dirps, d) in enumerate(dirs):
                b.tds_apply(hand[s0 + q], gb[3 * q + j], dirps.der1st, d, accumulate=True)
        want_row += list(row.cpu().numpy())
    want = [b.get_field_data(f) for f in hand]
    vel = seeded(b, dims, 5, 3)
    les.add(*vel)  # the call without species: today's sequence
    want_vel = [b.get_field_data(f) for f in vel]
    mine_vel, mine = seeded(b, dims, 5, 3), seeded(b, dims, 6, ns)
    torch.cuda.synchronize()
    free0, n0 = len(b.allocator.free), b.sync_count()
    les.add(*mine_vel, mine, list(s.species))
    assert len(b.allocator.free) >= free0  # the nine blocks went back to the pool, no tenth was taken and kept
    assert b.sync_count() == n0            # no call waited for the host
    for f, w in zip(mine_vel, want_vel):
        assert b.get_field_data(f).tobytes() == w.tobytes()
    for f, w in zip(mine, want):
        got = b.get_field_data(f)
        assert got.tobytes() == w.tobytes() and np.all(np.isfinite(got))
    assert les.row_phi.cpu().numpy().tobytes() == np.array(want_row).tobytes()
    m = les.monitor()
    assert len(m["eps_phi"]) == ns and all(e > 0.0 for e in m["eps_phi"])
    assert m["diffusion_number_phi"] == m["diffusion_number"] / min(PRT3[:ns]) > 0.0
    assert m["nut_max"] >= m["nut_mean"] > 0.0 and m["eps_sgs"] > 0.0


# ---------------------------------------------------------------- 3. the whole term against dense operators
def dense_reference(mesh, dims, u, v, w, phi, model, c2, inv_prt):
    deltas = [float(x) for x in mesh.d]
    ops = les_ref.dense_der1st(dims, deltas, [tuple(mesh.BCs_global[k]) for k in range(3)])
    tables = [np.full(n, h ** (2.0 / 3.0)) for n, h in zip(dims, deltas)]
    _, nt, _ = les_ref.dense_term(u, v, w, ops, tables, model, c2)
    return les_scalar_ref.dense_scalar_term(phi, nt, ops, inv_prt)


def device_term(kind, model, dims=(40, 40, 40)):
    """(device term of species 0, monitor, reference (sgs, g, kappa), phi) of Les.add on the noisy fields"""
    from x3d2_amd.common import DIR_X, VERT
    from x3d2_amd.les import Les, LesConfig
    case, dims = species_case(kind, 1, dims=dims)
    s = case.solver
    b = s.backend
    u, v, w = (np.asarray(a, dtype=b.get_field_data(s.u).dtype).astype(np.float64) for a in t.set_noisy(case, dims))
    phi = set_phi(case, dims)[0]
    cfg = LesConfig(model=model, prt=PRT[0])
    les = Les(s, cfg)
    d = [b.allocator.get_block(DIR_X, VERT) for _ in range(4)]
    for f in d:
        f.fill(0.0)
    n0 = b.sync_count()
    les.add(d[0], d[1], d[2], [d[3]], list(s.species))
    assert b.sync_count() == n0  # no call waited for the host
    got = b.get_field_data(d[3]).astype(np.float64)
    return got, les.monitor(), dense_reference(s.mesh, dims, u, v, w, phi, model, cfg.c2, INV_PRT[0]), phi


@pytest.mark.parametrize("kind", ["box", "wall"])
def test_species_term_against_the_dense_restatement(kind):
    """40^3, not smaller: DER1ST_RHO^n < 1e-16 (tests/test_hip_les.py::test_term_against_the_dense_restatement).  Smagorinsky:
    its nu_t does not vanish at the wall, so the wall rows of the operators carry weight"""
    dims = (40, 40, 40)
    assert all(t.DER1ST_RHO ** n < 1e-16 for n in dims)
    got, mon, (sgs, g, k), phi = device_term(kind, "smagorinsky")
    err = util.relerr(got, sgs)
    n = float(np.prod(dims))
    eps = float(np.sum(k * ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]))) / n
    print("les scalar check: term", kind, err, "eps_phi", mon["eps_phi"], eps)
    assert err < 1e-12
    assert eps > 0.0 and abs(mon["eps_phi"][0] - eps) <= 1e-12 * eps
    if kind == "box":  # conservation and the variance identity of the conservative form, on the device term
        assert abs(float(np.sum(got))) <= 1e-12 * float(np.sum(np.abs(got)))
        work = float(np.sum(phi * got)) / n
        print("les scalar check: variance identity", work, mon["eps_phi"][0])
        assert abs(work + mon["eps_phi"][0]) <= 1e-12 * mon["eps_phi"][0]


# ---------------------------------------------------------------- 4. steps
def smooth_phi(m):
    X = 2 * np.pi * m.vert_coords[0][None, None, :] / m.L[0]
    Y = np.pi * m.vert_coords[1][None, :, None] / m.L[1]
    Z = 2 * np.pi * m.vert_coords[2][:, None, None] / m.L[2]
    return np.sin(X) * np.cos(2 * Y) * np.cos(Z) + 0.5 * np.sin(2 * X + Z) * np.cos(Y)


def stepped(kind, time_intg, fused, cfg, nsteps=2, species=True):
    """([u, v, w, phi] after nsteps steps, case); cfg = None: no model attached; species = False: a solver without species"""
    from x3d2_amd import make_channel, make_tgv
    from x3d2_amd.common import VERT
    from x3d2_amd.les import Les
    kw = dict(fused=fused, time_intg=time_intg)
    if kind == "tgv":
        case = make_tgv(32, **kw, **(dict(n_species=1, pr_species=[0.7]) if species else {}))
    else:
        case = make_channel((24, 33, 16), **kw, **(dict(n_species=1, pr_species=[0.71]) if species else {}))
        s = case.solver
        for f, p in zip((s.u, s.v, s.w), t.perturbation(s.mesh)):
            s.backend.set_field_data(f, s.backend.get_field_data(f) + p)
    s = case.solver
    if species:
        s.species[0].set_data_loc(VERT)
        s.backend.set_field_data(s.species[0], smooth_phi(s.mesh) + np.zeros(tuple(int(n) for n in s.mesh.vert_dims)[::-1]))
    assert s.les is None
    if cfg is not None:
        s.les = Les(s, cfg)
    for it in range(1, nsteps + 1):
        case.step(it)
    s.flush_grad()
    return [s.backend.get_field_data(f).astype(np.float64) for f in [s.u, s.v, s.w] + list(s.species)], case


@pytest.mark.parametrize("kind,time_intg,model", [("tgv", "RK3", "smagorinsky"), ("tgv", "AB3", "wale"),
                                                   ("channel", "RK3", "wale")])
def test_steps_with_species_and_the_model(kind, time_intg, model):
    from x3d2_amd.les import LesConfig
    on = LesConfig(model=model, prt=0.85)
    off = LesConfig(model=model, cs=0.0, cw=0.0, prt=0.85)
    fused, case = stepped(kind, time_intg, True, on)
    opgran, _ = stepped(kind, time_intg, False, on)
    zero, _ = stepped(kind, time_intg, True, off)
    plain, _ = stepped(kind, time_intg, True, None)
    bare, _ = stepped(kind, time_intg, False, LesConfig(model=model), species=False)
    mon = case.solver.les.monitor()
    var_on, var_off = float(np.sum(fused[3] ** 2)), float(np.sum(plain[3] ** 2))
    print("les scalar check: steps", kind, time_intg, model, "fused vs op-granular", t.field_err(fused, opgran),
          "c = 0 vs none", t.field_err(zero, plain), "phi with vs without", util.relerr(fused[3], plain[3]),
          "sum phi^2", var_on, var_off, mon)
    assert t.field_err(fused, opgran) < 1e-12  # the bound of tests/test_hip_ibm.py for fused against op-granular steps
    assert t.field_err(zero, plain) < 1e-12
    assert util.relerr(fused[3], plain[3]) > 1e-9  # the eddy diffusivity does something
    if kind == "tgv":
        assert var_on < var_off
    assert 0.0 < mon["diffusion_number_phi"] < 1.0 and mon["eps_phi"][0] > 0.0
    # a passive species does not reach the velocity: the bits of LES on a solver without species (the module docstring says
    # why this is the op-granular driver)
    for a, c in zip(opgran[:3], bare):
        assert a.tobytes() == c.tobytes()


# ---------------------------------------------------------------- 5. Rayleigh-Benard with the model
def rb_case():
    from x3d2_amd import make_rayleigh_benard
    from x3d2_amd.les import LesConfig
    return make_rayleigh_benard((32, 33, 16), Ra=1e6, Pr=1.0, les=LesConfig(model="wale"), seed=7, fused=True)


def test_rayleigh_benard_with_wale_and_its_restart(tmp_path):
    """the model has no state: a checkpoint holds nothing of it, and the restarted run gives the bits of the uninterrupted one"""
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    ck = str(tmp_path / "checkpoint")
    case = rb_case()
    s = case.solver
    assert s.les is not None and s.les.serves_species and s.les.prt == [0.85] and s.scalars is not None
    case.checkpoints = Checkpoints(s, CheckpointConfig(checkpoint_freq=2, checkpoint_prefix=ck), case)
    case.run(n_iters=3)
    s.flush_grad()
    fields = [s.backend.get_field_data(f) for f in (s.u, s.v, s.w, s.species[0])]
    assert all(np.all(np.isfinite(a)) for a in fields)
    phi = fields[3]
    assert np.all(phi[:, 0, :] == 1.0) and np.all(phi[:, -1, :] == 0.0)
    mon = s.les.monitor()
    assert mon["eps_phi"][0] >= 0.0 and np.isfinite(mon["eps_phi"][0])
    sm = s.scalars.monitor()
    assert all(np.all(np.isfinite(np.asarray(v))) for v in sm.values())
    again = rb_case()
    assert restore(again, ck + "_000002.npz") == 2 and again.restarted
    again.run(n_iters=3)
    p = again.solver
    p.flush_grad()
    for a, f in zip(fields, (p.u, p.v, p.w, p.species[0])):
        assert a.tobytes() == p.backend.get_field_data(f).tobytes()
    assert p.les.monitor() == mon


# ---------------------------------------------------------------- 6. two ranks
MP_DIMS = t.MP_DIMS


def mp_run(layout, rank, comm):
    """(local species term, monitor dict, offsets, local dims, largest term of the row) of Les.add with one species on this
    rank's part of the noisy fields"""
    from x3d2_amd import make_tgv
    from x3d2_amd.common import DIR_X, DIR_Y, DIR_Z, VERT
    from x3d2_amd.les import Les, LesConfig
    case = make_tgv(MP_DIMS, nproc_dir=layout, rank=rank, comm=comm, poisson="CG", n_species=1, pr_species=[0.7])
    s = case.solver
    b = s.backend
    lo = [int(v) for v in b.mesh.n_offset]
    nl = [int(v) for v in b.mesh.get_dims(VERT)]
    for f, a in zip((s.u, s.v, s.w), util.noisy_tgv(MP_DIMS, lo, nl)):
        b.set_field_data(f, a)
    s.species[0].set_data_loc(VERT)
    b.set_field_data(s.species[0], les_scalar_ref.noisy_phi(MP_DIMS, lo, nl))
    les = Les(s, LesConfig(model="wale", prt=PRT[0]))
    d = [b.allocator.get_block(DIR_X, VERT) for _ in range(4)]
    for f in d:
        f.fill(0.0)
    les.add(d[0], d[1], d[2], [d[3]], list(s.species))
    term_max = None
    if comm is None:  # the largest term of the row, for the summation bound, from the library's own gradients
        grads = s.velocity_gradients()
        les.stress(grads)
        nut = b.get_field_data(grads[t.NUT_AT]).astype(np.float64)
        g = []
        for dirps, direction in ((s.xdirps, DIR_X), (s.ydirps, DIR_Y), (s.zdirps, DIR_Z)):
            b.tds_apply(grads[0], s.species[0], dirps.der1st, direction)
            g.append(b.get_field_data(grads[0]).astype(np.float64))
        for f in grads:
            b.allocator.release_block(f)
        term_max = float(np.max(nut * INV_PRT[0] * (g[0] ** 2 + g[1] ** 2 + g[2] ** 2)))
    return b.get_field_data(d[3]), les.monitor(), lo, nl, term_max


@functools.lru_cache(maxsize=None)
def mp_one_rank():
    return mp_run((1, 1, 1), 0, None)


@pytest.mark.parametrize("layout,port", [((1, 1, 2), 29581), ((1, 2, 1), 29582)])
def test_two_ranks_give_the_one_rank_species_term_and_eps_phi(layout, port, tmp_path):
    """the form and the tolerances of tests/test_hip_les.py::test_two_ranks_give_the_one_rank_term_and_monitor"""
    one, mon1, _, _, term_max = mp_one_rank()
    out = str(tmp_path / "mp")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(HERE, "mp_les_scalar_worker.py"),
           ",".join(map(str, layout)), out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    parts = [dict(np.load(out + ".%d.npz" % k)) for k in range(2)]
    got = np.zeros_like(one)
    for p in parts:
        lo, nl = p["lo"], p["nl"]
        got[lo[2]:lo[2] + nl[2], lo[1]:lo[1] + nl[1], lo[0]:lo[0] + nl[0]] = p["dphi"]
    err = util.relerr(got, one)
    print("les scalar check: two ranks", layout, err)
    assert err < 1e-12
    assert parts[0]["mon"].tobytes() == parts[1]["mon"].tobytes()  # every rank holds the global figures
    P = float(np.prod(MP_DIMS))
    eps2, dn2 = (float(x) for x in parts[0]["mon"])
    rows = [("eps_phi", abs(eps2 - mon1["eps_phi"][0]), 2 * (P - 1) * EPS * term_max + 1e-12 * mon1["eps_phi"][0]),
            ("diffusion_number_phi", abs(dn2 - mon1["diffusion_number_phi"]), 1e-12 * mon1["diffusion_number_phi"])]
    t.check_rows(rows)
    assert eps2 > 0.0


# ---------------------------------------------------------------- 7. deferred execution
def lazy_channel_case(lazy):
    """tests/test_hip_lazy_addons.py's channel with WALE, one species and its eddy diffusivity"""
    import test_hip_lazy_addons as la
    from x3d2_amd import make_channel
    from x3d2_amd.les import Les, LesConfig
    case = make_channel(la.CHANNEL_DIMS, lazy=lazy, n_species=1, pr_species=[0.71], **la.CHANNEL)
    s = case.solver
    m = s.mesh  # (channel_les_case's three-dimensional start that vanishes on the walls)
    x, y, z = (np.asarray(m.vert_coords[0])[None, None, :], np.asarray(m.vert_coords[1])[None, :, None] - 1.0,
               np.asarray(m.vert_coords[2])[:, None, None])
    kx, kz, env = 2.0 * np.pi / m.L[0], 2.0 * np.pi / m.L[2], 1.0 - y * y
    env[:, [0, -1], :] = 0.0
    for f, a in zip((s.u, s.v, s.w), (env * (1.0 + 0.3 * np.sin(kx * x) * np.cos(kz * z)), 0.2 * env * np.sin(2 * kx * x) * np.sin(kz * z),
                                      0.2 * env * np.cos(kx * x) * np.sin(2 * kz * z))):
        s.backend.set_field_data(f, a + 0.0 * (x + z))
    la.set_species(s, la.CHANNEL_PHI)
    case.calls = la.counting(s.backend, ("les_stress", "les_scalar_flux"))
    s.les = Les(s, LesConfig(model="wale", prt=PRT[0]))
    return case


def lazy_outputs(case):
    import test_hip_lazy_addons as la
    import torch
    o = la.fields_of(case)
    torch.cuda.synchronize()
    o["les_row"], o["les_row_phi"] = case.solver.les.row.cpu().numpy(), case.solver.les.row_phi.cpu().numpy()
    return o


def test_deferred_channel_steps_with_wale_and_a_species(monkeypatch):
    import test_hip_lazy_addons as la
    eager = lazy_channel_case(False)
    eager.run(n_iters=2)
    oe = lazy_outputs(eager)
    lazy = lazy_channel_case(True)
    lazy.run(n_iters=2)
    la.report("channel + wale + species", lazy.solver.backend)
    ol = lazy_outputs(lazy)
    names = ("u", "v", "w", "phi_1")
    worst = la.worst_ulp({k: oe[k] for k in names}, {k: ol[k] for k in names})
    print("channel + wale + species, default rules: worst distance %.3f ulp of the field maximum (bound 16)" % worst)
    print("channel + wale + species, default rules: row_phi eager %s deferred %s" % (oe["les_row_phi"], ol["les_row_phi"]))
    monkeypatch.setenv("X3D_LAZY_RULES", la.RULES_EXACT)
    exact = lazy_channel_case(True)
    exact.run(n_iters=2)
    la.report("channel + wale + species, rules %s" % la.RULES_EXACT, exact.solver.backend)
    assert worst <= 16.0
    la.same_bits("channel + wale + species without the reassociating rewrites", oe, lazy_outputs(exact))
    nsub = 2 * lazy.solver.time_integrator.nstage
    for case in (eager, lazy, exact):
        assert case.calls["les_scalar_flux"] == nsub and case.calls["les_stress"] == nsub
    assert oe["les_row_phi"][0] > 0.0


# ---------------------------------------------------------------- 8. errors
def test_bad_calls_raise_launch_nothing_and_a_valid_call_still_works():
    import ctypes
    import torch
    from x3d2_amd import make_tgv
    from x3d2_amd.common import DIR_X, VERT, X3dError
    from x3d2_amd.les import Les, LesConfig
    dims = (35, 9, 6)
    b = t.make_backend(dims)
    nut, g = synthetic_inputs(dims, 2, 41)
    blocks = t.poisoned_blocks(b, [nut] + g)
    before = [t.whole(f) for f in blocks]
    row = torch.zeros(2, dtype=torch.float64, device=b.device)
    VP, DBL = ctypes.c_void_p, ctypes.c_double
    from x3d2_amd import _lib

    def call(nut_=blocks[0].ptr, gphi=None, ns=2, dims_=dims, ipr=INV_PRT, null=()):
        gphi = [f.ptr for f in blocks[1:1 + 3 * max(min(ns, 2), 1)]] if gphi is None else gphi
        args = [b.h, nut_, (VP * len(gphi))(*gphi), ns, _lib.ints(*dims_), (DBL * len(ipr))(*ipr), VP(row.data_ptr())]
        for k in null:
            args[k] = None
        return b.lib.x3d_les_scalar_flux(*args), b.lib.x3d_last_error()

    for k in (0, 1, 2, 4, 5, 6):  # the backend, nu_t, the gradient table, dims, 1 / Pr_t, the row
        rc, msg = call(null=(k,))
        assert rc != 0 and b"null" in msg
    rc, msg = call(gphi=[f.ptr for f in blocks[1:6]] + [None])
    assert rc != 0 and b"null" in msg
    for ns in (0, 3, -1):
        rc, msg = call(ns=ns)
        assert rc != 0 and b"1 or 2" in msg
    for bad in ((35, 0, 6), (-1, 9, 6)):
        rc, msg = call(dims_=bad)
        assert rc != 0 and b"positive" in msg
    rc, msg = call(dims_=(10 ** 6, 9, 6))
    assert rc != 0 and b"outside" in msg
    for x in (0.0, -1.0, float("nan"), float("inf")):
        for ipr in ((x, 1.0), (1.0, x)):
            rc, msg = call(ipr=ipr)
            assert rc != 0 and b"finite and positive" in msg
    rc, msg = call(gphi=[f.ptr for f in blocks[1:6]] + [blocks[0].ptr])
    assert rc != 0 and b"same block" in msg
    rc, msg = call(gphi=[f.ptr for f in blocks[1:6]] + [blocks[2].ptr])
    assert rc != 0 and b"same block" in msg
    rc, msg = call(ns=1, gphi=[blocks[1].ptr, blocks[2].ptr, blocks[1].ptr])
    assert rc != 0 and b"same block" in msg
    assert not np.any(row.cpu().numpy())  # nothing was launched: the row and the blocks are what they were
    for f, w in zip(blocks, before):
        assert t.whole(f).tobytes() == w.tobytes()
    with pytest.raises(X3dError, match="one or two"):
        b.les_scalar_flux(blocks[0], blocks[1:7] + blocks[1:4], [1.0, 1.0, 1.0], row.data_ptr())
    with pytest.raises(X3dError, match="three gradient"):
        b.les_scalar_flux(blocks[0], blocks[1:6], INV_PRT, row.data_ptr())
    for x in (0.0, -2.0, float("nan")):
        with pytest.raises(X3dError, match="finite and positive"):
            b.les_scalar_flux(blocks[0], blocks[1:4], [x], row.data_ptr())
    cell = b.allocator.get_block(DIR_X)
    with pytest.raises(X3dError, match="VERT"):
        b.les_scalar_flux(cell, blocks[1:4], INV_PRT[:1], row.data_ptr())
    with pytest.raises(X3dError):  # two equal blocks, through the Python layer: the library's refusal
        b.les_scalar_flux(blocks[0], [blocks[1], blocks[2], blocks[1]], INV_PRT[:1], row.data_ptr())
    assert not np.any(row.cpu().numpy())
    for f, w in zip(blocks, before):
        assert t.whole(f).tobytes() == w.tobytes()
    with pytest.raises(X3dError, match="species"):
        Les(make_tgv(16, n_species=1, poisson="CG").solver, LesConfig())
    with pytest.raises(X3dError, match="entries"):
        Les(make_tgv(16, n_species=1, poisson="CG").solver, LesConfig(prt=[0.85, 0.4]))
    plain = Les(make_tgv(16, poisson="CG").solver, LesConfig(prt=0.85))
    assert not plain.serves_species and plain.row_phi.numel() == 0 and "eps_phi" not in plain.monitor()
    with pytest.raises(X3dError, match="species"):
        plain.add(*blocks[1:4], [blocks[4]], [blocks[5]])
    rc, msg = call()  # and a valid call still works
    assert rc == 0
    r = dict(nut=nut, g=g, ns=2, row=row.cpu().numpy(), got=[b.get_field_data(f).astype(np.float64) for f in blocks])
    t.check_rows(pointwise_rows(r) + row_rows(r))
    assert b.lib.x3d_abi_version() == 1


# ---------------------------------------------------------------- 9. FP32
def _sp_worker(*args):
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "les_scalar_sp_worker.py")] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, X3D_SINGLE_PREC="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("LESRESULT ")][-1][10:])


def test_kernel_and_term_in_the_fp32_flavour():
    """check 1 with 2^-24 |ref| (one rounding of a double result) on top of the double bound, the rows (still FP64), and
    check 3 at the 1e-5 relative of tests/sp_worker.py's operator checks, on 4-byte reals (libx3d2_hip_sp.so)"""
    res = _sp_worker("kernel")
    assert res["dtype"] == "float32" and res["row_dtype"] == "float64"
    assert len(res["rows"]) == len(SHAPES) * (3 + 1) * 3  # ns = 1 and ns = 2: 3 + 6 fluxes, 1 + 2 rows per shape
    t.check_rows([tuple(r) for r in res["rows"]])
    print("les scalar check: fp32 term", res["term"])
    assert len(res["term"]) == 2 and max(res["term"].values()) < 1e-5


def test_one_fp32_channel_step_with_a_species_against_the_fp64_library(tmp_path):
    """one fused channel step with WALE and the eddy diffusivity in FP32 against the FP64 library's, at the FP32 step
    tolerance of tests/test_hip_single_prec.py: fields 2e-5 max(|ref|, 1)"""
    from x3d2_amd.les import LesConfig
    out = str(tmp_path / "sp.npz")
    _sp_worker("step", out)
    ref, _ = stepped("channel", "RK3", True, LesConfig(model="wale", prt=PRT[0]), nsteps=1)
    got = np.load(out)
    for k, w in zip(("u", "v", "w", "phi"), ref):
        assert got[k].dtype == np.float32
        err = float(np.max(np.abs(got[k].astype(np.float64) - w)))
        print("les scalar check: fp32 step", k, err, 2e-5 * max(float(np.max(np.abs(w))), 1.0))
        assert err < 2e-5 * max(float(np.max(np.abs(w))), 1.0)
