"""Immersed boundary, host side (no GPU): the mask builder, the .npz form of the reference's ibm file, the ABI names, and
the pin of the GPU tests' checker (tests/cylinder_ref.py) on the oracle's own step."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("x3d_ibm_create", "x3d_ibm_destroy", "x3d_ibm_counts", "x3d_ibm_body", "x3d_outflow_params",
                "x3d_outflow_params_get", "x3d_cylinder_apply_bc", "x3d_inlet_noise")


def _mesh(dims=(65, 32, 8), L=(20.0, 12.0, 6.0), stretched=False):
    from x3d2_amd import Mesh
    if stretched:
        return Mesh(dims, (1, 1, 1), L, ("periodic",) * 2, ("dirichlet",) * 2, ("periodic",) * 2,
                    ("uniform", "top-bottom", "uniform"), (1.0, 0.259065151, 1.0))
    return Mesh(dims, (1, 1, 1), L, ("dirichlet",) * 2, ("periodic",) * 2, ("periodic",) * 2)


def _count_inside(mesh, cx, cy, r):
    """an independent count: a plain loop over the vertex coordinates"""
    n = 0
    for y in mesh.vert_coords[1]:
        for x in mesh.vert_coords[0]:
            n += (x - cx) * (x - cx) + (y - cy) * (y - cy) < r * r
    return n * len(mesh.vert_coords[2])


def test_cylinder_mask_point_count_and_values():
    from x3d2_amd.ibm import cylinder_mask
    m = _mesh()
    ep1 = cylinder_mask(m, (5.0, 6.0), 1.3)
    assert ep1.shape == (8, 32, 65) and ep1.dtype == np.float64
    assert set(np.unique(ep1)) == {0.0, 1.0}
    assert int((ep1 == 0).sum()) == _count_inside(m, 5.0, 6.0, 1.3) > 0
    assert np.array_equal(ep1, ep1[:1].repeat(8, axis=0))  # the axis runs along z
    # the same with all three coordinates given, and along another axis
    assert np.array_equal(cylinder_mask(m, (5.0, 6.0, 99.0), 1.3, axis=2), ep1)
    along_y = cylinder_mask(m, (5.0, 3.0), 1.3, axis=1)
    assert np.array_equal(along_y, along_y[:, :1].repeat(32, axis=1)) and (along_y == 0).any()


def test_cylinder_mask_is_symmetric_about_its_centre():
    from x3d2_amd.ibm import cylinder_mask
    m = _mesh()
    # a centre on a vertex in x (x_16 = 5.0) and in y (y_16 = 6.0): the mask mirrors about both
    ep1 = cylinder_mask(m, (m.vert_coords[0][16], m.vert_coords[1][16]), 1.3)[0]
    assert np.array_equal(ep1[:, 0:33], ep1[:, 0:33][:, ::-1])
    assert np.array_equal(ep1[1:32], ep1[1:32][::-1])  # rows 1..31 about row 16
    assert (ep1 == 0).any()


def test_cylinder_mask_radius_zero_is_all_ones_and_a_sphere_is_a_sphere():
    from x3d2_amd.ibm import cylinder_mask
    m = _mesh()
    assert np.all(cylinder_mask(m, (5.0, 6.0), 0.0) == 1.0)
    sph = cylinder_mask(m, (5.0, 6.0, 3.0), 1.5, axis=None)
    x, y, z = (np.asarray(c) for c in m.vert_coords)
    want = ((x[None, None, :] - 5.0) ** 2 + (y[None, :, None] - 6.0) ** 2 + (z[:, None, None] - 3.0) ** 2) < 1.5 ** 2
    assert np.array_equal(sph == 0, want) and want.any() and not want.all()


def test_cylinder_mask_on_a_stretched_y_mesh_uses_the_stretched_coordinates():
    from x3d2_amd.ibm import cylinder_mask
    m = _mesh((32, 33, 8), (4.0, 2.0, 2.0), stretched=True)
    y = np.asarray(m.vert_coords[1])
    assert not np.allclose(np.diff(y), np.diff(y)[0])  # (the mesh IS stretched)
    ep1 = cylinder_mask(m, (2.0, 0.3), 0.25)
    assert int((ep1 == 0).sum()) == _count_inside(m, 2.0, 0.3, 0.25) > 0
    # on uniform coordinates of the same extent the count differs: the builder did not assume them
    yu = np.linspace(0.0, 2.0, 33)
    x = np.asarray(m.vert_coords[0])
    uniform = int((((x[None, :] - 2.0) ** 2 + (yu[:, None] - 0.3) ** 2) < 0.25 ** 2).sum()) * 8
    assert uniform != int((ep1 == 0).sum())


def test_mask_file_round_trip_under_the_reference_names(tmp_path):
    """the reference's reader asks for "iibm" and "ep1" (src/module/ibm.f90:104, 123)"""
    from x3d2_amd.common import X3dError
    from x3d2_amd.ibm import cylinder_mask, load_mask, save_mask
    ep1 = cylinder_mask(_mesh(), (5.0, 6.0), 1.3)
    ep1[0, 0, 0] = 0.25  # (a fractional value survives too)
    path = str(tmp_path / "ibm_100.npz")
    save_mask(path, ep1, 1)
    with np.load(path) as z:
        assert sorted(z.files) == ["ep1", "iibm"]
        assert z["iibm"].dtype == np.int64 and int(z["iibm"]) == 1
        assert z["ep1"].shape == ep1.shape and z["ep1"].flags.c_contiguous
    iibm, back = load_mask(path)
    assert iibm == 1 and np.array_equal(back, ep1)
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, ep1=ep1)
    with pytest.raises(X3dError):
        load_mask(bad)


def test_entry_points_are_declared_in_header_ctypes_and_fortran():
    from x3d2_amd import _lib
    header = open(os.path.join(ROOT, "include", "x3d2_hip.h")).read()
    capi = open(os.path.join(ROOT, "fortran", "m_x3d2_hip_capi.f90")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
        assert "bind(C, name='%s')" % name in capi, name


def test_config_surface():
    from x3d2_amd.case import CylinderCase, CylinderConfig  # noqa: F401
    from x3d2_amd.solver import SolverConfig
    import x3d2_amd
    assert callable(x3d2_amd.make_cylinder)
    c = CylinderConfig()
    assert c.init_noise == (0.0, 0.0, 0.0) and c.inlet_noise == (0.0, 0.0, 0.0) and c.seed is None
    assert SolverConfig().ibm_on is False and SolverConfig(ibm_on=True).ibm_on is True


@pytest.mark.parametrize("time_intg", ["AB3", "RK3"])
def test_cylinder_ref_with_a_mask_of_ones_and_no_bc_is_the_oracle_step(time_intg):
    """the checker pins itself: on an all-periodic mesh, ep1 = 1 everywhere and the BC steps switched off, three steps of
    the composition reproduce orc.Solver.step bit for bit"""
    from oracle import x3d_oracle as orc
    import cylinder_ref
    dims, L = (32, 16, 8), (20.0, 12.0, 6.0)
    ref = cylinder_ref.CylinderRef(dims, L, time_intg=time_intg, ep1=np.ones((8, 16, 32)), bc=False,
                                   bc_x=("periodic", "periodic"))
    om = orc.Mesh(list(dims), [1, 1, 1], list(L), ["periodic"] * 2, ["periodic"] * 2, ["periodic"] * 2)
    o = orc.Solver(om, Re=300.0, dt=0.0075, time_intg=time_intg, poisson="FFT")
    for f in (o.u, o.v, o.w):
        f.data_loc = orc.VERT
    X = 2 * np.pi * np.asarray(om.vert_coords[0])[None, None, :] / L[0]
    Y = 2 * np.pi * np.asarray(om.vert_coords[1])[None, :, None] / L[1]
    Z = 2 * np.pi * np.asarray(om.vert_coords[2])[:, None, None] / L[2]
    init = (1.0 + 0.05 * np.sin(X) * np.cos(Y) * np.cos(Z), 0.04 * np.cos(X) * np.sin(Y) * np.cos(Z),
            0.03 * np.sin(2 * X) * np.cos(Y) * np.sin(Z))
    ref.set_velocity(*init)
    for f, a in zip((o.u, o.v, o.w), init):
        o.backend.set_field_data(f, a)
    for _ in range(3):
        ref.step()
        o.step()
    for got, f in zip(ref.velocity(), (o.u, o.v, o.w)):
        want = o.backend.get_field_data(f)
        assert np.all(np.isfinite(want)) and np.array_equal(got, want)
    assert ref.monitor() == o.monitor()


def test_cylinder_ref_runs_the_cylinder_and_keeps_the_reference_quirks():
    """three AB3 steps at 33 x 16 x 8: stable, zero inside the body before the projection's correction is added, out_vel 0
    on the very first sub-step (gdt = 0 then) and u_max dt / dx afterwards"""
    import cylinder_ref
    from x3d2_amd.ibm import cylinder_mask
    dims, L = (33, 16, 8), (20.0, 12.0, 6.0)
    ep1 = cylinder_mask(_mesh(dims, L), (5.0, 6.0), 1.3)
    assert (ep1 == 0).any()
    ref = cylinder_ref.CylinderRef(dims, L, time_intg="AB3", ep1=ep1)
    pert = cylinder_ref.smooth_perturbation(ref.mesh)
    ref.set_velocity(1.0 + pert[0], pert[1], pert[2])
    ref.step()
    assert ref.out_vel == 0.0
    for _ in range(2):
        ref.step()
    u, v, w = ref.velocity()
    assert np.all(np.isfinite(u)) and np.max(np.abs(u)) < 2.0
    assert abs(ref.out_vel - 0.0075 / (20.0 / 32)) < 0.2 * 0.012  # u_max ~ 1
