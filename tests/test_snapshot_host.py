"""Host side of the snapshots (x3d2_amd/snapshot.py) against tests/snapshot_ref.py: which iterations are due, the field
list, the error cases, the output geometry under the global rule, and the VTK description.  No GPU."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import snapshot_ref

PER = ("periodic",) * 2


def _mesh(dims, nproc_dir=(1, 1, 1), rank=0, L=(1.0, 1.0, 1.0)):
    from x3d2_amd import Mesh
    return Mesh(tuple(dims), nproc_dir, L, PER, PER, PER, nrank=rank)


def test_due_follows_the_reference():
    from x3d2_amd.snapshot import SnapshotConfig
    for freq in (-1, 0, 1, 2, 5):
        cfg = SnapshotConfig(snapshot_freq=freq)
        for it in range(0, 12):
            assert cfg.due(it) == snapshot_ref.due(freq, it), (freq, it)
    assert not SnapshotConfig().due(4)  # the default never writes


def test_field_list_for_every_subset():
    from x3d2_amd.snapshot import SnapshotConfig, snapshot_fields
    for r in range(len(snapshot_ref.OUTPUT_FIELDS) + 1):
        for subset in itertools.combinations(snapshot_ref.OUTPUT_FIELDS, r):
            for order in (subset, subset[::-1]):  # the order of the request does not matter
                for nspecies in (0, 2):
                    got = snapshot_fields(SnapshotConfig(output_fields=order), nspecies)
                    assert got == snapshot_ref.field_names(subset, nspecies), (order, nspecies)
    assert snapshot_fields(SnapshotConfig(output_fields=snapshot_ref.OUTPUT_FIELDS), 2) == \
        ["u", "v", "w", "p", "vort", "qcrit", "ibm", "phi_1", "phi_2"]


def test_error_cases():
    from x3d2_amd.common import X3dError
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots
    with pytest.raises(X3dError, match="unknown output field"):
        SnapshotConfig(output_fields=("pressure", "enstrophy"))
    with pytest.raises(X3dError, match="output_stride"):
        SnapshotConfig(output_stride=(1, 0, 1))
    solver = SimpleNamespace(mesh=_mesh((8, 8, 8)), species=[], ibm=None, keep_pressure=False)
    with pytest.raises(X3dError, match="no transported species"):
        Snapshots(solver, SnapshotConfig(snapshot_freq=1, output_fields=("species",)))
    with pytest.raises(X3dError, match="no immersed boundary"):
        Snapshots(solver, SnapshotConfig(snapshot_freq=1, output_fields=("ibm",)))
    assert solver.keep_pressure is False
    snap = Snapshots(solver, SnapshotConfig(snapshot_freq=1, output_fields=("pressure",)))
    assert solver.keep_pressure is True and snap.names == ["u", "v", "w", "p"]
    assert Snapshots(solver, SnapshotConfig()).write(3) is False  # never due: nothing is touched (there is no backend)


GEOMETRY = [((17, 6, 5), (1, 1, 1), (2, 3, 2)), ((17, 6, 5), (1, 1, 1), (4, 1, 5)), ((20, 7, 9), (1, 1, 1), (32, 8, 16)),
            ((16, 12, 20), (1, 1, 2), (1, 2, 3)),   # z offset 10 is not a multiple of 3
            ((16, 12, 20), (1, 2, 2), (3, 4, 3)),   # y offset 6 is not a multiple of 4 either
            ((16, 12, 20), (1, 2, 2), (2, 3, 5)),   # offsets 6 and 10: multiples of the strides
            ((16, 12, 20), (1, 1, 2), (1, 1, 1))]


@pytest.mark.parametrize("dims,nproc_dir,stride", GEOMETRY)
def test_geometry_tiles_the_global_output_exactly_once(dims, nproc_dir, stride):
    from x3d2_amd.common import VERT
    from x3d2_amd.snapshot import output_geometry
    nproc = int(np.prod(nproc_dir))
    filled, shape0 = None, None
    glob = np.arange(dims[0] * dims[1] * dims[2]).reshape(dims[2], dims[1], dims[0])  # a field that names its points
    want = snapshot_ref.strided(glob, (0, 0, 0), stride)
    out = None
    for rank in range(nproc):
        m = _mesh(dims, nproc_dir, rank)
        shape, start, count, first = output_geometry(m.get_global_dims(VERT), m.n_offset, m.get_dims(VERT), stride)
        for d in range(3):
            ref = snapshot_ref.geometry_global_rule(dims[d], int(m.n_offset[d]), int(m.vert_dims[d]), stride[d])
            assert (shape[d], start[d], count[d], first[d]) == ref, (rank, d)
            assert first[d] == (-int(m.n_offset[d])) % stride[d]
            if int(m.n_offset[d]) % stride[d] == 0:  # then the reference's own formulas hold (:175-188)
                assert (shape[d], start[d], count[d]) == snapshot_ref.geometry_reference(
                    dims[d], int(m.n_offset[d]), int(m.vert_dims[d]), stride[d])
        if filled is None:
            shape0 = shape
            filled = np.zeros(shape[::-1], dtype=int)
            out = np.full(shape[::-1], -1)
        assert shape == shape0
        o = [int(v) for v in m.n_offset]
        n = [int(v) for v in m.vert_dims]
        local = glob[o[2]:o[2] + n[2], o[1]:o[1] + n[1], o[0]:o[0] + n[0]]
        piece = snapshot_ref.strided(local, first, stride)
        assert piece.shape == count[::-1]
        sl = tuple(slice(start[d], start[d] + count[d]) for d in (2, 1, 0))
        filled[sl] += 1
        out[sl] = piece
    assert np.all(filled == 1)
    assert np.array_equal(out, want)  # a uniform grid: the global field at the multiples of the stride


def test_rank_one_of_the_two_rank_case_starts_at_local_plane_two():
    from x3d2_amd.common import VERT
    from x3d2_amd.snapshot import output_geometry
    m = _mesh((16, 12, 20), (1, 1, 2), 1)
    shape, start, count, first = output_geometry(m.get_global_dims(VERT), m.n_offset, m.get_dims(VERT), (1, 2, 3))
    assert (shape, start, count, first) == ((16, 6, 7), (0, 0, 4), (16, 6, 3), (0, 0, 2))


def test_vtk_xml_of_one_worked_case():
    """32 x 16 x 8 vertices on a 4 x 2 x 1 periodic box (d = 1/8 everywhere), stride (2, 1, 4): 16 x 16 x 2 output points,
    spacing (1/4, 1/8, 1/2); the literal is written from reading generate_vtk_xml (:245-285): extents in z, y, x order,
    a blank after WholeExtent's quote, G0 reals, the TIME array indented by eight"""
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots
    solver = SimpleNamespace(mesh=_mesh((32, 16, 8), L=(4.0, 2.0, 1.0)), species=[], ibm=None, keep_pressure=False)
    snap = Snapshots(solver, SnapshotConfig(snapshot_freq=2, output_stride=(2, 1, 4),
                                            output_fields=("qcriterion", "pressure", "vorticity")))
    literal = """<?xml version="1.0"?>
<VTKFile type="ImageData" version="0.1">
  <ImageData WholeExtent=" 0 1 0 15 0 15" Origin="0.0000000000000000 0.0000000000000000 0.0000000000000000" Spacing="0.25000000000000000 0.12500000000000000 0.50000000000000000">
    <Piece Extent="0 1 0 15 0 15">
      <PointData>
      <DataArray Name="u">u</DataArray>
      <DataArray Name="v">v</DataArray>
      <DataArray Name="w">w</DataArray>
      <DataArray Name="p">p</DataArray>
      <DataArray Name="vort">vort</DataArray>
      <DataArray Name="qcrit">qcrit</DataArray>
        <DataArray Name="TIME">time</DataArray>
      </PointData>
    </Piece>
  </ImageData>
</VTKFile>"""
    assert snap.shape == (16, 16, 2) and snap.spacing == (0.25, 0.125, 0.5) and snap.origin == (0.0, 0.0, 0.0)
    assert snap.vtk_xml == literal
    assert literal == snapshot_ref.vtk_xml((16, 16, 2), snap.names, "0.0000000000000000 " * 2 + "0.0000000000000000",
                                           "0.25000000000000000 0.12500000000000000 0.50000000000000000")
