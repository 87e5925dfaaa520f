"""numpy restatement of what the snapshot tests cite from the reference (src/io/snapshot_manager.f90,
src/io/io_field_utils.f90, src/backend/omp/backend.f90:616-649); nothing here imports x3d2_amd."""
import numpy as np

OUTPUT_FIELDS = ("pressure", "vorticity", "qcriterion", "ibm", "species")


def due(snapshot_freq, it):
    """snapshot_manager.f90:125-126"""
    return snapshot_freq > 0 and it % snapshot_freq == 0


def field_names(output_fields, nspecies):
    """get_snapshot_fields, :198-243"""
    names = ["u", "v", "w"]
    for key, name in (("pressure", "p"), ("vorticity", "vort"), ("qcriterion", "qcrit"), ("ibm", "ibm")):
        if key in output_fields:
            names.append(name)
    if "species" in output_fields:
        names += ["phi_%d" % i for i in range(1, nspecies + 1)]
    return names


def geometry_global_rule(n_global, offset, n_local, stride):
    """one direction, by enumeration: the kept points are the global indices 0, s, 2 s, ...; returns (shape, start,
    count, first) of the rank that owns [offset, offset + n_local)"""
    kept = [g for g in range(n_global) if g % stride == 0]
    mine = [g for g in kept if offset <= g < offset + n_local]
    if not mine:
        return len(kept), 0, 0, 0
    return len(kept), kept.index(mine[0]), len(mine), mine[0] - offset


def geometry_reference(n_global, offset, n_local, stride):
    """get_output_dimensions, io_field_utils.f90:155-188, one direction: (shape, start, count)"""
    return (n_global + stride - 1) // stride, offset // stride, (n_local + stride - 1) // stride


def strided(a, first, stride):
    """a[nz, ny, nx] at the kept points; first, stride in (x, y, z) order"""
    return a[first[2]::stride[2], first[1]::stride[1], first[0]::stride[0]]


def vorticity(g):
    """src/backend/omp/backend.f90:616-630; g = dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz"""
    dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz = g
    return np.sqrt((dwdy - dvdz) ** 2 + (dudz - dwdx) ** 2 + (dvdx - dudy) ** 2)


def qcriterion(g):
    """:632-649"""
    dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz = g
    return -0.5 * (dudx ** 2 + dvdy ** 2 + dwdz ** 2) - dudy * dvdx - dudz * dwdx - dvdz * dwdy


def q_scale(g):
    """the magnitude the Q bound is relative to: 1/2 (a11^2 + a22^2 + a33^2) + |a12 a21| + |a13 a31| + |a23 a32|"""
    dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz = g
    return 0.5 * (dudx ** 2 + dvdy ** 2 + dwdz ** 2) + np.abs(dudy * dvdx) + np.abs(dudz * dwdx) + np.abs(dvdz * dwdy)


def vtk_xml(dims, names, origin_str, spacing_str):
    """generate_vtk_xml, :245-285; dims (x, y, z), the two triples already formatted"""
    ext = "0 %d 0 %d 0 %d" % (dims[2] - 1, dims[1] - 1, dims[0] - 1)
    lines = ['<?xml version="1.0"?>', '<VTKFile type="ImageData" version="0.1">',
             '  <ImageData WholeExtent=" %s" Origin="%s" Spacing="%s">' % (ext, origin_str, spacing_str),
             '    <Piece Extent="%s">' % ext, "      <PointData>"]
    lines += ['      <DataArray Name="%s">%s</DataArray>' % (n, n) for n in names]
    lines += ['        <DataArray Name="TIME">time</DataArray>', "      </PointData>", "    </Piece>", "  </ImageData>",
              "</VTKFile>"]
    return "\n".join(lines)
