"""Host side of the diagnostics series (x3d2_amd/diagnostics.py) and the numpy restatement the GPU tests compare against
(tests/diagnostics_ref.py), pinned to closed forms.  No GPU."""
import math
import os

import numpy as np
import pytest

import diagnostics_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2


def channel_mesh(nproc_dir=(1, 1, 1), rank=0):
    from x3d2_amd import Mesh
    return Mesh((32, 17, 16), nproc_dir, (4.0, 2.0, 2.0), PER, WALL, PER, ("uniform", "top-bottom", "uniform"),
                (1.0, 0.259065151, 1.0), nrank=rank)


# ---------------------------------------------------------------- the restatement against closed forms
def test_restatement_on_the_taylor_green_initial_field():
    n, nu, dt = 16, 1.0 / 1600.0, 1e-3
    u, v, w, grads = ref.tgv_fields(n)
    ih = [np.full(n, n / (2.0 * math.pi))] * 3
    r = ref.row(u, v, w, grads, ih, (False, False))
    d = ref.derive(r, n ** 3, n ** 3, n * n, nu, dt, divergence=False)
    assert abs(d["ke"] - 0.125) <= 1e-14
    assert abs(d["enstrophy"] - 0.375) <= 1e-14
    # periodic and solenoidal: <S_ij S_ij> = 1/2 <|curl u|^2>
    assert abs(d["dissipation"] - 2.0 * nu * d["enstrophy"]) <= 1e-14 * 2.0 * nu * d["enstrophy"]
    assert r[5] == r[6] == r[7] == r[13] == r[14] == r[15] == 0.0
    assert abs(d["u_max"] - 1.0) <= 1e-15 and abs(d["v_max"] - 1.0) <= 1e-15 and d["w_max"] == 0.0
    # |u| / h + |v| / h <= sqrt(2) / h, reached where |sin x cos y| = |cos x sin y| ... on the grid: at most that
    assert d["cfl"] <= dt * math.sqrt(2.0) * n / (2.0 * math.pi) * (1 + 1e-15) and d["cfl"] >= dt * n / (2.0 * math.pi)
    # the product's own formulas give the same columns
    from x3d2_amd import diagnostics as dg
    got = dg.derive(r, n ** 3, n ** 3, n * n, nu, dt, divergence=False)
    assert dg.column_names(False, False) == ref.column_names(False, False)
    assert got == [d[c] for c in ref.column_names(False, False)]


def test_restatement_finds_a_single_maximum_and_the_wall_rows():
    shape = (4, 5, 6)  # [nz, ny, nx]
    zero = np.zeros(shape)
    ih = (np.arange(1.0, 7.0), np.arange(1.0, 6.0) * 10.0, np.arange(1.0, 5.0) * 100.0)
    v = zero.copy()
    v[2, 3, 4] = -3.0
    r = ref.row(zero, v, zero, [zero] * 9, ih, (True, True))
    assert r[1] == 9.0 and r[9] == 3.0 and r[12] == 3.0 * 40.0
    assert not np.any(np.delete(r, [1, 9, 12]))
    uy = zero.copy()
    uy[1, 0, 2], uy[3, 4, 5], uy[2, 2, 2] = 2.0, -5.0, 7.0
    g = [zero] * 9
    g[1] = uy
    r = ref.row(zero, zero, zero, g, ih, (True, True))
    assert r[5] == 2.0 and r[6] == -5.0 and r[3] == 4.0 + 25.0 + 49.0 and r[4] == 0.5 * r[3] and r[11] == 49.0
    r = ref.row(zero, zero, zero, g, ih, (False, True))
    assert r[5] == 0.0 and r[6] == -5.0
    d = ref.derive(r, 120, 60, 24, 0.5, 0.1, divergence=False, y_walls=True)
    assert d["tau_w_lo"] == 0.0 and d["tau_w_hi"] == 0.5 * 5.0 / 24 and d["vort_max"] == 7.0


# ---------------------------------------------------------------- the file
def test_a_row_written_and_parsed_back(tmp_path):
    from x3d2_amd import diagnostics as dg
    cols = dg.column_names(True, True)
    vals = [0.125, 0.375, 4.6875e-4, 1.0, 1.0, 0.0, 3.0e-101, 1.5e100, 6.786132408593e-15, 7.4e-16, -2.5, 2.5]
    assert len(vals) == len(cols)
    path = str(tmp_path / "series.csv")
    with open(path, "w") as fh:
        fh.write(dg.format_header(cols))
        fh.write(dg.format_row(0.001, vals))
    assert dg.format_header(cols) == ref.format_header(cols) and dg.format_row(0.001, vals) == ref.format_row(0.001, vals)
    text = open(path).read().splitlines()
    assert text[0] == "# time, " + ", ".join(cols)
    assert all(len(f) == 20 for f in text[1].split(",")[:7])  # ES20.12: twenty characters per value
    assert "3.000000000000E-101" in text[1]  # (a three-digit exponent the way Python writes it)
    got_cols, rows = dg.parse_csv(path)
    assert got_cols == cols and rows.shape == (1, 1 + len(cols))
    want = np.array([float("%.12E" % v) for v in [0.001] + vals])
    assert np.array_equal(rows[0], want)


def test_the_reference_line_at_t0_is_reproduced_character_for_character():
    from x3d2_amd import diagnostics as dg
    path = os.path.join(HERE, "golden", "ref_tgv32_rk3_nopoisson.csv")
    lines = open(path).read().splitlines()
    header = [l for l in lines if l.startswith("# time")][0]
    data = [l for l in lines if not l.startswith("#")]
    cols = tuple(c.strip() for c in header[1:].split(",")[1:])
    assert dg.format_header(cols) == header + "\n"
    vals = [float(v) for v in data[0].split(",")]
    assert vals[0] == 0.0
    assert dg.format_row(vals[0], vals[1:]) == data[0] + "\n"
    for line in data:  # (and every other line of the fixture)
        vals = [float(v) for v in line.split(",")]
        assert dg.format_row(vals[0], vals[1:]) == line + "\n"


def test_append_keeps_the_rows_up_to_the_restart_time(tmp_path):
    from x3d2_amd import diagnostics as dg
    from x3d2_amd.common import X3dError
    cols = dg.column_names(False, False)
    path = str(tmp_path / "series.csv")
    dt = 1e-3
    with open(path, "w") as fh:
        fh.write(dg.format_header(cols))
        for it in range(1, 7):
            fh.write(dg.format_row(it * dt, [float(it)] * len(cols)))
    before = open(path).read().splitlines(True)
    assert dg.trim_csv(path, 4 * dt, cols) == 4
    after = open(path).read().splitlines(True)
    assert after == before[:5]
    assert dg.trim_csv(path, 4 * dt, cols) == 4 and open(path).read().splitlines(True) == after  # (idempotent)
    assert dg.trim_csv(path, 0.0, cols) == 0 and open(path).read() == dg.format_header(cols)
    with pytest.raises(X3dError, match="columns"):
        dg.trim_csv(path, 1.0, dg.column_names(True, False))


def test_sample_due():
    from x3d2_amd.common import X3dError
    from x3d2_amd.diagnostics import DiagnosticsConfig
    c = DiagnosticsConfig()
    assert (c.initdiag, c.idiagfreq, c.prefix, c.flush_every, c.divergence) == (1, 1, "diagnostics", 256, True)
    assert not c.sample_due(0) and all(c.sample_due(it) for it in range(1, 6))
    c = DiagnosticsConfig(initdiag=3, idiagfreq=4)
    assert [it for it in range(0, 16) if c.sample_due(it)] == [3, 7, 11, 15]
    assert not any(DiagnosticsConfig(initdiag=0).sample_due(it) for it in range(0, 10))
    for bad in (dict(idiagfreq=0), dict(flush_every=0)):
        with pytest.raises(X3dError):
            DiagnosticsConfig(**bad)


def test_column_set():
    from x3d2_amd.diagnostics import column_names
    base = ("ke", "enstrophy", "dissipation", "u_max", "v_max", "w_max", "vort_max", "cfl")
    assert column_names(False, False) == base
    assert column_names(True, False) == base + ("div_u_max", "div_u_mean")
    assert column_names(False, True) == base + ("tau_w_lo", "tau_w_hi")
    assert column_names(True, True) == base + ("div_u_max", "div_u_mean", "tau_w_lo", "tau_w_hi")
    for d in (False, True):
        for w in (False, True):
            assert column_names(d, w) == ref.column_names(d, w)


# ---------------------------------------------------------------- spacing tables
def test_spacing_tables_on_the_channel_mesh():
    from x3d2_amd.diagnostics import inverse_spacing, spacing_tables
    m = channel_mesh()
    ihx, ihy, ihz = spacing_tables(m)
    assert ihx.shape == (32,) and ihy.shape == (17,) and ihz.shape == (16,)
    assert np.all(ihx == 1.0 / (4.0 / 32)) and np.all(ihz == 1.0 / (2.0 / 16))
    y = np.asarray(m.vert_coords[1], dtype=np.float64)
    assert np.all(ihy > 0.0)
    assert np.max(np.abs(ihy - ihy[::-1]) / ihy) <= 1e-12  # symmetric about the centre plane
    assert ihy[0] == 1.0 / (y[1] - y[0]) and ihy[-1] == 1.0 / (y[-1] - y[-2])  # one-sided at the walls
    assert ihy[8] == 1.0 / (0.5 * (y[9] - y[7]))
    assert ihy[0] > ihy[8]  # (stretched towards the walls)
    assert np.array_equal(ihy, ref.inverse_spacing(y, False, 2.0))
    # a periodic direction wraps around
    c = np.array([0.0, 0.1, 0.3, 0.6])
    assert np.allclose(inverse_spacing(c, True, 1.0), 1.0 / np.array([0.25, 0.15, 0.25, 0.35]), rtol=1e-15)
    assert np.array_equal(inverse_spacing(c, True, 1.0), ref.inverse_spacing(c, True, 1.0))


def test_spacing_tables_of_two_z_slabs_are_slices_of_the_whole():
    from x3d2_amd.diagnostics import spacing_tables
    whole = spacing_tables(channel_mesh())
    for rank in (0, 1):
        ihx, ihy, ihz = spacing_tables(channel_mesh((1, 1, 2), rank))
        assert np.array_equal(ihx, whole[0]) and np.array_equal(ihy, whole[1])
        assert np.array_equal(ihz, whole[2][8 * rank:8 * rank + 8])
