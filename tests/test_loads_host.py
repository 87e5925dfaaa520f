"""Host side of the loads and probes series (x3d2_amd/loads.py, x3d2_amd/probes.py) against the numpy restatement
(tests/loads_ref.py) and closed forms.  No GPU."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import loads_ref as ref

PER, WALL = ("periodic",) * 2, ("dirichlet",) * 2


def channel_mesh(nproc_dir=(1, 1, 1), rank=0):
    from x3d2_amd import Mesh
    return Mesh((32, 17, 16), nproc_dir, (4.0, 2.0, 2.0), PER, WALL, PER, ("uniform", "top-bottom", "uniform"),
                (1.0, 0.259065151, 1.0), nrank=rank)


# ---------------------------------------------------------------- nearest vertex
def test_nearest_vertex_on_a_uniform_axis_with_ties_and_ends():
    from x3d2_amd.probes import nearest_vertex
    c = np.arange(9) * 0.25  # (quarters: midpoints are exact, so a tie IS a tie)
    x = np.array([0.0, 0.1, 0.125, 0.13, 0.375, 1.0, 1.874, 1.875, 1.876, 2.0])
    got = nearest_vertex(c, x)
    assert list(got) == [0, 0, 0, 1, 1, 4, 7, 7, 8, 8]
    assert list(got) == [ref.nearest_vertex(c, v) for v in x]
    # periodic, length 2.25: vertex 0's image lies at 2.25; 2.125 is the tie between the last vertex and that image
    xp = np.array([2.0, 2.1, 2.125, 2.13, 2.25, 0.0])
    gotp = nearest_vertex(c, xp, True, 2.25)
    assert list(gotp) == [8, 8, 0, 0, 0, 0]
    assert list(gotp) == [ref.nearest_vertex(c, v, True, 2.25) for v in xp]


def test_nearest_vertex_on_a_stretched_axis():
    from x3d2_amd.probes import nearest_vertex, snap
    m = channel_mesh()
    y = np.asarray(m.vert_coords[1], dtype=np.float64)
    assert np.ptp(np.diff(y)) > 0.01  # (stretched indeed)
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.uniform(y[0], y[-1], 200), y, [y[0], y[-1]], 0.5 * (y[3:5].sum()) * np.ones(1)])
    got = nearest_vertex(y, x)
    assert list(got) == [ref.nearest_vertex(y, float(v)) for v in x]
    assert list(got[200:200 + y.size]) == list(range(y.size))  # a vertex snaps to itself
    # the index space midpoint is NOT the rule: a point just above the coordinate midpoint of two unequal cells
    j = 1
    mid = 0.5 * (y[j] + y[j + 1])
    assert nearest_vertex(y, [mid - 1e-9])[0] == j and nearest_vertex(y, [mid + 1e-9])[0] == j + 1
    ijk, xyz = snap(m, [[0.0, 0.0, 0.0], [3.99, 2.0, 1.99], [1.0 + 0.0625, y[5] + 1e-6, 0.51]])
    assert ijk.tolist() == [[0, 0, 0], [0, 16, 0], [8, 5, 4]]  # (x: the tie 8 | 9 goes down; 3.99 and 1.99 wrap to vertex 0)
    assert xyz[2].tolist() == [1.0, float(y[5]), 0.5]


def test_snap_uses_the_global_coordinates_on_every_rank():
    from x3d2_amd.probes import snap
    pts = [[1.3, 0.7, 0.3], [2.0, 1.9, 1.7]]
    whole = snap(channel_mesh(), pts)
    for rank in range(2):
        part = snap(channel_mesh((1, 1, 2), rank), pts)
        assert np.array_equal(part[0], whole[0]) and np.array_equal(part[1], whole[1])


def test_a_probe_outside_the_domain_and_bad_point_lists_are_errors():
    from x3d2_amd.common import X3dError
    from x3d2_amd.probes import ProbesConfig, snap
    m = channel_mesh()
    for bad in ([-1e-9, 1.0, 1.0], [4.0 + 1e-9, 1.0, 1.0], [1.0, 2.0 + 1e-9, 1.0], [1.0, -1e-9, 1.0], [1.0, 1.0, 2.5]):
        with pytest.raises(X3dError):
            snap(m, [bad])
    snap(m, [[4.0, 2.0, 2.0]])  # the domain's far corner is inside
    for bad in ([], [[1.0, 2.0]], np.zeros((4097, 3)), [[1.0, float("nan"), 0.0]]):
        with pytest.raises(X3dError):
            ProbesConfig(bad)
    assert ProbesConfig(np.zeros((4096, 3))).points.shape == (4096, 3)
    with pytest.raises(X3dError):
        ProbesConfig([[0.0, 0.0, 0.0]], iprobefreq=0)
    with pytest.raises(X3dError):
        ProbesConfig([[0.0, 0.0, 0.0]], flush_every=0)


# ---------------------------------------------------------------- weights and the restatement
def test_weights_sum_to_the_domain_and_the_restatement_meets_a_closed_form():
    from x3d2_amd import loads
    m = channel_mesh()
    w = loads.weights(m)
    for d, (a, c) in enumerate(zip(w, ref.weights(m))):  # the product's tables against the coordinates themselves
        print("weights", d, float(np.max(np.abs(a - c))), ref.weights_tolerance(m, d))
        assert a.shape == c.shape and float(np.max(np.abs(a - c))) <= ref.weights_tolerance(m, d)
    for rank in range(2):  # every rank holds its slice of the global tables
        part, lo = channel_mesh((1, 1, 2), rank), 8 * rank
        for d, (a, c) in enumerate(zip(loads.weights(part), w)):
            assert np.array_equal(a, c[lo:lo + 8] if d == 2 else c)
    assert abs(w[0].sum() - 4.0) <= 1e-14 * 4.0 and abs(w[2].sum() - 2.0) <= 1e-14 * 2.0  # periodic: the period
    y = np.asarray(m.vert_coords[1])
    # walls: one-sided first and last weight, centred in between -- the sum telescopes to this
    assert abs(w[1].sum() - (1.5 * (y[1] - y[0]) + 1.5 * (y[-1] - y[-2]) + (y[-2] - y[1]))) <= 1e-14
    ep1 = np.ones((16, 17, 32))
    ep1[2:5, 3:9, 10:20] = 0.0
    ep1[7, 7, 7] = 0.25
    u = np.full(ep1.shape, 2.0)
    row, mag = ref.impulse(ep1, u, -u, 0.0 * u, w)
    vol = w[0][10:20].sum() * w[1][3:9].sum() * w[2][2:5].sum() + 0.75 * w[0][7] * w[1][7] * w[2][7]
    assert abs(row[0] - 2.0 * vol) <= 1e-14 * 2.0 * vol and row[1] == -row[0] and row[2] == 0.0 and mag[0] == row[0]
    assert abs(ref.masked_volume(ep1, w) - vol) <= 1e-14 * vol


# ---------------------------------------------------------------- the file
def test_csv_header_round_trip_and_trim(tmp_path):
    from x3d2_amd import loads, probes
    from x3d2_amd.diagnostics import format_header, format_row, parse_csv, trim_csv
    assert format_header(loads.COLUMNS) == "# time, fx, fy, fz, cx, cy, cz\n"
    cols = probes.column_names(2)
    assert format_header(cols) == "# time, u_0, v_0, w_0, u_1, v_1, w_1\n"
    ijk = np.array([[0, 4, 2], [31, 16, 15]])
    xyz = np.array([[0.0, 0.1234567890123456, 0.25], [3.875, 2.0, 1.875]])
    comments = probes.header_comments(ijk, xyz)
    assert comments[1] == "# probe 1: vertex 32 17 16 at 3.875 2 1.875\n"
    assert float(comments[0].split()[-2]) == xyz[0, 1]  # (17 digits: the coordinate's own bits)
    path = str(tmp_path / "probes.csv")
    rng = np.random.default_rng(8)
    data = rng.standard_normal((5, 6)) * 10.0 ** rng.integers(-30, 30, (5, 6))
    dt = 0.0075
    with open(path, "w") as fh:
        fh.write(format_header(cols))
        fh.writelines(comments)
        for r in range(5):
            fh.write(format_row((r + 1) * dt, data[r]))
    got_cols, arr = parse_csv(path)
    assert got_cols == cols and arr.shape == (5, 7)
    assert np.allclose(arr[:, 1:], data, rtol=1e-12, atol=0.0) and np.allclose(arr[:, 0], dt * np.arange(1, 6), rtol=1e-12)
    assert trim_csv(path, 3 * dt, cols) == 3
    lines = open(path).read().splitlines(True)
    assert lines[0] == format_header(cols) and lines[1:3] == comments and len(lines) == 6
    assert parse_csv(path)[1].shape == (3, 7)
    from x3d2_amd.common import X3dError
    with pytest.raises(X3dError):
        trim_csv(path, dt, loads.COLUMNS)  # another series' file


# ---------------------------------------------------------------- Strouhal number
def test_strouhal_of_a_sine_with_a_mean_lies_within_half_a_bin():
    from x3d2_amd import loads
    n, dt, d, u0 = 4096, 0.0075, 1.0, 1.0
    t = dt * np.arange(1, n + 1)
    for f in (0.2, 0.2137, 1.0 / 3.0, 3.21):
        assert abs(f * n * dt - round(f * n * dt)) > 0.05  # (a non-integer number of periods)
        y = 1.3 + 0.4 * np.sin(2.0 * math.pi * f * t + 0.3)
        st = loads.strouhal(t, y, d, u0)
        print("strouhal", f, st, "half bin", 0.5 / (n * dt))
        assert abs(st - f) <= 0.5 / (n * dt)
        assert abs(loads.strouhal(t, y, 2.0, 4.0) - 0.5 * st) <= 1e-15
    y = 1.3 + 0.4 * np.sin(2.0 * math.pi * 0.2137 * t + 0.3)
    assert abs(loads.strouhal(t, y, d, u0) - ref.strouhal(t, y, d, u0)) <= 1e-9
    # the mean is removed: an offset a thousand times the amplitude changes nothing that matters
    assert abs(loads.strouhal(t, y + 400.0, d, u0) - 0.2137) <= 0.5 / (n * dt)


def test_strouhal_rejects_short_and_non_uniform_series():
    from x3d2_amd import loads
    from x3d2_amd.common import X3dError
    t = 0.1 * np.arange(8)
    y = np.sin(t)
    loads.strouhal(t, y, 1.0, 1.0)
    with pytest.raises(X3dError):
        loads.strouhal(t[:7], y[:7], 1.0, 1.0)
    bent = t.copy()
    bent[5] += 0.01
    with pytest.raises(X3dError):
        loads.strouhal(bent, y, 1.0, 1.0)
    with pytest.raises(X3dError):
        loads.strouhal(t, y[:7], 1.0, 1.0)
    with pytest.raises(X3dError):
        loads.strouhal(t[::-1], y, 1.0, 1.0)
    with pytest.raises(X3dError):
        loads.strouhal(t, np.full(8, 2.5), 1.0, 1.0)  # no variance: there is no peak to name


# ---------------------------------------------------------------- configuration errors that need no device
def test_loads_configuration_errors():
    from x3d2_amd.common import X3dError
    from x3d2_amd.loads import Loads, LoadsConfig
    for kw in (dict(iloadfreq=0), dict(flush_every=0), dict(u_ref=0.0), dict(area_ref=0.0)):
        with pytest.raises(X3dError):
            LoadsConfig(**kw)
    cfg = LoadsConfig()
    assert (cfg.initload, cfg.iloadfreq, cfg.prefix, cfg.flush_every, cfg.u_ref, cfg.area_ref) == (1, 1, "loads", 256, 1.0, None)
    assert [it for it in range(1, 8) if LoadsConfig(initload=2, iloadfreq=2).sample_due(it)] == [2, 4, 6]
    assert not any(LoadsConfig(initload=0).sample_due(it) for it in range(0, 8))
    sparse = SimpleNamespace(iibm=1, h=object(), area_ref=None)
    for ibm in (None, SimpleNamespace(iibm=0, h=None, area_ref=6.0), SimpleNamespace(iibm=1, h=None, area_ref=6.0), sparse):
        with pytest.raises(X3dError):  # no mask; a mask that is off; the dense form; no reference area from anywhere
            Loads(SimpleNamespace(ibm=ibm), cfg)
    assert getattr(sparse, "loads", None) is None  # (a refused Loads attaches nothing)
