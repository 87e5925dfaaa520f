"""Energy spectra, host side (no GPU): the sampling schedule, the file and state round trips, the ABI names, and the numpy
checker of the GPU tests (tests/spectra_ref.py) against two facts that need no device."""
import os
import re

import numpy as np
import pytest

import spectra_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("x3d_spectra_create", "x3d_spectra_destroy", "x3d_spectra_sizes", "x3d_spectra_sample",
                "x3d_spectra_reduce", "x3d_spectra_accumulate", "x3d_spectra_read", "x3d_spectra_load")
TWOPI = 2.0 * np.pi


@pytest.mark.parametrize("initspec", [0, 1, 5])
@pytest.mark.parametrize("ispecfreq", [1, 3])
def test_sample_schedule_mirrors_the_statistics(initspec, ispecfreq):
    from x3d2_amd.spectra import SpectraConfig
    from x3d2_amd.stats import StatsConfig
    cfg = SpectraConfig(initspec=initspec, ispecfreq=ispecfreq, ispecout=4)
    st = StatsConfig(initstat=initspec, istatfreq=ispecfreq, istatout=4)
    assert cfg.active == (initspec > 0)
    for it in range(21):
        assert cfg.sample_due(it) == st.sample_due(it) == cfg.due(it), (initspec, ispecfreq, it)
        assert cfg.output_due(it) == st.output_due(it)


def test_config_checks():
    from x3d2_amd.common import X3dError
    from x3d2_amd.spectra import SpectraConfig
    assert SpectraConfig().fields == ("u", "v", "w") and not SpectraConfig().active
    assert SpectraConfig(fields=("u", "phi_2")).fields == ("u", "phi_2")
    for kw in (dict(mode="ring"), dict(ispecfreq=0), dict(dk=0.0), dict(dk=-1.0), dict(fields=()), dict(fields=("u", "u")),
               dict(fields=("p",)), dict(fields=("phi_0",))):
        with pytest.raises(X3dError):
            SpectraConfig(**kw)


def test_header_and_prototypes_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "x3d2_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    from x3d2_amd import _lib
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES


def _fake_raw(layout, nfields, seed):
    return np.random.default_rng(seed).random((nfields, layout.len))


@pytest.mark.parametrize("mode", ["shell", "plane"])
def test_file_round_trip_through_load_spectra(mode, tmp_path):
    from x3d2_amd import spectra as sp
    fields = ("u", "v", "w") if mode == "shell" else ("u", "w")
    lay = sp.Layout(mode, (40, 24, 12), (5.0, TWOPI, 3.0), y=np.linspace(0.0, 2.0, 24))
    inst, mean = lay.arrays(_fake_raw(lay, len(fields), 1), fields), lay.arrays(_fake_raw(lay, len(fields), 2), fields)
    prefix = str(tmp_path / "spectra")
    name = sp.save_spectra(prefix, 12, mode, fields, 7, inst, mean)
    assert name == prefix + "_000012.npz" and os.path.exists(name)
    back = sp.load_spectra(prefix, 12)
    assert back["mode"] == mode and back["fields"] == fields and back["sample_count"] == 7 and back["iteration"] == 12
    assert sorted(back["spectrum"]) == sorted(inst) and sorted(back["mean"]) == sorted(mean)
    for k in inst:
        assert np.array_equal(back["spectrum"][k], inst[k]), k
        assert np.array_equal(back["mean"][k], mean[k]), k
    if mode == "shell":
        assert lay.nbins == 16 and np.array_equal(inst["k"], np.arange(16) * lay.dk)
        assert np.array_equal(inst["E"], (inst["E_u"] + inst["E_v"]) + inst["E_w"])
    else:
        assert inst["Ex_u"].shape == (24, 21) and inst["Ez_w"].shape == (24, 7) and np.array_equal(inst["y"], np.linspace(0.0, 2.0, 24))


@pytest.mark.parametrize("mode", ["shell", "plane"])
def test_state_dict_round_trip(mode):
    from x3d2_amd import spectra as sp
    from x3d2_amd.common import X3dError
    fields = ("u", "v", "w", "phi_1")
    lay = sp.Layout(mode, (32, 17, 16), (4.0, 2.0, 2.0))
    raw = _fake_raw(lay, len(fields), 3)
    state = sp.state_from_mean(mode, fields, 5, lay.arrays(raw, fields))
    assert all(k.startswith("spectra_") for k in state)
    # (through a file, as a checkpoint carries it)
    import io
    buf = io.BytesIO()
    np.savez(buf, **state)
    buf.seek(0)
    z = dict(np.load(buf, allow_pickle=False))
    count, mean = sp.mean_from_state(z, mode, fields)
    assert count == 5
    assert np.array_equal(lay.raw(mean, fields), raw)
    with pytest.raises(X3dError, match="mode"):
        sp.mean_from_state(z, "plane" if mode == "shell" else "shell", fields)
    with pytest.raises(X3dError, match="fields"):
        sp.mean_from_state(z, mode, ("u", "v", "w"))


def test_checker_tgv_16_energy_sits_in_bin_2():
    """the Taylor-Green initial field on 16^3 in a 2 pi box: |k| = sqrt(3) for all of its modes, bin 2 holds the whole
    energy 1/8"""
    u, v, w = spectra_ref.tgv((16, 16, 16))
    E = sum(spectra_ref.shell(f, (TWOPI,) * 3) for f in (u, v, w))
    assert E.size == spectra_ref.nbins((16,) * 3, (TWOPI,) * 3, 1.0) == 15
    assert abs(E[2] - 0.125) <= 4e-16
    assert np.all(np.delete(E, 2) < 1e-32)
    assert abs(E.sum() - 0.125) <= 4e-16


@pytest.mark.parametrize("L,nb", [((5.0, TWOPI, 3.0), 16), ((3.0, TWOPI, 5.0), 22)])
def test_checker_parseval_on_three_distinct_dims_and_lengths(L, nb):
    """random u, v, w on 40 x 24 x 12 (nx, ny, nz) in the box (5, 2 pi, 3) of the GPU tests -- dk = 2 pi / 3, 16 bins -- and
    in the box with x and z exchanged -- 22 bins: no bin empty, sum E = 1/2 <u^2 + v^2 + w^2>; per y row the plane spectra
    both sum to that row's 1/2 <f^2>"""
    dims = (40, 24, 12)
    rng = np.random.default_rng(5)
    fs = [rng.standard_normal((dims[2], dims[1], dims[0])) for _ in range(3)]
    b, margin = spectra_ref.shell_bins(dims, L, spectra_ref.default_dk(L))
    assert margin > 1e-9 and b.max() == nb - 1
    E = sum(spectra_ref.shell(f, L) for f in fs)
    assert E.size == nb and np.all(E > 0.0)
    want = 0.5 * sum(float(np.mean(f * f)) for f in fs)
    assert abs(E.sum() - want) <= 4e-16 * 8 * want
    ex, ez = spectra_ref.plane(fs[0])
    row = 0.5 * np.mean(fs[0] * fs[0], axis=(0, 2))
    assert ex.shape == (24, 21) and ez.shape == (24, 7)
    assert np.max(np.abs(ex.sum(axis=1) - row)) <= 1e-14 * row.max()
    assert np.max(np.abs(ez.sum(axis=1) - row)) <= 1e-14 * row.max()


def test_host_layout_restates_the_checker():
    from x3d2_amd import spectra as sp
    for dims, L in (((16, 16, 16), (TWOPI,) * 3), ((40, 24, 12), (5.0, TWOPI, 3.0)), ((160, 8, 6), (TWOPI,) * 3)):
        lay = sp.Layout("shell", dims, L)
        assert lay.dk == spectra_ref.default_dk(L) and lay.nbins == spectra_ref.nbins(dims, L, lay.dk)
    assert sp.shell_nbins((16, 16, 16), (TWOPI,) * 3, 1e-3) > sp.MAXBINS
