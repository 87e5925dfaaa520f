"""The X3D_* environment switches are declared in two tables -- csrc/switches.hip (the library's, resolved once per
x3d_backend) and x3d2_amd/switches.py (the driver's, one snapshot per owner) -- and nothing else reads the environment.
Host checks: no GPU is needed (x3d_backend_switch(NULL, ...) resolves against the environment without a device)."""
import ctypes
import os
import re

import pytest

from util import library_switch_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "x3d2_amd")
CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "x3d2_hip.h")
TABLE_FILE = "switches.hip"
TOKEN = re.compile(r"X3D_[A-Z0-9_]+")


def read(path):
    with open(path) as fh:
        return fh.read()


def library_names():
    """the names of the table in csrc/switches.hip (each is then asked of the library itself, test_library_*)"""
    return library_switch_names()


def driver_table():
    from x3d2_amd import switches
    return switches.TABLE


def driver_names():
    return [row[0] for row in driver_table()]


def switch(lib, name):
    v = ctypes.c_long(-12345)
    rc = lib.x3d_backend_switch(None, name.encode(), ctypes.byref(v))
    assert rc == 0, lib.x3d_last_error().decode()
    return v.value


@pytest.fixture(scope="module")
def lib():
    from x3d2_amd import _lib
    return _lib.load()


@pytest.fixture
def clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("X3D_"):
            monkeypatch.delenv(k)
    return monkeypatch


# ---------------------------------------------------------------- 1, 2: who reads the environment
def test_library_reads_the_environment_in_the_table_file_only():
    hits = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            for n, line in enumerate(read(os.path.join(CSRC, f)).splitlines(), 1):
                if "getenv(" in line:
                    hits.append((f, n, line.strip()))
    outside = [h for h in hits if h[0] != TABLE_FILE]
    assert [h[0] for h in outside] == ["prof.hip"] and 'getenv("X3D_ROCTX")' in outside[0][2], outside
    assert len([h for h in hits if h[0] == TABLE_FILE]) == 1, hits  # the one getenv of the table file


def test_driver_reads_the_environment_in_switches_py_only():
    pat = re.compile(r"\benviron\b|getenv")
    hits = sorted(f for f in os.listdir(PKG) if f.endswith(".py") and pat.search(read(os.path.join(PKG, f))))
    assert hits == ["_lib.py", "switches.py"], hits
    # ... and _lib.py for X3D_SINGLE_PREC alone, which the table declares as read at import
    assert set(TOKEN.findall(" ".join(l for l in read(os.path.join(PKG, "_lib.py")).splitlines() if pat.search(l)))) \
        == {"X3D_SINGLE_PREC"}
    kinds = {row[0]: row[1] for row in driver_table()}
    assert kinds["X3D_SINGLE_PREC"] == "import"


# ---------------------------------------------------------------- 3: every name is declared, once
def compile_time_names():
    """what the sources #define and what the public header's enums declare: not switches"""
    names = set()
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".hip", ".h")):
                names.update(re.findall(r"^\s*#\s*define\s+(X3D_[A-Z0-9_]+)", read(os.path.join(d, f)), flags=re.M))
    hdr = re.sub(r"/\*.*?\*/", "", read(HEADER), flags=re.S)
    names.update(re.findall(r"^\s*#\s*define\s+(X3D_[A-Z0-9_]+)", hdr, flags=re.M))
    for body in re.findall(r"enum\s*\{(.*?)\}", hdr, flags=re.S):
        names.update(TOKEN.findall(body))
    names.add("X3D_SINGLE_PREC")  # -DX3D_SINGLE_PREC of the Makefile (and, as a variable, the driver table's import-time entry)
    return names


def test_every_name_in_the_package_is_declared_in_exactly_one_table():
    lib_names, drv_names = library_names(), driver_names()
    assert len(set(lib_names)) == len(lib_names) and len(set(drv_names)) == len(drv_names)
    assert not set(lib_names) & set(drv_names), set(lib_names) & set(drv_names)
    declared = set(lib_names) | set(drv_names)
    macros = compile_time_names()
    assert not (declared - {"X3D_SINGLE_PREC"}) & macros
    unknown = {}
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".h", "Makefile")):
                for tok in TOKEN.findall(read(os.path.join(d, f))):
                    if tok in declared or tok in macros or tok == "X3D_ROCTX" or tok.startswith("X3D_SHIM_"):
                        continue
                    if tok.endswith("_") and any(m.startswith(tok) for m in macros):  # (a family by its prefix: X3D_K_*)
                        continue
                    unknown.setdefault(tok, f)
    assert not unknown, unknown


# ---------------------------------------------------------------- 4: the README's table
def test_readme_table_lists_exactly_the_declared_names():
    txt = read(os.path.join(ROOT, "README.md"))
    sec = txt[txt.index("\n## Switches"):]
    sec = sec[sec.index("\n| switch | owner | default | meaning |"):]
    rows = [l for l in sec[:sec.index("\n\n")].splitlines() if l.startswith("| `X3D_")]  # (the first table of the section)
    names = [TOKEN.match(l[3:]).group(0) for l in rows]
    owners = {n: l.split("|")[2].strip() for n, l in zip(names, rows)}
    assert len(set(names)) == len(names)
    assert set(names) == set(library_names()) | set(driver_names())
    assert {n for n, o in owners.items() if o == "library"} == set(library_names())
    assert {n for n, o in owners.items() if o == "driver"} == set(driver_names())


# ---------------------------------------------------------------- 5: the library's parsing
FLAG_VALUES = [(None, 0), ("1", 1), ("0", 0), ("", 0), ("10", 1)]  # the first character decides
SPECIAL = {
    "X3D_PAD_X": [(None, -2 ** 31), ("0", 0), ("48", 48)],  # unset is not 0: the backend's own rule (X3D_SW_UNSET)
    "X3D_SLAB_Z_SPLIT": [(None, -1), ("2", 2), ("0", 0)],
    "X3D_LAZY_RULES": [(None, 0xffffffff), ("249", 249), ("0x2f9", 0x2f9), ("0", 0)],
    "X3D_Y010_FORM": [(None, 1), ("", 1), ("split", 0), ("staged", 1), ("st", 1), ("1", 0)],  # compiled default: staged
}


def test_library_table_has_the_special_kinds():
    assert set(SPECIAL) <= set(library_names())


@pytest.mark.parametrize("name", library_names())
def test_library_switch_values(lib, clean_env, name):
    for value, want in SPECIAL.get(name, FLAG_VALUES):
        if value is None:
            clean_env.delenv(name, raising=False)
        else:
            clean_env.setenv(name, value)
        assert switch(lib, name) == want, (name, value)


def test_library_refuses_an_unknown_name(lib, clean_env):
    v = ctypes.c_long(7)
    for name in ("X3D_NO_SUCH_SWITCH", "X3D_NO_DEFER", "X3D_ROCTX", ""):  # (a driver's name is not the library's)
        assert lib.x3d_backend_switch(None, name.encode(), ctypes.byref(v)) != 0
        assert name in lib.x3d_last_error().decode() and "not a switch" in lib.x3d_last_error().decode()
        assert v.value == 7
    assert lib.x3d_backend_switch(None, None, ctypes.byref(v)) != 0
    assert lib.x3d_backend_switch(None, b"X3D_NO_CIRC", None) != 0


# ---------------------------------------------------------------- 6: the driver's snapshot
def driver_cases(kind, default):
    if kind == "flag":  # the driver's flags are on for exactly "1"
        return [(None, False), ("1", True), ("0", False), ("", False), ("10", False)]
    if kind == "int":
        return [(None, default), ("0", 0), ("48", 48), ("-3", -3)]
    if kind == "float":
        return [(None, default), ("2.5", 2.5), ("61", 61.0)]
    return [(None, default), ("", ""), ("slab", "slab"), ("64,160,160,128", "64,160,160,128")]


@pytest.mark.parametrize("row", [r for r in driver_table() if r[1] != "import"], ids=lambda r: r[0])
def test_driver_switch_values(clean_env, row):
    from x3d2_amd.switches import Switches
    name, kind, default, meaning = row
    assert meaning and "\n" not in meaning
    attr = name[len("X3D_"):].lower()
    for value, want in driver_cases(kind, default):
        if value is None:
            clean_env.delenv(name, raising=False)
        else:
            clean_env.setenv(name, value)
        got = getattr(Switches.from_env(), attr)
        assert got == want and type(got) is type(want), (name, value, got)


def test_driver_snapshot_is_fixed_and_closed(clean_env):
    from x3d2_amd.switches import Switches
    clean_env.setenv("X3D_NO_DEFER", "1")
    clean_env.setenv("X3D_SLAB_PARTS", "3")
    sw = Switches.from_env()
    clean_env.delenv("X3D_NO_DEFER")
    clean_env.setenv("X3D_SLAB_PARTS", "5")
    clean_env.setenv("X3D_NO_EPI3", "1")
    assert sw.no_defer is True and sw.slab_parts == 3 and sw.no_epi3 is False  # the environment moved on, the snapshot did not
    later = Switches.from_env()
    assert later.no_defer is False and later.slab_parts == 5 and later.no_epi3 is True
    with pytest.raises(AttributeError):
        sw.no_such_switch
    with pytest.raises(AttributeError):
        sw.no_circ  # (the library's: HipBackend.lib_switch asks x3d_backend_switch)
    with pytest.raises(AttributeError):
        sw.single_prec  # (import-time, _lib.SINGLE)
    with pytest.raises(AttributeError):
        sw.no_defer = False
    with pytest.raises(AttributeError):
        del sw.no_defer
    with pytest.raises(AttributeError):
        sw.new_name = 1
