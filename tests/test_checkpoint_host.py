"""The host side of checkpoints (x3d2_amd/checkpoint.py) without a GPU: configuration and naming, the numpy reference of
the checksums (tests/checkpoint_ref.py), the safe write and the finiteness guard on plain files, and every refusal of
`restore`, against a host stand-in for backend and solver.  All comparisons are of bits or integers."""
import os

import numpy as np
import pytest

import checkpoint_ref as ref
from x3d2_amd.checkpoint import (CheckpointConfig, Checkpoints, checksum_rows, file_name, read_checkpoint, restore,
                                 restart_from_checkpoint, state_fields)
from x3d2_amd.common import X3dError


# ---------------------------------------------------------------- configuration and naming
def test_config_defaults_are_the_reference_s():
    c = CheckpointConfig()
    assert (c.checkpoint_freq, c.checkpoint_prefix, c.keep_checkpoint, c.restart_from_checkpoint, c.restart_file) == \
        (0, "checkpoint", True, False, "")


def test_due():
    assert not any(CheckpointConfig().due(it) for it in range(0, 7))
    c = CheckpointConfig(checkpoint_freq=3)
    assert [it for it in range(1, 10) if c.due(it)] == [3, 6, 9]
    assert not CheckpointConfig(checkpoint_freq=-2).due(4)


def test_file_names_for_one_and_several_ranks():
    assert file_name("ck", 3) == "ck_000003.npz"
    assert file_name("out/ck", 123456, nproc=1) == "out/ck_123456.npz"
    assert file_name("ck", 3, nproc=2, nrank=1) == "ck_000003.r1.npz"
    assert file_name("ck", 3, tag=".nonfinite") == "ck_000003.nonfinite.npz"
    assert file_name("ck", "temp") == "ck_temp.npz" and file_name("ck", "temp", 4, 2) == "ck_temp.r2.npz"
    ck = Checkpoints(ref.StubSolver(nproc_dir=(1, 2, 1), nrank=1), CheckpointConfig(checkpoint_prefix="p"))
    assert ck._file_name(12) == "p_000012.r1.npz"


# ---------------------------------------------------------------- the checksums
def test_reference_table_on_hand_made_arrays():
    one = np.array([-1.0, -2.0, 1.0])
    b = [0xBFF0000000000000, 0xC000000000000000, 0x3FF0000000000000]
    s1 = sum(b) % 2 ** 64
    s2 = (b[0] * 1 + b[1] * 3 + b[2] * 5) % 2 ** 64
    assert [int(v) for v in ref.table_row(one)] == [s1, s2, 0]
    assert sum(b) >= 2 ** 64  # (the sum did wrap)
    f = np.array([1.0, np.nan, np.inf, -np.inf, 3.0], dtype=np.float32)
    row = ref.table_row(f)
    fb = [int(v) for v in f.view(np.uint32)]  # zero-extended: no wrap in s1 at this length
    assert int(row[0]) == sum(fb) and int(row[1]) == sum(v * (2 * i + 1) for i, v in enumerate(fb)) and int(row[2]) == 3
    for a in (one, f, np.random.default_rng(1).standard_normal((3, 4, 5))):
        assert np.array_equal(checksum_rows(a), ref.table_row(a))  # the package's host form is the same function


def test_a_swapped_pair_keeps_s1_and_changes_s2():
    a = np.random.default_rng(2).standard_normal(40)
    c = a.copy()
    c[[7, 29]] = c[[29, 7]]
    ra, rc = ref.table_row(a), ref.table_row(c)
    assert ra[0] == rc[0] and ra[1] != rc[1] and ra[2] == rc[2] == 0
    d = a.copy()
    d[11] = np.nan
    assert ref.table_row(d)[2] == 1 and ref.table_row(d)[0] != ra[0]


# ---------------------------------------------------------------- files
def make(tmp_path, keep=True, **kw):
    s = ref.StubSolver(**kw)
    s.randomise(5)
    case = ref.StubCase(s)
    ck = Checkpoints(s, CheckpointConfig(checkpoint_freq=3, checkpoint_prefix=str(tmp_path / "ck"), keep_checkpoint=keep), case)
    return s, case, ck


def test_write_poll_and_the_file(tmp_path):
    s, case, ck = make(tmp_path, time_intg="AB3", n_species=1)
    assert not ck.write(2) and ck.ring.allocated == 0  # idle: no buffer
    s.backend.landed = False
    assert ck.write(3) and s.flushes == 1 and ck.poll() == [] and ck.files == []
    s.backend.landed = True
    name = str(tmp_path / "ck_000003.npz")
    assert ck.poll() == [name] and ck.poll() == [] and os.listdir(tmp_path) == ["ck_000003.npz"]  # no _temp file left
    z = read_checkpoint(name)
    names = [str(n) for n in z["names"]]
    assert names == ["u", "v", "w", "phi_1"] + ["%s_rhs_old%d" % (v, j) for v in ("u", "v", "w", "phi_1") for j in (1, 2)]
    assert names == [k for k, _ in state_fields(s)]
    for k, f in zip(names, s.fields()):
        assert z[k].tobytes() == f.a.tobytes() and z[k].shape == (3, 4, 5)
    assert np.array_equal(z["checksums"], ref.table([f.a for f in s.fields()]))
    assert int(z["timestep"]) == 3 and float(z["time"]) == 3 * s.dt and int(z["ti_order"]) == 3 and bool(z["ti_is_ab"])
    assert int(z["precision"]) == 8 and tuple(z["dims"]) == (5, 4, 3) and int(z["case_noise_draws"]) == 7
    # a second checkpoint before the first was written waits for it
    s.backend.landed = False
    assert ck.write(6) and s.backend.waits == 0
    assert ck.write(9) and s.backend.waits == 1 and ck.files[-1].endswith("ck_000006.npz")
    assert ck.finalise() == [str(tmp_path / "ck_000009.npz")] and ck.finalise() == []


def test_nonfinite_file_keeps_the_predecessor(tmp_path):
    s, case, ck = make(tmp_path, keep=False)
    ck.write(3)
    ck.poll()
    s.w.a[1, 2, 3] = np.nan
    ck.write(6)
    assert ck.poll() == [str(tmp_path / "ck_000006.nonfinite.npz")]
    assert sorted(os.listdir(tmp_path)) == ["ck_000003.npz", "ck_000006.nonfinite.npz"]
    z = read_checkpoint(ck.files[-1])
    assert [int(v) for v in z["checksums"][:, 2]] == [0, 0, 1] + [0] * 6
    assert ck.last_good == str(tmp_path / "ck_000003.npz")


def test_keep_checkpoint_false_removes_exactly_the_predecessor(tmp_path):
    s, case, ck = make(tmp_path, keep=False)
    other = tmp_path / "ck_000001.npz"
    other.write_bytes(b"somebody else's")
    for it in (3, 6, 9):
        ck.write(it)
        ck.poll()
    assert sorted(os.listdir(tmp_path)) == ["ck_000001.npz", "ck_000009.npz"]
    s2, case2, ck2 = make(tmp_path, keep=True)
    ck2.cfg.checkpoint_prefix = str(tmp_path / "keep")
    for it in (3, 6):
        ck2.write(it)
        ck2.poll()
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("keep")) == ["keep_000003.npz", "keep_000006.npz"]


# ---------------------------------------------------------------- restore
def written(tmp_path, **kw):
    s, case, ck = make(tmp_path, **kw)
    s.time_integrator.istep, s.time_integrator.gdt = 4, 0.25
    ck.write(3)
    return s, ck.finalise()[0]


def rewrite(path, **changes):
    z = read_checkpoint(path)
    z.update(changes)
    np.savez(path, **z)


def test_restore_round_trip(tmp_path):
    s, path = written(tmp_path, time_intg="AB3", n_species=1)
    t = ref.StubSolver(time_intg="AB3", n_species=1)
    case = ref.StubCase(t)
    case.state = {}
    cfg = CheckpointConfig(restart_from_checkpoint=True, restart_file=path)
    assert restart_from_checkpoint(case, CheckpointConfig()) is None and t.backend.unpacked == 0
    assert restart_from_checkpoint(case, cfg) == 3
    for f, g in zip(s.fields(), t.fields()):
        assert f.a.tobytes() == g.a.tobytes()
    ti = t.time_integrator
    assert (t.current_iter, ti.istep, ti.nstep, ti.gdt, case.restarted) == (3, 4, 3, 0.25, True)
    assert int(case.state["noise_draws"]) == 7


@pytest.mark.parametrize("what,other,word", [
    ("dims", dict(dims=(5, 4, 4)), "dims"),
    ("order", dict(time_intg="AB2"), "ti_order"),
    ("family", dict(time_intg="RK3"), "ti_is_ab"),
    ("species", dict(n_species=1), "n_species"),
    ("decomposition", dict(nproc_dir=(1, 2, 1)), "global_dims"),
])
def test_restore_refuses_what_does_not_fit(tmp_path, what, other, word):
    s, path = written(tmp_path, time_intg="AB3")
    t = ref.StubSolver(**dict(dict(time_intg="AB3"), **other))
    with pytest.raises(X3dError, match=word):
        restore(ref.StubCase(t), path)
    assert t.backend.unpacked == 0 and t.current_iter == 0 and not np.any(t.u.a)


def test_restore_refuses_the_other_precision(tmp_path):
    s, path = written(tmp_path)
    rewrite(path, precision=np.int64(4))
    t = ref.StubSolver()
    with pytest.raises(X3dError, match="precision"):
        restore(ref.StubCase(t), path)
    assert t.backend.unpacked == 0


def test_restore_refuses_a_truncated_file(tmp_path):
    s, path = written(tmp_path)
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:len(raw) // 2])
    t = ref.StubSolver()
    with pytest.raises(X3dError, match="ck_000003.npz"):
        restore(ref.StubCase(t), path)
    assert t.backend.unpacked == 0


def test_restore_finds_one_flipped_bit_in_v(tmp_path):
    s, path = written(tmp_path)
    v = read_checkpoint(path)["v"].copy()
    v.view(np.uint64)[1, 2, 3] ^= np.uint64(1) << np.uint64(17)
    rewrite(path, v=v)  # (a well-formed file: the archive's own CRC does not see it, the table must)
    t = ref.StubSolver()
    with pytest.raises(X3dError, match="`v`"):
        restore(ref.StubCase(t), path)
    assert t.backend.unpacked == 0 and t.current_iter == 0 and not np.any(t.v.a)
    # ... and in the raw bytes of the file as it lies on disk (the archive notices, or the table does)
    s, path = written(tmp_path)
    raw = bytearray(open(path, "rb").read())
    at = raw.index(b"v.npy") + 200
    raw[at] ^= 0x10
    open(path, "wb").write(bytes(raw))
    with pytest.raises(X3dError, match="v"):
        restore(ref.StubCase(t), path)
    assert t.backend.unpacked == 0
