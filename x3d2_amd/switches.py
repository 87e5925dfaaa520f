"""The driver's environment switches: the one table of their names and the one place that reads the environment.

A switch is read when its owner is constructed -- HipBackend takes `self.sw = Switches.from_env()`, and the solver, the
cases, the Poisson solvers and the block allocator read `backend.sw`; Comm and Ibm, which are built without a backend, take
a snapshot of their own -- and never in a method that runs per step.  The library's switches (csrc/switches.hip) follow
the same rule per x3d_backend; Python asks for them through HipBackend.lib_switch.

Kinds: "flag" is True when the value is exactly "1"; "int" / "float" / "str" give the value converted, or the default
when the variable is not set (None: the reader has a default of its own); "import" is read once by _lib.py when the
package is imported (it selects the library that is loaded) and is not part of a snapshot."""
import os

TABLE = (
    # name, kind, default, meaning
    ("X3D_SINGLE_PREC", "import", False, "load the FP32 flavour of the library (libx3d2_hip_sp.so)"),
    ("X3D_LAZY", "flag", False, "HipBackend(lazy=None): deferred execution of the op-granular call sequence"),
    ("X3D_COMM_RESERVE_CUS", "int", 0, "CUs the persistent kernels leave free for communication kernels"),
    ("X3D_EMULATE_DECOMP", "str", "", "directions (y, z, yz) treated as decomposed on one rank"),
    ("X3D_EMULATE_ALIAS", "flag", False, "emulated slab solvers: receive buffers alias the send buffers (no stand-in copies)"),
    ("X3D_PACK_Z_HALOS", "flag", False, "z halo rows through a pack kernel instead of straight out of the block"),
    ("X3D_NO_HALO_TILE", "flag", False, "decomposed directions: the distributed two-sweep kernels, not the HALO tile forms"),
    ("X3D_NO_YPERM", "flag", False, "channel: y rows permuted by copies, not inside the z pair kernels"),
    ("X3D_BLOCK_STAGGER", "int", None, "elements between the start offsets of consecutive blocks (field.Allocator.STAGGER)"),
    ("X3D_EPI3_STAGES", "str", None, "RK / AB stages that run as the epilogue of the three-in-one z launch"),
    ("X3D_NO_ROT_FUSED", "flag", False, "rotation and mean shift as separate launches"),
    ("X3D_NO_DEFER", "flag", False, "no deferred accumulation of the transeq terms into the stage's linear combination"),
    ("X3D_NO_EPI3", "flag", False, "the stage not as the epilogue of the three-in-one z launch"),
    ("X3D_NO_RK_RUNSUM", "flag", False, "RK stages in the z launch store the derivatives, not the running sum of the final combination"),
    ("X3D_STAGE_IN_TILE", "flag", False, "the stage in the per-component z tile kernel"),
    ("X3D_NO_DEFER_GRAD", "flag", False, "pressure gradient applied at once, not folded into the next x launch"),
    ("X3D_NO_DEFER_WALLS", "flag", False, "channel: wall values set by separate launches"),
    ("X3D_NO_MEAN_IN_LINCOMB", "flag", False, "channel: bulk-velocity sum by a reduction of its own"),
    ("X3D_NO_CHANNEL_DEFER_GRAD", "flag", False, "channel: the velocity correction applied by the pressure step instead of the next transeq_x kernel"),
    ("X3D_NO_IBM_SPARSE", "flag", False, "immersed boundary: dense mask multiply"),
    ("X3D_FORCE_PENCIL_FFT", "str", None, "'1': generic pencil Poisson solver, 'slab': z slabs, 'yslab': y slabs"),
    ("X3D_NO_YSLAB_FFT", "flag", False, "never pick the y-slab Poisson solver"),
    ("X3D_NO_SLAB_FFT", "flag", False, "never pick the z-slab Poisson solver"),
    ("X3D_PENCIL_PARTS", "int", 0, "pencil solver: parts its transposes are pipelined in (0: its own choice)"),
    ("X3D_SLAB_PARTS", "int", None, "slab solvers: parts the all-to-all is pipelined in"),
    ("X3D_SLAB_YPARTS", "int", 0, "y-slab solver: groups of y rows"),
    ("X3D_SLAB_ROWS", "str", None, "y-slab solver: uneven groups, e.g. '64,160,160,128'"),
    ("X3D_SLAB_SCHEDULE", "str", None, "y-slab solver: 'blocks' = one exchange per block"),
    ("X3D_SLAB_TAIL", "int", None, "y-slab solver: groups exchanged behind the last transform"),
    ("X3D_NO_OVERLAP", "flag", False, "Comm: every exchange ordered on the compute stream"),
    ("X3D_COMM_SELF_VIA_NCCL", "flag", False, "Comm, world size 1: exchanges with this rank through RCCL"),
    ("X3D_COMM_FAKE_PEERS", "flag", False, "Comm, world size 1: every peer of an all-to-all is this rank"),
    ("X3D_COMM_EMULATE_LINKS", "str", None, "Comm, world size 1: GB/s per emulated link and direction"),
    ("X3D_COMM_EMULATE_LATENCY_US", "float", 30.0, "Comm: microseconds every emulated group holds its stream"),
    ("X3D_COMM_NO_STREAM_PROBE", "flag", False, "Comm: take the first communication stream without probing"),
)
_CONVERT = {"flag": lambda v: v == "1", "int": int, "float": float, "str": str}


def _attr(name):
    return name[len("X3D_"):].lower()


class Switches:
    """immutable snapshot of the driver's switches; `sw.no_defer` is X3D_NO_DEFER, an undeclared name raises"""
    __slots__ = tuple(_attr(name) for name, kind, _, _ in TABLE if kind != "import")

    def __init__(self, values):
        for k in self.__slots__:
            object.__setattr__(self, k, values[k])

    def __setattr__(self, k, v):
        raise AttributeError("Switches is a snapshot: %s cannot be set" % k)

    def __delattr__(self, k):
        raise AttributeError("Switches is a snapshot: %s cannot be deleted" % k)

    @classmethod
    def from_env(cls):
        values = {}
        for name, kind, default, _ in TABLE:
            if kind != "import":
                v = os.environ.get(name)
                values[_attr(name)] = default if v is None else _CONVERT[kind](v)
        return cls(values)

