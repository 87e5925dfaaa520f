"""worker of the two-rank snapshot test (tests/test_hip_snapshot.py): N processes share cuda:0 and exchange through gloo
(host-staged), like tests/mp_stats_worker.py; z slabs.  Every rank holds its slab of the same global random u, v, w and
writes one snapshot of iteration 3 with the given stride: `<out>_000003.r<rank>.npz`."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    dims = tuple(int(x) for x in sys.argv[1].split(","))
    stride = tuple(int(x) for x in sys.argv[2].split(","))
    out = sys.argv[3]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    rank, size = dist.get_rank(), dist.get_world_size()
    import test_hip_stats as t
    from x3d2_amd.parallel import Comm
    from x3d2_amd.snapshot import SnapshotConfig, Snapshots
    b = t.make_backend(dims, t.WALL, nproc_dir=(1, 1, size), rank=rank, comm=Comm())
    s = t.Fields(b)
    s.dt = 1e-3  # (the part of Solver that Snapshots reads beyond what Stats does: `time` = it * dt)
    nzl = dims[2] // size
    rng = np.random.default_rng(31)
    arrays = [rng.standard_normal((dims[2], dims[1], dims[0]), dtype=np.float32).astype(np.float64) for _ in range(3)]
    s.set([np.ascontiguousarray(a[rank * nzl:(rank + 1) * nzl]) for a in arrays])
    snap = Snapshots(s, SnapshotConfig(snapshot_freq=3, snapshot_prefix=out, output_stride=stride))
    assert not snap.write(2) and snap.write(3)
    assert snap.finalise() == ["%s_000003.r%d.npz" % (out, rank)]
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
