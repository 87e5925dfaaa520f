"""worker of the two-rank budgets test (tests/test_hip_budgets.py): N processes share cuda:0 and exchange through gloo
(host-staged), like tests/mp_stats_worker.py.  Every rank takes n samples of its part of the same global random fields
through Budgets.sample along y and saves the global running profile it holds."""
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
    layout = tuple(int(x) for x in sys.argv[2].split(","))
    n, out = int(sys.argv[3]), sys.argv[4]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    rank, size = dist.get_rank(), dist.get_world_size()
    assert int(np.prod(layout)) == size
    import test_hip_budgets as t
    from x3d2_amd.budgets import Budgets, BudgetsConfig, MOMENT_NAMES
    from x3d2_amd.common import VERT
    from x3d2_amd.parallel import Comm
    b = t.make_backend(dims, t.WALL, nproc_dir=layout, rank=rank, comm=Comm())
    s = t.Fields(b)
    lo = [int(v) for v in b.mesh.n_offset]
    nl = [int(v) for v in b.mesh.get_dims(VERT)]
    cut = (slice(lo[2], lo[2] + nl[2]), slice(lo[1], lo[1] + nl[1]), slice(lo[0], lo[0] + nl[0]))
    bud = Budgets(s, BudgetsConfig(initbud=1, profile_dir=2))
    for it in range(1, n + 1):
        s.set([np.ascontiguousarray(a[cut]) for a in t.sample_arrays(dims, 7000 + it)])
        bud.sample(s.u, s.v, s.w, s.p, s.grads, t.P_SCALE)
    assert bud.sample_count == n
    np.savez(out + ".%d.npz" % rank, prof=np.stack([bud.moments()[k] for k in MOMENT_NAMES]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
