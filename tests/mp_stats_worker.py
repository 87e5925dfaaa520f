"""worker of the two-rank statistics test (tests/test_hip_stats.py): N processes share cuda:0 and exchange through gloo
(host-staged), like tests/mp_gpu_worker.py; z slabs.  Every rank takes n samples of its slab of the same global random
fields in the profile mode along y (z reduced over the ranks) and along z (the kept direction is decomposed) and saves
its profiles."""
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
    n, out = int(sys.argv[2]), sys.argv[3]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    rank, size = dist.get_rank(), dist.get_world_size()
    import test_hip_stats as t
    from x3d2_amd.parallel import Comm
    from x3d2_amd.stats import Stats, StatsConfig
    b = t.make_backend(dims, t.WALL, nproc_dir=(1, 1, size), rank=rank, comm=Comm())
    s = t.Fields(b)
    nzl = dims[2] // size
    res = {}
    for dir_keep in (2, 3):
        st = Stats(s, StatsConfig(initstat=1, profile_dir=dir_keep))
        for it in range(1, n + 1):
            s.set([np.ascontiguousarray(a[rank * nzl:(rank + 1) * nzl]) for a in t.sample_arrays(dims, 200 + it)])
            st.update(it)
        for name, a in st.means().items():
            res["d%d_%s" % (dir_keep, name)] = a
    np.savez(out + ".%d.npz" % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
